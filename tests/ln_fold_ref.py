"""Exact references, data, a kernel model and its mutants for the LayerNorm-fold forms of the 8-phase GEMM
(csrc/gemm.hip gemm_bf16_tn_p8<LNM, STO>: mmr_linear_bf16_ln) and for mmr_ln_row_coef, shared by test_ln_fold_cpu.py and
test_ln_fold_gpu.py.  Helpers (rne_bits, bf2f, verify_exact, verify_gelu, gelu_ref_tol, GUARD, SENT, _hash, data) are
gemm_routes_ref's.

The row coefficients are an input of mmr_linear_bf16_ln, so the tests supply them: ra(row) a hashed power of two in
{1/4, 1/2, 1, 2}, rb(row) a hashed multiple of 1/4 in [-4, 4], distinct from row to row, so a coefficient pair read from
the other tile-parity slot, the other 128-row half or another tile's rows changes the output.  x, w, bias and residual
are gemm_routes_ref's exact family (integers in [-4, 4], bias multiples of 1/4, residual integers in [-64, 64]).
  ln_mode 1  v1 = c integers in [-8, 8], bias = d multiples of 1/4: fma(ra, acc, fma(rb, c, d)) is exact (rb c a
             multiple of 1/16 below 2^6, ra acc a multiple of 1/4 below 2^13), the output rne_bits of ra acc + rb c + d
             BIT FOR BIT.  With act = 1: gemm_routes_ref's gelu family (x, w in {-1, 0, 1}, d multiples of 1/8) with ra one
             octave lower, {1/8 .. 1}, and |c| <= 2, so that z = ra acc + rb c + d stays an exact multiple of 1/8 with
             |z| <= ZMAX (asserted), under gelu_ref_tol's 8-phase entries.
  ln_mode 2  v1 = gamma in {1/2, 1, 2}, v2 = beta multiples of 1/4, residual r integers in [-64, 64]:
             fma(gamma, fma(ra, r, rb), beta) and the add to acc + b are exact; rne_bits of acc + b + gamma (ra r + rb)
             + beta BIT FOR BIT.
  ln_mode 0  with statistics, with and without a residual: y bit for bit (round1), and per row and part
             (part p = 4 n_tile + wave column = the columns [16 NT p, 16 NT (p + 1))) the pair (sum, M2) of the STORED
             bf16 outputs.
Statistics bounds, from the kernel's order (epilogue of gemm_bf16_tn_p8, STO):
  sum   each lane adds its 4 NT stored values, sum4 adds the row's four lanes.  The stored values are multiples of 1/4
        (rounding to bf16 only coarsens acc + b + r) below 2^10, at most 64 per part: every partial sum is a multiple
        of 1/4 below 2^16, exact in f32: the part sum equals the f64 sum BIT FOR BIT.
  M2    pm = sum * fl(1 / (16 NT)) = mean (1 + e1), |e1| <= 2^-23 (the rounded constant and the product); d = fl(w - pm)
        carries 2^-24; a lane's chain st2 = fma(d0, d0, fma(d1, d1, st2)) over its 4 NT values adds at most 4 NT
        roundings of a growing sum of non-negative terms, sum4 two more: relative error <= (4 NT + 4) 2^-24 of
        sum (w - pm)^2 = M2 + n_p (pm - mean)^2.  That is inside the bound the suite holds it to,
            |M2 - M2_ref| <= (16 NT + 8) 2^-23 M2_ref + M2_FLOOR(mean),   M2_FLOOR = 2 * 16 NT * (|mean| 2^-23)^2,
        the floor being n_p (pm - mean)^2 (what a constant part, M2_ref = 0, may show), doubled.  model_stats restates
        the order in f32; the CPU test records its worst ratio to the bound, the GPU test records the device's.
mmr_ln_row_coef (two passes over np parts, 8 lanes per row, xor-swap reductions), with u = 2^-24, A = sum |sum_p| / n,
pm_p = sum_p / n_p, D_p = |pm_p - mean|:
  mean    np / 16 + 4 roundings of partial sums bounded by sum |sum_p|:           dmean <= (np / 16 + 5) u A
  d_p     fl(fl(sum_p inv_cnt) - mean):                                           dd_p <= u (|pm_p| + |mean| + D_p) + |pm_p| u + dmean
  var     (cnt dm + m2) / n + eps, dm and m2 chains of np / 16 + 4 roundings:     dvar <= [n_p sum (2 D_p dd_p + dd_p^2)
                                                                                  + (np / 16 + 8) u (n_p sum D_p^2 + sum M2_p)] / n
  rstd    rsqrtf: 2 ulp stated by the HIP math API, = 4 u, + the fma and product:  |drstd| / rstd <= dvar / (2 (var + eps)) + 6 u
  -mean rstd                                                                      <= |mean| rstd (drstd / rstd + u) + dmean rstd
COEF_MARGIN = 2 on both (the device's v_rsq and fused contractions).  Measured worst ratios are recorded by the tests."""
import collections

import numpy as np
import torch

import gemm_routes_ref as G

GUARD, SENT = G.GUARD, G.SENT
SENT_F = float.fromhex("0x1.fa5p+100")            # statistics sentinel: no statistic of these rows equals it
GUARD_ST = 64                                     # guard floats on each side of the statistics
COEF_MARGIN = 2.0
U = 2.0 ** -24

Case = collections.namedtuple("Case", "m n k nt")
_MK = ((256, 128), (768, 384), (4096, 128))
CASES = tuple(Case(m, n, k, nt) for n, nt in ((192, 3), (576, 3), (4416, 3), (256, 4), (4352, 4), (768, 3))
              for m, k in _MK)
# (name, ln_mode, act, residual, statistics): every built combination of the entry point
COMBOS = (("fold", 1, 0, False, False), ("fold_gelu", 1, 1, False, False), ("normres", 2, 0, True, False),
          ("normres_stats", 2, 0, True, True), ("stats", 0, 0, False, True), ("stats_res", 0, 0, True, True))
UNBUILT = ((1, 0, True, False), (1, 0, False, True), (1, 1, True, False), (2, 1, True, False), (0, 0, False, False),
           (0, 0, True, False), (0, 1, False, False))            # (ln_mode, act, residual, statistics)
MUTANTS = ("parity", "half", "vcol", "rbnoc", "gammalate", "prestats", "transpose", "skippair", "m2zero")


def case_id(c):
    return f"nt{c.nt}-{c.m}x{c.n}x{c.k}"


def ln_nt(m, n, cus=G.CUS):
    """The launcher's tile width (64 NT): the one n admits, or by fill of the CUs where both do (ties to 256)."""
    ok3, ok4 = n % 192 == 0, n % 256 == 0
    if not (ok3 and ok4):
        return 4 if ok4 else (3 if ok3 else 0)

    def eff(nt):
        tiles = m // 256 * (n // (64 * nt))
        return tiles / (-(-tiles // cus) * cus)
    return 3 if eff(3) > eff(4) + 1e-9 else 4


def built(c, mode):
    """Whether (case, ln_mode) is built: ln_mode 2 runs 256 x 192 tiles only."""
    return mode != 2 or c.n % 192 == 0


def nt_of(c, mode):
    return 3 if mode == 2 else c.nt


def cut(c):
    return min(c.m, 512), min(c.n, 2 * 64 * c.nt)


# ---------------------------------------------------------------------------------------------- data
def extras(c, act, rows=None, cols=None, device="cpu"):
    """coef (rows, 2) = (ra, rb), v1 for ln_mode 1 (c), gamma, beta: f32."""
    rows, cols = c.m if rows is None else rows, c.n if cols is None else cols
    s = (c.m * 13 + c.n * 29 + c.k * 5 + (3 if act else 0)) % 1000003
    i = torch.arange(rows, dtype=torch.int64, device=device)
    j = torch.arange(cols, dtype=torch.int64, device=device)
    ra = torch.ldexp(torch.ones(rows, device=device), (G._hash(i, 0, s + 1) % 4 - (3 if act else 2)).int())
    rb = (G._hash(i, 0, s + 2) % 33 - 16).float() / 4
    cw = 2 if act else 8
    return {"coef": torch.stack([ra, rb], 1).contiguous(), "c": (G._hash(j, 0, s + 3) % (2 * cw + 1) - cw).float(),
            "gamma": torch.ldexp(torch.ones(cols, device=device), (G._hash(j, 0, s + 4) % 3 - 1).int()),
            "beta": (G._hash(j, 0, s + 5) % 33 - 16).float() / 4}


def pre_f32(mode, acc, b, r, e):
    """The f32 value before the output rounding (exact: every operation below is).  acc f64, b / r f32."""
    ra, rb = e["coef"][:, :1], e["coef"][:, 1:]
    a = acc.float()
    if mode == 1:
        return ra * a + (rb * e["c"] + b)
    v = a + b
    if mode == 2:
        return v + (e["gamma"] * (ra * r + rb) + e["beta"])
    return v if r is None else v + r


def exact_f64(mode, acc, b, r, e):
    ra, rb = e["coef"][:, :1].double(), e["coef"][:, 1:].double()
    if mode == 1:
        return ra * acc + rb * e["c"].double() + b.double()
    v = acc + b.double()
    if mode == 2:
        return v + e["gamma"].double() * (ra * r.double() + rb) + e["beta"].double()
    return v if r is None else v + r.double()


# ---------------------------------------------------------------------------------------------- statistics
def stats_ref(bits16, nt):
    """Stored bf16 outputs (rows, n) int16 -> (sum, M2, mean) per part in f64, each (rows, parts)."""
    y = G.bf2f(bits16).double()
    p = y.view(y.shape[0], -1, 16 * nt)
    mean = p.mean(-1)
    return p.sum(-1), ((p - mean[..., None]) ** 2).sum(-1), mean


def m2_tol(m2_ref, mean, nt):
    return (16 * nt + 8) * 2.0 ** -23 * m2_ref + 2 * 16 * nt * (mean.abs() * 2.0 ** -23) ** 2


def verify_stats(sbuf, bits16, nt):
    """sbuf: GUARD_ST + rows * parts * 2 + GUARD_ST f32 -> (guards intact, slots never written, part sums != the f64 sum
    of the stored outputs, worst |M2 - ref| / tol)."""
    rows = bits16.shape[0]
    mid = sbuf[GUARD_ST:sbuf.numel() - GUARD_ST].view(rows, -1, 2)
    s, m2, mean = stats_ref(bits16, nt)
    ok = bool((sbuf[:GUARD_ST] == SENT_F).all() and (sbuf[sbuf.numel() - GUARD_ST:] == SENT_F).all())
    ratio = (mid[..., 1].double() - m2).abs() / m2_tol(m2, mean, nt).clamp(min=1e-300)
    ratio = torch.where((mid[..., 1].double() == m2), torch.zeros_like(ratio), ratio)
    worst = float("nan") if bool(torch.isnan(ratio).any()) else ratio.max().item()
    return ok, int((mid == SENT_F).sum()), int((mid[..., 0].double() != s).sum()), worst


def stats_pass(res):
    return res[0] and res[1] == 0 and res[2] == 0 and res[3] <= 1.0


def model_stats(vals, nt):
    """The kernel's order in f32 on the values the statistics are taken of (rows, n) f32 -> (rows, parts, 2) f32.
    Lane fq of a row holds, per n-tile j of the part, the columns 16 j + 4 fq .. + 3 as the pairs (w0, w1), (w2, w3)."""
    f = np.float32
    w = vals.numpy().astype(f).reshape(vals.shape[0], -1, nt, 4, 4)              # (row, part, j, fq, e)
    st1 = np.zeros(w.shape[:2] + (4,), f)
    for j in range(nt):
        st1 = st1 + ((w[:, :, j, :, 0] + w[:, :, j, :, 1]) + (w[:, :, j, :, 2] + w[:, :, j, :, 3]))

    def sum4(v):                                                                 # lanes fq ^ 2, then fq ^ 1
        return (v[..., 0] + v[..., 2]) + (v[..., 1] + v[..., 3])
    s = sum4(st1)
    pm = s * f(1.0 / (16 * nt))
    st2 = np.zeros_like(st1)
    for j in range(nt):
        for e0 in (0, 2):
            d0, d1 = w[:, :, j, :, e0] - pm[..., None], w[:, :, j, :, e0 + 1] - pm[..., None]
            inner = (d1.astype(np.float64) * d1 + st2).astype(f)                 # fmaf: one rounding
            st2 = (d0.astype(np.float64) * d0 + inner).astype(f)
    return torch.from_numpy(np.stack([s, sum4(st2)], -1))


# ---------------------------------------------------------------------------------------------- kernel model
def model(c, mode, act, x, w, b, r, e, stats, mutant=None):
    """-> (the (rows + 2 GUARD, cols) int16 output buffer, the statistics buffer with guards or None)."""
    rows, cols = x.shape[0], w.shape[0]
    nt = nt_of(c, mode)
    tn = 64 * nt
    acc = G.preact(x, w)
    e = dict(e)
    ri = torch.arange(rows)
    if mutant == "parity" and rows > 256:
        e["coef"] = e["coef"][(ri - 256) % rows]                   # the slot still holds the previous tile's rows
    if mutant == "half":
        e["coef"] = e["coef"][ri ^ 128]
    if mutant == "vcol":
        sh = (torch.arange(cols) + tn) % cols
        e["c"], e["gamma"], e["beta"] = e["c"][sh], e["gamma"][sh], e["beta"][sh]
    if mutant == "rbnoc":
        e["c"] = torch.ones_like(e["c"])
    if mutant == "gammalate" and mode == 2:
        ra, rb = e["coef"][:, :1], e["coef"][:, 1:]
        v = (acc.float() + b) + e["gamma"] * ((ra * r + rb) + e["beta"])
    else:
        v = pre_f32(mode, acc, b, r, e)
    if act:
        v = torch.from_numpy(G.gelu_fast_np(v.numpy(), "fast2", np.float32))
    out = G.rne_bits(v)
    buf = torch.full((rows + 2 * GUARD, cols), SENT, dtype=torch.int16)
    buf[GUARD:GUARD + rows] = out
    if not stats:
        return buf, None
    st = model_stats(v if mutant == "prestats" else G.bf2f(out), nt)
    parts = st.shape[1]
    if mutant == "m2zero":
        st[..., 1] = (G.bf2f(out).double().view(rows, parts, -1) ** 2).sum(-1).float()
    if mutant == "transpose" and parts > 4:                        # part index wc * tiles_n + n_tile
        p = torch.arange(parts)
        st = st[:, (p % (parts // 4)) * 4 + p // (parts // 4)]
    if mutant == "skippair":
        st[rows - 1, parts - 1] = SENT_F
    sbuf = torch.full((rows * parts * 2 + 2 * GUARD_ST,), SENT_F)
    sbuf[GUARD_ST:GUARD_ST + rows * parts * 2] = st.reshape(-1)
    return buf, sbuf


# ---------------------------------------------------------------------------------------------- mmr_ln_row_coef
COEF_CASES = tuple((m, nparts, fam, eps) for nparts in (4, 16, 36, 48) for m in (1, 7, 256)
                   for fam, eps in (("gauss", 1e-12), ("bigmean", 1e-5), ("constant", 1e-12), ("constant", 1e-5)))


def coef_parts(m, nparts, fam, n_p=48, seed=0):
    """Parts built by the test: rows of n = nparts * n_p bf16-like values -> (stats (m, nparts, 2) f32, the f64 values)."""
    g = torch.Generator().manual_seed(1000 * nparts + 10 * m + seed)
    y = torch.randn(m, nparts * n_p, generator=g, dtype=torch.float64) * (torch.rand(m, 1, generator=g, dtype=torch.float64) * 4 + 0.5)
    if fam == "bigmean":
        y = y + 1e3 * (torch.rand(m, 1, generator=g, dtype=torch.float64) + 0.5) * y.std(1, keepdim=True)
    if fam == "constant":
        y = torch.ones_like(y) * torch.randn(m, 1, generator=g, dtype=torch.float64)
    y = y.to(torch.bfloat16).double()
    p = y.view(m, nparts, n_p)
    mean = p.mean(-1)
    st = torch.stack([p.sum(-1), ((p - mean[..., None]) ** 2).sum(-1)], -1).float()
    return st, y


def coef_ref_tol(st, n, eps):
    """f64 coefficients of the f32 parts as given (Chan's merge) and the bound of the docstring."""
    m, nparts, _ = st.shape
    s, m2 = st[..., 0].double(), st[..., 1].double()
    n_p = n // nparts
    mean = s.sum(1) / n
    pm = s / n_p
    D = (pm - mean[:, None]).abs()
    var = (n_p * (D ** 2).sum(1) + m2.sum(1)) / n
    rstd = 1 / torch.sqrt(var + eps)
    ref = torch.stack([rstd, -mean * rstd], 1)
    A = s.abs().sum(1) / n
    dmean = (nparts / 16 + 5) * U * A
    dd = U * (pm.abs() + mean.abs()[:, None] + D) + pm.abs() * U + dmean[:, None]
    dvar = (n_p * (2 * D * dd + dd ** 2).sum(1) + (nparts / 16 + 8) * U * (n_p * (D ** 2).sum(1) + m2.sum(1))) / n
    rel = dvar / (2 * (var + eps)) + 6 * U
    tol = torch.stack([rstd * rel, mean.abs() * rstd * (rel + U) + dmean * rstd], 1) * COEF_MARGIN
    return ref, tol


def model_coef(st, n, eps):
    """ln_row_coef restated in f32 (8 lanes per row, two parts per lane and step, xor-swap reductions)."""
    f = np.float32
    m, nparts, _ = st.shape
    p = st.numpy().astype(f)
    inv_n = f(1.0) / f(n)
    cnt, inv_cnt = f(1.0) / (inv_n * f(nparts)), inv_n * f(nparts)

    def xor_reduce(v):                                       # v (m, 8)
        for o in (1, 2, 4):
            v = v + v[:, np.arange(8) ^ o]
        return v[:, 0]
    s1 = np.zeros((m, 8), f)
    for sub in range(8):
        for q in range(2 * sub, nparts, 16):
            s1[:, sub] = s1[:, sub] + (p[:, q, 0] + p[:, q + 1, 0])
    mean = xor_reduce(s1) * inv_n
    m2, dm = np.zeros((m, 8), f), np.zeros((m, 8), f)
    for sub in range(8):
        for q in range(2 * sub, nparts, 16):
            d0, d1 = p[:, q, 0] * inv_cnt - mean, p[:, q + 1, 0] * inv_cnt - mean
            m2[:, sub] = m2[:, sub] + (p[:, q, 1] + p[:, q + 1, 1])
            inner = (d1.astype(np.float64) * d1 + dm[:, sub]).astype(f)
            dm[:, sub] = (d0.astype(np.float64) * d0 + inner).astype(f)
    var = ((cnt.astype(np.float64) * xor_reduce(dm) + xor_reduce(m2)).astype(f) * inv_n + f(eps)).astype(f)
    rstd = (f(1.0) / np.sqrt(var.astype(np.float64))).astype(f)
    return torch.from_numpy(np.stack([rstd, -mean * rstd], 1))
