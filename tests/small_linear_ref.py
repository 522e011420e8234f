"""Plain-torch f64 references, per-element tolerances, input families, f32 models and their mutants for the linears
outside the tiled GEMM and the f32 row kernels of the x3 mode (csrc/tower.hip linear_f32, csrc/linear_x3.hip
linear_x3, csrc/gemm_rw.hip gemm_rw, csrc/x3.hip x3_bert_embed / x3_mean_rows / x3_gather_rows), shared by
test_small_linear_cpu.py and test_small_linear_gpu.py.  bits, bf16_rn, _gen, measure and bit_share are rowwise_ref's.

Reference.  ref = act(x w^T + bias) (+ r) in f64 on the operand the kernel forms (f32 or bf16 inputs widened, erf
GELU, the residual added after the activation).  With A = |x| |w|^T, S = A + |bias|, z the pre-activation, all f64:
  linear_f32   pre = n 2^-24 S, n = 16 ceil(cin / 128) + 7 + 2: the roundings on the longest path of the kernel's
               own sum (the products of one wave's chain, per = ceil(cin / 16 / 8) k-steps of 16; the 7 adds over the
               waves' partials; bias and residual)
  linear_x3    pre = n 2^-24 S + 3 2^-18 (1 + 2^-8) A, n = 3 cin / NW + NW + 2.  The second term is the split:
               |x - hi| <= 2^-9 |x|, |lo - (x - hi)| <= 2^-18 |x|, the lo lo product dropped.  n counts one rounding
               per product, which holds for any order inside an MFMA.
  no act       tol = pre + 2 2^-24 |ref|
  GELU         tol = 1.13 pre + 0.75e-7 |z| + 4 2^-24 |gelu(z)| + 2 2^-24 |ref|   (1.13 >= max |gelu'|; 0.75e-7 |z| is
               half of Abramowitz-Stegun 7.1.26's |erf error| <= 1.5e-7, the form common.h erf_as evaluates, times |z|;
               the pre-activation term enters once, amplified, not a second time beside its amplified self)
  linear_rw    tol = 2^-8 |ref| + (K + 3) 2^-24 (S + |r|), and >= BIT_SHARE of a case's elements equal bf16_rn(ref)
These bounds assume the worst summation order and are loose for long cin.  The sharp checks are the exact families,
which must come out bit for bit (without GELU; with it they are held to the bound):
  integer   x, w, bias, r small integers: every product and every partial sum in any order is exact in f32; linear_rw
            gives bf16_rn of the exact value.  A dropped, doubled or misplaced product changes bits.
  onehot    x = I (row b = e_b, b over every k of the case: the first and last k of every wave's range and of every
            chunk among them): y[b][o] = fl32(fl32(w[o][b] + bias[o]) + r[b][o]), the two adds single IEEE f32
            operations of the epilogue.  For linear_x3 w carries 16 significant bits, so hi + lo = w exactly and the
            expected value f32(hi + lo) does not depend on how an MFMA rounds a sum.  Pins the k permutation of the
            operand loads, the K split over the waves and the clamped chunk tail.
  split     linear_x3: x = hi + lo and w = hi + lo, hi in +-{1, 2, 3}, lo in {-1, 0, 1} 2^-10; the kernel's split
            reproduces these parts and sum |terms| < 2^14, so the three-term sum is exact in any order: expected is
            hi hi + hi lo + lo hi (+ bias + r, integers), not x w, which differs by the lo lo term.
  gauss     x ~ N, w ~ N cin^-1/2, bias ~ N, r ~ N: the per-element bounds.
  rowscale  gauss with row b of x and r scaled by 2^(b mod 9 - 4): a row read from, or written to, a neighbouring
            row is wrong by a factor of at least 2.

f32 models (the kernels' summation structure: K split over the waves, k-steps in order with one rounding per MFMA,
the partials added in wave order, bias, GELU through erf_as, residual) must stay within MODEL_F32 / MODEL_X3 /
MODEL_RW of the bounds on every case of the GPU file and reproduce the exact families bit for bit
(test_small_linear_cpu.py).  The shares are the largest err / tol the models reach against the f64 reference, rounded
up to the next 0.05; an input that breaks a share is changed, never the bound.

Mutants of the models and the family that catches each at every case where it is a mutant at all (CAUGHT_BY):
droptail (the last k-step of the K range skipped), nopart (wave NW - 1's partial left out), biastile (bias indexed by
the column inside the 32-wide tile), resstride (residual read with ldy instead of ldr), bias0 (batched: every
problem reads problem 0's bias), actlate (GELU after the residual), nolohi (x3: lo hi dropped), lolo (x3: a fourth
lo lo term), trunc (rw: truncating bf16 store), chan (rw: two channels of a tile swapped), tanh (tanh-form GELU)."""
import torch

import rowwise_ref as R
from rowwise_ref import BIT_SHARE, U24, _gen, bf16_rn, bit_share, bits, measure  # noqa: F401  (re-exported)

FAMILIES = ("integer", "onehot", "split", "gauss", "rowscale")
EXACT = ("integer", "onehot", "split")
MODEL_F32, MODEL_X3, MODEL_RW, MODEL_MEAN = 0.5, 0.5, 1.0, 0.35
CAUGHT_BY = {"droptail": "onehot", "nopart": "onehot", "biastile": "integer", "resstride": "integer", "bias0": "integer",
             "actlate": "gauss", "nolohi": "split", "lolo": "split", "trunc": "integer", "chan": "integer",
             "tanh": "onehot"}
MUTANTS = {"f32": ("droptail", "nopart", "biastile", "resstride", "bias0", "actlate", "tanh"),
           "x3": ("droptail", "nopart", "biastile", "resstride", "bias0", "actlate", "nolohi", "lolo", "tanh"),
           "rw": ("droptail", "biastile", "trunc", "chan")}

# ---- the cases of the GPU file (test_small_linear_cpu.py runs the models over the same lists)
LIN_B = (1, 31, 32, 33, 70)
X3_CIN, X3_COUT, X3_PINS = (128, 256, 384, 512, 640, 1536), (32, 96, 160), (4, 8, None)
X3_AUTO4 = (512, 256, 1024)                      # (B, cin, cout): 16 * 32 = 512 tiles take 4 waves unpinned
F32_CIN, F32_COUT = (16, 48, 112, 128, 144, 768, 1552), (32, 96)
EPILOGUES = tuple((a, b, r) for a in (0, 1) for b in (False, True) for r in (False, True))   # (act, bias, residual)
# strides: (name, x column offset inside a buffer of width cin + 8, ldy - cout, ldr - cout or None: r aliases y)
STRIDES = (("xslice", 4, 0, 0), ("ldy", 0, 3, 3), ("ldr", 0, 3, 7), ("alias", 0, 3, None))
STRIDE_SHAPES = {"x3": ((128, 32), (640, 96)), "f32": ((16, 32), (144, 96))}                  # (cin, cout)
STRIDE_B = (33, 70)
BATCH_N = (1, 3, 5)
BATCH_SHAPES = {"x3": ((128, 32), (640, 96)), "f32": ((16, 32), (144, 96), (1552, 32))}
BATCH_B = (1, 33)
RW_NK = ((32, 64), (64, 64), (96, 64), (160, 192), (576, 192), (1152, 192))
RW_M = (1, 31, 32, 33, 261)
RW_PERSISTENT = (1152, 192)
X3_EMBED_C, X3_EMBED_BL = (8, 64, 100, 768, 1000, 1024), ((1, 1), (3, 5), (2, 33))
X3_MEAN_C, X3_MEAN_L, X3_MEAN_B = (1, 255, 257, 768), (1, 49, 128), (1, 3)
X3_GATHER = ((5, 96, 200), (3, 7, 9), (2, 300, 300))                                          # (b, c, ldx)
MAX_GRID_Y = 65535


def families(kind):
    return tuple(f for f in FAMILIES if f != "split" or kind == "x3")


# ---------------------------------------------------------------------------------------------- routes
def x3_nw(cin, cout, b, nbatch=1, pin=None):
    """Waves per tile, as mmr_linear_x3 chooses them."""
    nw = 8 if cin % 256 == 0 and -(-b // 32) * (cout // 32) * nbatch < 512 else 4
    return pin if pin == 4 or (pin == 8 and cin % 256 == 0) else nw


def x3_route(cin, nw):
    """(NW, k-steps of 32 per wave, live steps in the last 3-step chunk)."""
    steps = cin // nw // 32
    return nw, steps, steps - 3 * ((steps - 1) // 3)


def f32_route(cin):
    """k-steps of 16 per wave of linear_f32's 8 waves: per = ceil(nsteps / 8), the tail waves short or idle."""
    nsteps = cin // 16
    per = -(-nsteps // 8)
    return [max(0, min(nsteps, (w + 1) * per) - w * per) for w in range(8)]


def rw_route(n, k, m, cus):
    """mmr_linear_rw's launch: parts, CT, LDS bytes (with bias), workgroups per CU, grid.x, 32-token tiles and tiles
    per wave of the busiest wave."""
    def ok(p, three):
        no = n // p
        return n % p == 0 and no % 32 == 0 and no * k * 2 <= 150 * 1024 and (not three or (no // 32) % 3 == 0)
    parts = next((p for three in (True, False) for p in range(1, n // 32 + 1) if ok(p, three)), 0)
    no = n // parts
    ct = 3 if (no // 32) % 3 == 0 else 2 if (no // 32) % 2 == 0 else 1
    lds = no * k * 2 + no * 4
    per_cu = max(1, min(4, 160 * 1024 // lds))
    tiles = -(-m // 32)
    grid_x = max(1, min(cus * per_cu // parts, -(-tiles // 8)))
    return {"parts": parts, "ct": ct, "lds": lds, "per_cu": per_cu, "grid_x": grid_x, "tiles": tiles,
            "tiles_per_wave": -(-tiles // (grid_x * 8))}


def rw_persistent_m(n, k, cus):
    """M at which every wave of the full grid sweeps twice, the first four own a third tile and the last tile holds
    5 rows."""
    gx = rw_route(n, k, 1 << 40, cus)["grid_x"]
    return 2 * gx * 8 * 32 + 3 * 32 + 5


# ---------------------------------------------------------------------------------------------- inputs
def split_bf16(t):
    """hi = bf16(t), lo = bf16(t - hi), as f32: the kernels' split (ops.X3W for the weights)."""
    hi = bf16_rn(t).float()
    return hi, bf16_rn(t - hi).float()


def lin_inputs(kind, fam, rows, cin, cout, seed):
    """x (rows, cin), w (cout, cin), bias (cout,), r (rows, cout): f32 for kind f32 / x3; bf16 with an f32 bias for
    rw.  onehot: rows = cin whatever is asked."""
    g_ = _gen(7, ("f32", "x3", "rw").index(kind), FAMILIES.index("gauss" if fam == "rowscale" else fam), cin, cout, seed)
    if fam == "onehot":
        rows = cin
    ri = (lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g_).float())
    rn = (lambda *s: torch.randn(*s, generator=g_))
    extra = {}
    if fam == "integer":
        m = 8 if kind == "rw" else 4
        x, w, bias, r = ri(-m, m, rows, cin), ri(-m, m, cout, cin), ri(-8, 8, cout), ri(-8, 8, rows, cout)
    elif fam == "split":
        def part(*s):
            hi = ri(1, 3, *s) * (2 * ri(0, 1, *s) - 1)
            return hi, ri(-1, 1, *s) * 2.0 ** -10          # |lo| below half a bf16 ulp under 1: 2^-9
        (xh, xl), (wh, wl) = part(rows, cin), part(cout, cin)
        x, w, bias, r = xh + xl, wh + wl, ri(-8, 8, cout), ri(-8, 8, rows, cout)
        extra = {"xh": xh, "xl": xl, "wh": wh, "wl": wl}
    else:
        x = torch.eye(cin) if fam == "onehot" else rn(rows, cin)
        w, bias, r = rn(cout, cin) * (1.0 if fam == "onehot" else cin ** -0.5), rn(cout), rn(rows, cout)
        if fam == "onehot" and kind == "x3":
            w = (w.view(torch.int32) & -256).view(torch.float32)          # 16 significant bits: hi + lo = w
        if fam == "rowscale":
            sc = 2.0 ** (torch.arange(rows) % 9 - 4).float()[:, None]
            x, r = x * sc, r * sc
    if kind == "rw":
        x, w, r = bf16_rn(x), bf16_rn(w), bf16_rn(r)
    return {"kind": kind, "fam": fam, "rows": rows, "cin": cin, "cout": cout, "x": x, "w": w, "bias": bias, "r": r,
            **extra}


def products(x, w):
    """(x w^T, |x| |w|^T) in f64: shared by the epilogues of one case."""
    xd, wd = x.double(), w.double()
    return xd @ wd.t(), xd.abs() @ wd.abs().t()


def gelu_f64(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


def n_roundings(kind, cin, nw=None):
    return 16 * -(-cin // 128) + 7 + 2 if kind == "f32" else 3 * cin // nw + nw + 2


def lin_ref(kind, P, A, bias, r, act, cin, nw=None):
    """(ref, tol) in f64 from products(x, w); bias / r None or tensors; rows may be a prefix of r's."""
    rows = P.shape[0]
    z = P + bias.double() if bias is not None else P
    S = A + bias.double().abs() if bias is not None else A
    rd = r[:rows].double() if r is not None else None
    if kind == "rw":
        ref = z + rd if rd is not None else z
        return ref, 2.0 ** -8 * ref.abs() + (cin + 3) * U24 * (S + (rd.abs() if rd is not None else 0.0))
    pre = n_roundings(kind, cin, nw) * U24 * S
    if kind == "x3":
        pre = pre + 3 * 2.0 ** -18 * (1 + 2.0 ** -8) * A
    if act:
        g = gelu_f64(z)
        t = 1.13 * pre + 0.75e-7 * z.abs() + 4 * U24 * g.abs()
    else:
        g, t = z, pre
    ref = g + rd if rd is not None else g
    return ref, t + 2 * U24 * ref.abs()


def expected_exact(inp, bias_on, res_on, rows=None):
    """The bit-exact expectation of an exact family without GELU (module docstring); None for the others."""
    kind, fam = inp["kind"], inp["fam"]
    rows = inp["rows"] if rows is None else rows
    bias, r = (inp["bias"] if bias_on else None), (inp["r"][:rows] if res_on else None)
    if fam == "onehot":                                # two IEEE f32 adds on the exact w[o][b]
        v = inp["w"].float().t()[:rows]
        v = v + bias if bias is not None else v
        v = v + r.float() if r is not None else v
    elif fam in ("integer", "split"):
        if fam == "split":
            xh, xl, wh, wl = (inp[k].double() for k in ("xh", "xl", "wh", "wl"))
            v = xh[:rows] @ wh.t() + xh[:rows] @ wl.t() + xl[:rows] @ wh.t()
        else:
            v = inp["x"][:rows].double() @ inp["w"].double().t()
        v = v + bias.double() if bias is not None else v
        v = v + r.double() if r is not None else v
        assert torch.equal(v.float().double(), v), "the exact value is not an f32"
        v = v.float()
    else:
        return None
    return bf16_rn(v) if kind == "rw" else v


def abs_term_sum(inp):
    """sum of |terms| of an integer / split case in f64: below 2^24 units of the smallest term, so f32 sums are exact."""
    if inp["fam"] == "split":
        xh, xl, wh, wl = (inp[k].double().abs() for k in ("xh", "xl", "wh", "wl"))
        s = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
    else:
        s = inp["x"].double().abs() @ inp["w"].double().abs().t()
    return s + inp["bias"].double().abs() + inp["r"].double().abs()


# ---------------------------------------------------------------------------------------------- f32 models
def erf_as(x):
    """common.h erf_as restated (Abramowitz-Stegun 7.1.26) in x's dtype."""
    a = x.abs()
    t = 1.0 / (0.3275911 * a + 1.0)
    p = 1.061405429 * t - 1.453152027
    p = p * t + 1.421413741
    p = p * t - 0.284496736
    p = p * t + 0.254829592
    y = 1.0 - p * t * torch.exp2(-1.44269504088896341 * a * a)
    return torch.copysign(y, x)


def gelu_model(v, tanh=False):
    if tanh:
        return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v * v * v)))
    return 0.5 * v * (1.0 + erf_as(v * 0.70710678118654752))


def _acc(acc, d):
    """One MFMA: the exact dot product added to the f32 accumulator with one rounding."""
    return (acc.double() + d).float()


def model_partials(kind, x, w, nw=None, mutant=None):
    """The waves' partial tiles (waves, rows, cout) f32 of linear_f32 (8 waves, 32x32x2 MFMAs over the k pairs
    (k, k + 8) of each 16-wide step) or linear_x3 (NW waves, per 32-wide step hi hi, hi lo, lo hi)."""
    rows, cin = x.shape
    cout = w.shape[0]
    x = x.clone()
    if mutant == "droptail":
        x[:, cin - (16 if kind == "f32" else 32):] = 0
    if kind == "f32":
        per = -(-(cin // 16) // 8)
        pad = 8 * per * 16 - cin
        X = torch.nn.functional.pad(x, (0, pad)).double().view(rows, 8, per, 2, 8)
        W = torch.nn.functional.pad(w, (0, pad)).double().view(cout, 8, per, 2, 8)
        acc = torch.zeros(8, rows, cout)
        for s in range(per):
            for s8 in range(8):
                acc = _acc(acc, torch.einsum("bwh,owh->wbo", X[:, :, s, :, s8], W[:, :, s, :, s8]))
        return acc
    steps = cin // nw // 32
    (xh, xl), (wh, wl) = split_bf16(x), split_bf16(w)
    v = (lambda t: t.double().view(t.shape[0], nw, steps, 32))
    X, W = {"h": v(xh), "l": v(xl)}, {"h": v(wh), "l": v(wl)}
    terms = [("h", "h"), ("h", "l"), ("l", "h")]
    if mutant == "nolohi":
        terms.pop()
    if mutant == "lolo":
        terms.append(("l", "l"))
    acc = torch.zeros(nw, rows, cout)
    for s in range(steps):
        for a, b in terms:
            acc = _acc(acc, torch.einsum("bwk,owk->wbo", X[a][:, :, s], W[b][:, :, s]))
    return acc


def _strided_residual(r, ldr, ldy):
    """r as the kernel would read it with row stride ldy from a buffer that holds it at row stride ldr."""
    rows, cout = r.shape
    buf = 100.0 + (torch.arange(rows * max(ldr, ldy) + cout) % 7).float()
    buf.as_strided((rows, cout), (ldr, 1)).copy_(r)
    return buf.as_strided((rows, cout), (ldy, 1)).clone()


def model_epilogue(parts, bias, r, act, mutant=None, ldr=None, ldy=None):
    """Partials in wave order, bias, GELU, residual: (rows, cout) f32."""
    n = parts.shape[0] - (1 if mutant == "nopart" else 0)
    v = parts[0]
    for wv in range(1, n):
        v = v + parts[wv]
    if bias is not None:
        v = v + (bias[torch.arange(v.shape[1]) % 32] if mutant == "biastile" else bias)
    if act and mutant != "actlate":
        v = gelu_model(v, tanh=mutant == "tanh")
    if r is not None:
        v = v + (_strided_residual(r, ldr, ldy) if mutant == "resstride" else r)
    if act and mutant == "actlate":
        v = gelu_model(v)
    return v


def model_linear(kind, x, w, bias, r, act, nw=None, mutant=None, ldr=None, ldy=None):
    if kind == "rw":
        return model_rw(x, w, bias, r, mutant)
    return model_epilogue(model_partials(kind, x, w, nw, mutant), bias, r, act, mutant, ldr, ldy)


def model_batched(kind, xs, ws, biases, rs, act, nw=None, mutant=None):
    """Lists over the problems -> list of outputs; bias0: every problem reads problem 0's bias."""
    return [model_linear(kind, xs[i], ws[i], None if biases is None else biases[0 if mutant == "bias0" else i],
                         None if rs is None else rs[i], act, nw) for i in range(len(xs))]


def model_rw(x, w, bias, r, mutant=None):
    """gemm_rw: K / 16 MFMAs of 16 k each into one f32 accumulator, + bias, + residual, bf16 store."""
    m, k = x.shape
    xd, wd = x.double().clone(), w.double()
    if mutant == "droptail":
        xd[:, k - 16:] = 0
    acc = torch.zeros(m, w.shape[0])
    for ks in range(k // 16):
        acc = _acc(acc, xd[:, 16 * ks:16 * ks + 16] @ wd[:, 16 * ks:16 * ks + 16].t())
    if bias is not None:
        acc = acc + (bias[torch.arange(acc.shape[1]) % 32] if mutant == "biastile" else bias)
    if r is not None:
        acc = acc + r.float()
    if mutant == "chan":
        acc[:, [3, 12]] = acc[:, [12, 3]]
    if mutant == "trunc":
        return (acc.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return acc.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- x3 row kernels
def x3_embed_case(fam, b, l, c, seed, eps=1e-12):
    """x3_bert_embed: rowwise_ref.embed_case's tables and ids; v32 = (word + type) + pos in f32, the kernel's order;
    f32 output under tol_f32."""
    k = R.embed_case(fam, b, l, c, seed, eps)
    flat, p = k["ids"].view(-1), torch.arange(b * l) % l
    v32 = (k["word"][flat] + k["type0"]) + k["pos"][p]
    ref, xhat, kappa, _ = R.ln_f64(v32, k["g"], k["b"], eps)
    k.update(v32=v32, ref=ref, xhat=xhat, kappa=kappa, tol_f32=R.tol_f32(ref, xhat, kappa, k["g"], k["b"]))
    return k


def x3_mean_case(fam, b, l, c, seed, extra):
    """x3_mean_rows: y = (extra + sum_t x) / (l + 1) or sum_t x / l.  tol = (nt + 1) 2^-24 sum |terms| / nt over the
    nt = l (+ 1) terms: nt - 1 adds and one division, each within 2^-24 of a partial sum <= sum |terms| (for
    extra = None this is mean_tokens' (l + 1) 2^-24 mean_t |x|).  integer: sums exact, the one division correctly
    rounded: expected bit for bit."""
    g_ = _gen(8, c, l, b, seed, int(extra))
    if fam == "integer":
        x = torch.randint(-8, 9, (b, l, c), generator=g_).float()
        e = torch.randint(-8, 9, (b, c), generator=g_).float() if extra else None
    else:
        x = 3 * torch.randn(b, l, c, generator=g_) + 1
        e = 3 * torch.randn(b, c, generator=g_) if extra else None
    nt = l + (1 if extra else 0)
    s, sa = x.double().sum(1), x.double().abs().sum(1)
    if extra:
        s, sa = s + e.double(), sa + e.double().abs()
    exact = (s.float() / torch.tensor(float(nt))) if fam == "integer" else None
    return {"x": x, "extra": e, "ref": s / nt, "tol": (nt + 1) * U24 * sa / nt, "exact": exact}


def model_mean_rows(x, extra):
    b, l, c = x.shape
    s = torch.zeros(b, c)
    for t in range(l):
        s = s + x[:, t]
    return (extra + s) / (l + 1) if extra is not None else s / l
