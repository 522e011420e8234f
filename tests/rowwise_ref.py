"""Plain-torch f64 references, per-element tolerances, input families, an f32 model and its mutants for the
row kernels (csrc/tower.hip layernorm_bf16, bert_embed, patch_merge_ln_g, patch_merge_ln, swin_head, mean_tokens,
l2_normalize_rows; csrc/fusion.hip ln_rows, ln_rows_v, ln_rows_s, add_pos_bf16, assemble_seq, assemble_seq8,
rows_to_f32), shared by test_rowwise_cpu.py and test_rowwise_gpu.py.

Reference.  ln_f64 is LayerNorm in f64 on exactly the operand the kernel forms: bf16 / f32 inputs widened, the
product alpha * x rounded to f32 first (torch's `alpha * x + r`; mul_rn in ln_rows), the sum with the residual
(and of the three embedding rows) taken as the kernel takes it.  It returns ref, xhat = (v - mean) / sigma and
kappa = max|v| / sigma per row, sigma = sqrt(var + eps).

Bounds (constants fixed by the arithmetic, not fitted to the kernels):
  f32_term = 2^-24 (|g| (64 kappa + 16 |xhat|) + 2 (|g xhat| + |b|))
      the f32 error of a two-pass LayerNorm whose row sum is <= 64 serial adds per lane plus a 6-level tree:
      the error of the mean scales with kappa, rsqrtf and the variance add a few ulps of xhat, the final
      multiply and add the rest;
  tol_bf16 = 2^-8 |ref| + f32_term       (half a bf16 ulp is at most 2^-8 |ref|)
  tol_f32  = 2^-23 |ref| + f32_term
  every element: |got - ref| <= tol; bf16 outputs also: >= 99 % of a case's elements equal bf16_rn(ref) bit for
  bit (BIT_SHARE, a cap: the f32 model stays above 0.997).
  post term of ln_rows (+ ps * post, one f32 product and one add): + 2 * 2^-24 |ps post|.
  swin_head: patches = LN(LN(x)): the first stage's tol_f32 (e1) times |g_j| / sigma2 plus the second stage's
  own tol_f32; global = token mean of the first stage: mean_t e1 + t 2^-24 mean_t|u| (t - 1 adds and one division,
  any order); pool = (global + sum_t patches) / (t + 1) likewise.
  mean_tokens: l 2^-24 mean_t|x|.
The f32 model (sequential sums: the worst order) must stay within MODEL_BF16 = 1.0 of tol_bf16 and MODEL_F32 = 0.5
of the f32 bounds on every input the GPU file uses (test_rowwise_cpu.py); an input that does not is changed by
lowering kappa, never the bound.  That is why the `constant` family is not run with alpha (0.7 * 3 is no small
integer, its row sums round, and kappa = 2.1 / sqrt(eps) = 660 turns that into many flipped roundings).

Families, functions of (rows, c, seed): gauss 3 N + 1; bigmean 0.5 N + 40 (kappa ~ 90; a lower mean where the
model's row sums round, see bigmean_offset); tinyvar 0.01 N (variance
1e-4 against eps 1e-5; also run at eps 1e-12); outlier 0.02 N with one element = 30 inside the row's last chunk
of 8; constant 3.0 (row sums exact in f32 up to c = 4096, v - mean = 0, output = beta exactly).
gamma = 1 + 0.5 N, beta = 0.3 N per channel (per group).

Mutants of the model (what the rules must catch): trunc (truncating bf16 store), cm1 (variance / (c - 1)), noeps,
onepass (E[x^2] - mean^2), gshift (gamma / beta read one chunk of 8 further on), cpad (mean = sum / (c + 8))."""
import torch

U24 = 2.0 ** -24
BIT_SHARE = 0.99
MODEL_BF16, MODEL_F32 = 1.0, 0.5
FAMILIES = ("gauss", "bigmean", "tinyvar", "outlier", "constant")
MUTANTS = ("trunc", "cm1", "noeps", "onepass", "gshift", "cpad")
# the family that catches each mutant at every width (test_rowwise_cpu.py asserts it)
CAUGHT_BY = {"trunc": "gauss", "cm1": "gauss", "noeps": "tinyvar", "onepass": "bigmean", "gshift": "gauss",
             "cpad": "bigmean"}

# ---- the cases of the GPU file (test_rowwise_cpu.py runs the model over the same lists)
LN_WIDTHS = (8, 24, 96, 160, 192, 320, 384, 640, 768, 1000, 1280, 1536, 3072, 3080, 4096)
LN_ROWS = (1, 33, 67)
LN_Q8 = ((160, 256), (992, 1024))                      # (c, kp) at rows = 256
EMBED_WIDTHS = (256, 768, 1024, 40, 520, 1280)         # register path | generic path
EMBED_BL = ((1, 1), (3, 5), (2, 33))                   # (b, l): b*l = 1, 15, 66
MERGE_WIDTHS = (96, 192, 8, 104, 384, 512, 520, 1024)  # c (the row is 4c wide)
MERGE_BH = ((1, 2), (1, 6), (3, 6))
HEAD_WIDTHS, HEAD_T, HEAD_B = (64, 192, 768, 1024), (1, 15, 16, 17, 49), (1, 3)
MEAN_WIDTHS, MEAN_L = (1, 255, 257, 768), (1, 128)
LNROWS_BF16 = (65, 100, 192, 256, 384, 512, 768, 1000, 1024)
LNROWS_F32 = ((256, 0), (1024, 0), (128, 0), (384, 0), (8, 0), (100, 0), (200, 0), (520, 1))  # (c, row stride - c)
LNROWS_ROWS = (1, 9, 13)


def eps_list(fam):
    return (1e-5, 1e-12) if fam == "tinyvar" else (1e-5,)


def bf16_rn(t):
    return t.float().to(torch.bfloat16)


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def family(name, rows, c, seed, dtype=torch.bfloat16, offset=40.0):
    """(rows, c) of `dtype` (bf16-rounded where the kernel takes bf16); offset: bigmean's mean."""
    n = torch.randn(rows, c, generator=_gen(1, FAMILIES.index(name), c, seed))
    if name == "gauss":
        x = 3 * n + 1
    elif name == "bigmean":
        x = 0.5 * n + offset
    elif name == "tinyvar":
        x = 0.01 * n
    elif name == "outlier":
        x = 0.02 * n
        i = torch.arange(rows)
        x[i, c - 1 - i % min(8, c)] = 30.0
    elif name == "constant":
        x = torch.full((rows, c), 3.0)
    else:
        raise ValueError(name)
    return x.to(dtype)


def bigmean_offset(c, exact_sums, f32_out=False):
    """bigmean's mean.  40 where the row sums are exact in f32 (bf16 inputs near 40 are multiples of 2^-2, with or
    without a bf16 residual) and for f32 outputs (no bit-equality rule).  Where they round (alpha = 0.7, f32
    embedding tables) the model's 4096 serial adds at kappa ~ 100 flip 6 % of the bf16 roundings, so kappa is
    lowered with the width, kappa sqrt(c) held constant: 160 / sqrt(c)."""
    return 40.0 if exact_sums or f32_out else min(40.0, 160.0 / c ** 0.5)


def params(c, seed, groups=1):
    """gamma (groups, c) = 1 + 0.5 N, beta = 0.3 N (f32); (c,) when groups == 1."""
    g_ = _gen(2, c, seed, groups)
    ga, be = 1 + 0.5 * torch.randn(groups, c, generator=g_), 0.3 * torch.randn(groups, c, generator=g_)
    return (ga[0], be[0]) if groups == 1 else (ga, be)


def ln_f64(v, g, b, eps):
    """v (rows, c) f64, g / b broadcastable to it -> ref, xhat (rows, c), kappa, sigma (rows, 1), all f64."""
    v, g, b = v.double(), g.double(), b.double()
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    sigma = torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xhat = d / sigma
    return xhat * g + b, xhat, v.abs().max(-1, keepdim=True).values / sigma, sigma


def f32_term(xhat, kappa, g, b):
    g, b = g.double().abs(), b.double().abs()
    return U24 * (g * (64 * kappa + 16 * xhat.abs()) + 2 * (g * xhat.abs() + b))


def tol_bf16(ref, xhat, kappa, g, b):
    return 2.0 ** -8 * ref.abs() + f32_term(xhat, kappa, g, b)


def tol_f32(ref, xhat, kappa, g, b):
    return 2.0 ** -23 * ref.abs() + f32_term(xhat, kappa, g, b)


def measure(got, ref, tol):
    """worst |got - ref| / tol (nan if got has a NaN; an exact element counts 0 even at tol 0)."""
    err = (got.detach().double().cpu() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp(min=1e-300))
    return float("nan") if bool(torch.isnan(ratio).any()) else ratio.max().item()


def bit_share(got, ref):
    """share of the elements of bf16 `got` equal to bf16_rn(ref) bit for bit."""
    return (bits(got.detach().cpu()) == bits(bf16_rn(ref))).double().mean().item()


def operand(x, alpha=None, r=None):
    """The f32 row the kernels normalise: fl32(fl32(alpha * x) + r); alpha a float, a (rows, 1) f32 or None."""
    v = x.float()
    if alpha is not None:
        v = v * (alpha if torch.is_tensor(alpha) else torch.tensor(alpha, dtype=torch.float32))
    if r is not None:
        v = v + r.float()
    return v


def operand_f64(x, alpha=None, r=None):
    """Its f64 form: the product rounded to f32, the sum exact."""
    v = operand(x, alpha).double()
    return v + r.double() if r is not None else v


# ---------------------------------------------------------------------------------------------- cases
def ln_case(fam, rows, c, seed, eps=1e-5, alpha=None, res=False, dtype=torch.bfloat16, groups=1, group_div=1,
            post=False):
    """One LayerNorm case on the CPU: inputs, the kernel's f32 operand `v32`, the f64 reference and both bounds.
    groups > 1: row i uses parameter set (i // group_div) % groups of g / b (groups, c), alpha and post_scale
    (groups,) (alpha then means `with alpha`)."""
    off = bigmean_offset(c, exact_sums=alpha is None and dtype == torch.bfloat16, f32_out=dtype == torch.float32)
    x = family(fam, rows, c, seed, dtype, off)
    r = family(fam, rows, c, seed + 1000, dtype, off) if res else None
    g, b = params(c, seed, groups)
    gi = (torch.arange(rows) // group_div) % groups
    g_ = _gen(3, c, seed, groups)
    a = ps = pt = None
    if alpha is not None:
        a = torch.full((groups,), float(alpha)) + (0.1 * torch.arange(groups) if groups > 1 else 0)
    if post:
        ps = 1.3 - 0.4 * torch.arange(groups).float()
        pt = torch.randn(rows, c, generator=g_)
    gr, br = (g[gi], b[gi]) if groups > 1 else (g, b)
    ar = a[gi][:, None] if a is not None else None
    ref, xhat, kappa, sigma = ln_f64(operand_f64(x, ar, r), gr, br, eps)
    extra32, post_term = None, 0.0
    if post:
        extra32 = ps[gi][:, None] * pt                                     # f32 product, as the kernel forms it
        ref = ref + extra32.double()
        post_term = 2 * U24 * extra32.double().abs()                       # the product and the add before it
    base = f32_term(xhat, kappa, gr, br) + post_term
    tb, tf = 2.0 ** -8 * ref.abs() + base, 2.0 ** -23 * ref.abs() + base
    return {"fam": fam, "c": c, "rows": rows, "eps": eps, "x": x, "r": r, "g": g, "b": b, "alpha": a, "post": pt,
            "post_scale": ps, "groups": groups, "group_div": group_div, "v32": operand(x, ar, r), "g_rows": gr,
            "b_rows": br, "extra32": extra32, "ref": ref, "xhat": xhat, "kappa": kappa, "sigma": sigma,
            "tol_bf16": tb, "tol_f32": tf, "exact_beta": fam == "constant" and alpha is None and not post}


def embed_case(fam, b, l, c, seed, eps=1e-12, vocab=37):
    """bert_embed: ids (b, l) holding 0, vocab - 1 and repeats; word rows of the family, pos / type rows small
    Gaussians (f32 tables); v32 = (word + pos) + type in f32, the kernel's order."""
    g_ = _gen(4, c, seed, b, l)
    ids = torch.randint(0, vocab, (b, l), generator=g_)
    flat = ids.view(-1)
    flat[0] = vocab - 1
    if flat.numel() > 1:
        flat[-1] = 0
    if flat.numel() > 3:
        flat[1] = flat[2] = 5
    word = family(fam, vocab, c, seed, torch.float32, bigmean_offset(c, exact_sums=False))
    if fam == "constant":
        pos, typ = torch.zeros(max(l, 2), c), torch.zeros(c)      # keeps the row constant: output = beta exactly
    else:
        pos, typ = 0.05 * torch.randn(max(l, 2), c, generator=g_), 0.05 * torch.randn(c, generator=g_)
        if fam == "tinyvar":
            pos, typ = 0.1 * pos, 0.1 * typ
    g, be = params(c, seed)
    p = torch.arange(b * l) % l
    v32 = (word[flat] + pos[p]) + typ
    ref, xhat, kappa, sigma = ln_f64(v32, g, be, eps)
    return {"fam": fam, "c": c, "rows": b * l, "eps": eps, "ids": ids, "word": word, "pos": pos, "type0": typ,
            "g": g, "b": be, "v32": v32, "g_rows": g, "b_rows": be, "extra32": None, "ref": ref, "xhat": xhat,
            "kappa": kappa, "tol_bf16": tol_bf16(ref, xhat, kappa, g, be), "exact_beta": fam == "constant"}


MERGE_QUADS = ("gauss", "tinyvar", "outlier", "bigmean")  # families of x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2]


def merge_case(B, H, c, seed, eps=1e-5, quads=MERGE_QUADS):
    """patch_merge_ln: x (B, H, H, c) bf16 whose four source pixels of a merged row carry different families
    (a swapped quadrant order moves every output), merged in timm's quadrant order."""
    x = torch.empty(B, H, H, c, dtype=torch.bfloat16)
    n = B * (H // 2) ** 2
    for q, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        x[:, dy::2, dx::2] = family(quads[q], n, c, seed + q).view(B, H // 2, H // 2, c)
    v = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(n, 4 * c)
    g, b = params(4 * c, seed)
    ref, xhat, kappa, sigma = ln_f64(v, g, b, eps)
    return {"fam": "mixed", "c": 4 * c, "rows": n, "eps": eps, "x": x, "g": g, "b": b, "v32": v.float(), "g_rows": g,
            "b_rows": b, "extra32": None, "ref": ref, "xhat": xhat, "kappa": kappa,
            "tol_bf16": tol_bf16(ref, xhat, kappa, g, b), "exact_beta": False}


def head_case(fam, b, t, c, seed, eps=1e-5):
    """swin_head: x (b, t, c) bf16 -> patches = LN(LN(x)) (b, t, c), global = mean_t LN(x), pool = (global +
    sum_t patches) / (t + 1), with their bounds (module docstring)."""
    x = family(fam, b * t, c, seed)
    g, be = params(c, seed)
    u, xh1, k1, s1 = ln_f64(x, g, be, eps)
    e1 = tol_f32(u, xh1, k1, g, be)
    p, xh2, k2, s2 = ln_f64(u, g, be, eps)
    tp = e1 * g.double().abs() / s2 + tol_f32(p, xh2, k2, g, be)
    u3, e3, p3, tp3 = (z.view(b, t, c) for z in (u, e1, p, tp))
    glob = u3.mean(1)
    tg = e3.mean(1) + t * U24 * u3.abs().mean(1)
    pool = (glob + p3.sum(1)) / (t + 1)
    tpool = (tg + tp3.sum(1)) / (t + 1) + (t + 1) * U24 * (glob.abs() + p3.abs().sum(1)) / (t + 1)
    return {"fam": fam, "c": c, "b": b, "t": t, "eps": eps, "x": x.view(b, t, c), "g": g, "b_": be, "patches": p3,
            "tol_patches": tp3, "glob": glob, "tol_glob": tg, "pool": pool, "tol_pool": tpool}


def mean_case(b, l, c, seed):
    x = family("gauss", b * l, c, seed).view(b, l, c)
    return {"x": x, "ref": x.double().mean(1), "tol": l * U24 * x.double().abs().mean(1)}


LN_VARIANTS = ((None, False), (None, True), (0.7, False), (0.7, True))                  # (alpha, residual)
# (groups, group_div, alpha, residual, post)
LNROWS_VARIANTS = ((1, 1, None, False, False), (3, 1, 0.7, True, True), (3, 2, 0.7, False, True), (3, 2, None, True, False))


def layernorm_cases(c, rows=max(LN_ROWS)):
    """Every (family, eps, alpha, residual) of the layernorm_launch tests at width c (constant: no alpha)."""
    for fam in FAMILIES:
        for eps in eps_list(fam):
            for alpha, res in LN_VARIANTS:
                if not (fam == "constant" and alpha is not None):
                    yield ln_case(fam, rows, c, c, eps, alpha, res)


def lnrows_cases(c, dtype, rows=max(LNROWS_ROWS)):
    for fam in FAMILIES:
        for eps in eps_list(fam):
            for groups, gdiv, alpha, res, post in LNROWS_VARIANTS:
                if not (fam == "constant" and alpha is not None):
                    yield ln_case(fam, rows, c, c + 1, eps, alpha, res, dtype, groups, gdiv, post)


def embed_cases(c, b, l):
    for fam in FAMILIES:
        for eps in ((1e-12, 1e-5) if fam == "tinyvar" else (1e-12,)):
            yield embed_case(fam, b, l, c, c + l, eps)


# ---------------------------------------------------------------------------------------------- f32 model
def _seq_sum(v):
    """Row sums of f32 (rows, c), one add per column in index order."""
    vt = v.t().contiguous()
    s = torch.zeros(v.shape[0], dtype=torch.float32)
    for j in range(vt.shape[0]):
        s = s + vt[j]
    return s


def model_f32(v32, g, b, eps, mutant=None, out="bf16", extra32=None):
    """Plain two-pass f32 LayerNorm of the f32 operand rows, every sum sequential; `mutant` one of MUTANTS."""
    assert v32.dtype == torch.float32 and mutant in (None,) + MUTANTS
    c = v32.shape[1]
    g, b = g.float().expand(v32.shape), b.float().expand(v32.shape)
    if mutant == "gshift":
        idx = (torch.arange(c) + 8).clamp(max=c - 1)
        g, b = g[:, idx], b[:, idx]
    mean = (_seq_sum(v32) / (c + 8 if mutant == "cpad" else c))[:, None]
    d = v32 - mean
    if mutant == "onepass":
        var = (_seq_sum(v32 * v32) / c - mean[:, 0] * mean[:, 0]).clamp(min=0)
    else:
        var = _seq_sum(d * d) / (c - 1 if mutant == "cm1" else c)
    e = torch.tensor(0.0 if mutant == "noeps" else eps, dtype=torch.float32)
    rstd = (1.0 / torch.sqrt(var + e))[:, None]
    y = d * rstd * g + b
    if extra32 is not None:
        y = y + extra32
    if out == "f32":
        return y
    if mutant == "trunc":
        return (y.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return y.to(torch.bfloat16)


def model_head(x, g, b, eps):
    """The f32 model of swin_head: (patches (b, t, c), global, pool), sequential token sums."""
    bsz, t, c = x.shape
    u = model_f32(x.reshape(bsz * t, c).float(), g, b, eps, out="f32")
    p = model_f32(u, g, b, eps, out="f32")
    u, p = u.view(bsz, t, c), p.view(bsz, t, c)
    s1, s2 = torch.zeros(bsz, c), torch.zeros(bsz, c)
    for k in range(t):
        s1, s2 = s1 + u[:, k], s2 + p[:, k]
    glob = s1 / t
    return p, glob, (glob + s2) / (t + 1)
