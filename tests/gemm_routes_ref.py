"""Exact references, data, per-route kernel models and their mutants for the bf16 tiled GEMM mmr_linear_bf16
(csrc/gemm.hip: gemm_bf16_tn, gemm_bf16_tn_w4, gemm_bf16_tn_big, gemm_bf16_tn_p8), shared by test_gemm_routes_cpu.py
and test_gemm_routes_gpu.py.  bits and gelu_f64 are rowwise_ref's and small_linear_ref's.

Routes.  mmr_linear_bf16 has 11 launch variants and 11 kernels (ROUTES, the MMR_GEMM_ROUTE_* of mmr.h); a variant
names a wish and the shape guards decide, so a case states the variant it pins and the route it must reach, without
(route) and with a residual (route_res): mmr_linear_bf16_route answers for both, with and without a GPU.  CASES holds,
for 256 CUs, the smallest shape that reaches each route and the route's edges (M, N, K tails where the route admits
them, the fall-through rows of the w4 variants, whose kernels take no residual).

Residual rounding (RES_MODEL, read from the epilogues):
  round2  rne(rne(act(acc + b)) + r): the base kernel and big_epilogue stage act(acc + b) in LDS as bf16, then add
          the bf16 residual in f32 and round again.  The w4 kernels would add in f32, but the launcher gives them no
          residual; their entry is never used.
  round1  rne(act(acc + b) + r): the 8-phase kernel adds the residual to the f32 value and rounds once (both its
          permlane GELU epilogue and its LDS-staged epilogue).
GELU form (GELU_FORM): gelu_fast in the base, w4 and big kernels, gelu_fast2 (packed f32, -log2 e folded into the
coefficients) in the 8-phase kernel.

Data is a hash of the element's indices, so any row or column range of a case is generated alone and on any device.
  exact   act = 0.  x, w integers in [-4, 4] (x times 8 where K < 64, so that outputs still leave the exact bf16
          range and the two rounding models differ), bias multiples of 1/4 in [-8, 8], residual integers in
          [-64, 64].  Every product and partial sum is an integer below 2^22 and the bias a multiple of 1/4, so
          the f32 accumulation and both epilogue adds are exact in any order: the output is expected BIT FOR BIT,
          rne_bits of the exact value under the route's rounding model.  Most outputs need rounding (|acc| ~ 100
          with quarter bits), ties included.
  gelu    act = 1.  x, w in {-1, 0, 1} with density min(1, sqrt(10 / K)), bias multiples of 1/8 in [-4, 4],
          residual multiples of 1/8 in [-8, 8]: z = acc + b is exact, a multiple of 1/8 with std ~ 3.3, so it
          passes the transition region, exact 0 and the saturated range beyond +-7; |z| <= ZMAX is asserted.
          |got - (gelu_f64(z) + r)| <= tol per element, tol built from
            FIT     1.2e-5, the fit error common.h states for gelu_fast (re-measured in f64 over [-40, 40]:
                    1.1951e-5 at |z| = 3.880, gelu_fast2's folded constants the same to 5 digits);
            SLACK   the f32 evaluation: twice the largest |f32 restatement - f64 evaluation of the same formula|
                    of gelu_fast / gelu_fast2 over every multiple of 1/8 in [-40, 40] (every z a case can take).
                    Measured 4.016e-7 (at z = 4.25, the same for both forms; beyond |z| ~ 5.3 the sigmoid is
                    1 or 0 in f32 and the result exact); twice that, the margin for the v_exp_f32 / v_rcp_f32
                    ulps the restatement does not have: SLACK = 8.1e-7;
            one bf16 half-ulp per rounding of the route's model, each taken at the largest magnitude the rounded
            value can have (|value| + the error so far), and 2^-24 |ref| for the f32 add of the residual.

model(route, x, w, b, r, act, mutant) restates a kernel: exact accumulation over the route's tiles, the route's
epilogue in f32 (numpy restatement of gelu_fast / gelu_fast2), its rounding model, written into the middle rows of a
sentinel-filled (M + 2 GUARD, N) buffer, which is what verify_exact / verify_gelu take from model and GPU alike.
Mutants (test_gemm_routes_cpu.py: wherever a mutant changes the model's output at all, the checks fail; each is
caught on every route it applies to, MUTANT_ROUTES):
  kchunk    one 8-wide K chunk of the last tile dropped          ktail     k beyond the last full KB slice ignored
  tileswap  the first and last output tiles exchanged            skiptile  the last tile never written
  trunc     truncating bf16 store                                biascol   bias read one tile width further on
  actlate   GELU after the residual (gelu family)                round     the other residual model (exact family)
  tanh      tanh-form GELU (gelu family)                         overrun   rows >= M of the last row tile written"""
import collections

import numpy as np
import torch

from rowwise_ref import U24, bits  # noqa: F401  (re-exported)
from small_linear_ref import gelu_f64

ROUTES = ("base_128x128", "w4_256x256", "w4_256x192", "big_256x256_kb64x2", "big_256x256_kb32x4",
          "big_256x192_kb64x2", "big_256x128_kb32x2", "big_256x128_kb32x3", "big_256x128_kb64x3", "p8_256x256",
          "p8_256x192")
RID = {n: i for i, n in enumerate(ROUTES)}
# route -> (tile rows, tile columns, K slice depth)
TILE = {"base_128x128": (128, 128, 64), "w4_256x256": (256, 256, 64), "w4_256x192": (256, 192, 64),
        "big_256x256_kb64x2": (256, 256, 64), "big_256x256_kb32x4": (256, 256, 32),
        "big_256x192_kb64x2": (256, 192, 64), "big_256x128_kb32x2": (256, 128, 32),
        "big_256x128_kb32x3": (256, 128, 32), "big_256x128_kb64x3": (256, 128, 64),
        "p8_256x256": (256, 256, 64), "p8_256x192": (256, 192, 64)}
RES_MODEL = {r: ("round1" if r.startswith(("p8", "w4")) else "round2") for r in ROUTES}
GELU_FORM = {r: ("fast2" if r.startswith("p8") else "fast") for r in ROUTES}
N_VARIANTS, CUS = 11, 256
GUARD = 4                       # guard rows on each side of the output
SENT = 0x7FD3                   # bf16 quiet NaN with a payload: no result equals it
FIT, SLACK, ZMAX = 1.2e-5, 8.1e-7, 40.0

Case = collections.namedtuple("Case", "route variant m n k route_res note")


def _c(route, variant, m, n, k, route_res=None, note=""):
    return Case(route, variant, m, n, k, route_res or route, note)


CASES = (
    # base 128x128: variant 8, and any variant below M = 4096
    _c("base_128x128", 8, 257, 136, 72, note="M, N and K tails at once"),
    _c("base_128x128", 8, 1, 136, 72, note="M = 1"),
    _c("base_128x128", 8, 257, 8, 72, note="N = 8"),
    _c("base_128x128", 8, 257, 136, 8, note="K = 8"),
    _c("base_128x128", 0, 257, 136, 72, note="variant 0 below M = 4096"),
    _c("base_128x128", 9, 257, 256, 128, note="variant 9, M % 256 != 0, below M = 4096"),
    # w4 256x256: variant 0; with a residual it falls through to the 8-wave kernels
    _c("w4_256x256", 0, 4096, 4096, 256, "big_256x128_kb64x3", "256 tiles, one per workgroup"),
    _c("w4_256x256", 0, 8000, 2048, 320, "big_256x128_kb64x3", "shifted last row tile, 5 slices"),
    _c("w4_256x256", 0, 8192, 4096, 256, "big_256x256_kb64x2", "2 tiles per workgroup; 0 with a residual"),
    # w4 256x192: variant 1, or 0 when N % 256 != 0
    _c("w4_256x192", 1, 4096, 192, 256, "base_128x128", "16 tiles"),
    _c("w4_256x192", 0, 4096, 192, 256, "base_128x128", "variant 0, N % 256 != 0"),
    _c("w4_256x192", 1, 4099, 576, 320, "base_128x128", "51 tiles, uneven XCD shares, shifted last row tile"),
    # big 256x256, KB64 x2 (variant 2) / KB32 x4 (variant 3)
    _c("big_256x256_kb64x2", 2, 8192, 4096, 256),
    _c("big_256x256_kb64x2", 2, 8192, 4096, 264, note="K = 264"),
    _c("big_256x256_kb64x2", 2, 8000, 4096, 256, note="M = 8000"),
    _c("big_256x256_kb64x2", 1, 8192, 4096, 256, note="variant 1, N % 192 != 0"),
    _c("big_256x256_kb32x4", 3, 8192, 4096, 256),
    _c("big_256x256_kb32x4", 3, 8192, 4096, 264, note="K = 264"),
    _c("big_256x256_kb32x4", 3, 8000, 4096, 256, note="M = 8000"),
    # big 256x128 KB64 x3: variant 4, and the fall-through of the others
    _c("big_256x128_kb64x3", 4, 8192, 2048, 256),
    _c("big_256x128_kb64x3", 4, 8192, 2048, 264, note="K = 264"),
    _c("big_256x128_kb64x3", 9, 8000, 2048, 256, note="fall-through from variant 9 (M % 256 != 0)"),
    # big 256x128 KB32 x2 / x3: variants 5 / 6
    _c("big_256x128_kb32x2", 5, 4096, 128, 256),
    _c("big_256x128_kb32x2", 5, 4100, 128, 264, note="M and K tails"),
    _c("big_256x128_kb32x2", 5, 4096, 256, 256, note="two tile columns"),
    _c("big_256x128_kb32x3", 6, 4096, 128, 256),
    _c("big_256x128_kb32x3", 6, 4100, 128, 264, note="M and K tails"),
    _c("big_256x128_kb32x3", 6, 4096, 256, 256, note="two tile columns"),
    # big 256x192 KB64 x2: variant 7
    _c("big_256x192_kb64x2", 7, 4096, 3072, 256),
    _c("big_256x192_kb64x2", 7, 4100, 3072, 264, note="M and K tails"),
    # 8-phase 256x256 / 256x192: variants 9 / 10
    _c("p8_256x256", 9, 256, 256, 128, note="1 tile, 7 idle workgroups"),
    _c("p8_256x256", 9, 768, 768, 384, note="9 tiles, uneven XCD shares"),
    _c("p8_256x256", 9, 4096, 4352, 128, note="272 tiles, 1-2 per workgroup, one K iteration per tile"),
    _c("p8_256x192", 10, 256, 192, 128, note="1 tile"),
    _c("p8_256x192", 10, 768, 576, 384, note="9 tiles"),
    _c("p8_256x192", 10, 4096, 4416, 128, note="368 tiles, 1-2 per workgroup"),
)
# (name, act, bias, residual, in place)
EPILOGUES = (("none", 0, False, False, False), ("bias", 0, True, False, False), ("bias_gelu", 1, True, False, False),
             ("bias_res", 0, True, True, False), ("bias_gelu_res", 1, True, True, False),
             ("bias_res_inplace", 0, True, True, True))
TUNER_SHAPE = (4096, 768, 256)          # a shape no other test of the suite gives mmr_linear_bf16

MUTANTS = ("kchunk", "ktail", "tileswap", "skiptile", "trunc", "biascol", "actlate", "round", "tanh", "overrun")
# the routes on which the case table gives each mutant something to change: K tails and rows past M exist on the
# base and big routes only, a residual on every route but the w4 pair
_TAILS = tuple(r for r in ROUTES if r.startswith(("base", "big")))
_RES = tuple(r for r in ROUTES if not r.startswith("w4"))
MUTANT_ROUTES = {"kchunk": ROUTES, "ktail": _TAILS, "tileswap": ROUTES, "skiptile": ROUTES, "trunc": ROUTES,
                 "biascol": ROUTES, "actlate": _RES, "round": _RES, "tanh": ROUTES, "overrun": _TAILS}


def case_id(c):
    return f"{c.route}-v{c.variant}-{c.m}x{c.n}x{c.k}"


def family_of(act):
    return "gelu" if act else "exact"


def route_of(c, res):
    return c.route_res if res else c.route


# ---------------------------------------------------------------------------------------------- data
def _hash(i, j, salt):
    """32 well-mixed bits of (i, j, salt); i, j int64 tensors (broadcast), every intermediate below 2^63."""
    h = (i * 0x9E3779B1 + j * 0x85EBCA77 + salt * 0x27D4EB2F) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h = h ^ (h >> 12)
    h = (h * 0x297A2D39) & 0xFFFFFFFF
    return h ^ (h >> 15)


def density(k):
    return min(1.0, (10.0 / k) ** 0.5)


def x_scale(k):
    return 8.0 if k < 64 else 1.0


def data(fam, m, n, k, rows=None, cols=None, device="cpu", parts="xwbr"):
    """The operands of a case's family as f32 tensors holding bf16-exact values (bias: f32): x (rows, k), w (cols,
    k), b (cols,), r (rows, cols); rows / cols: the first so many of the case's (default all).  parts: which to
    make."""
    rows, cols = m if rows is None else rows, n if cols is None else cols
    salt = (m * 31 + n * 17 + k * 7 + (5 if fam == "gelu" else 0)) % 1000003
    ar = (lambda cnt: torch.arange(cnt, dtype=torch.int64, device=device))
    i, j, kk = ar(rows)[:, None], ar(cols)[:, None], ar(k)[None, :]
    out = {}
    if fam == "exact":
        if "x" in parts:
            out["x"] = (_hash(i, kk, salt + 1) % 9 - 4).float() * x_scale(k)
        if "w" in parts:
            out["w"] = (_hash(j, kk, salt + 2) % 9 - 4).float()
        if "b" in parts:
            out["b"] = (_hash(ar(cols), 0, salt + 3) % 65 - 32).float() / 4
        if "r" in parts:
            out["r"] = (_hash(i, ar(cols)[None, :], salt + 4) % 129 - 64).float()
    else:
        thr = int(density(k) * 4096)

        def tern(h):
            return torch.where((h & 4095) < thr, 1 - 2 * ((h >> 12) & 1), torch.zeros_like(h)).float()
        if "x" in parts:
            out["x"] = tern(_hash(i, kk, salt + 1))
        if "w" in parts:
            out["w"] = tern(_hash(j, kk, salt + 2))
        if "b" in parts:
            out["b"] = (_hash(ar(cols), 0, salt + 3) % 65 - 32).float() / 8
        if "r" in parts:
            out["r"] = (_hash(i, ar(cols)[None, :], salt + 4) % 129 - 64).float() / 8
    return out


def preact(x, w):
    """The exact accumulator x w^T in f64 on the CPU (integers: exact); shared by a shape's epilogues."""
    return x.double().cpu() @ w.double().cpu().t()


def abs_term_bound(k):
    """An upper bound of sum |terms| of an exact-family output in units of 1/4: below 2^24, so every f32 sum is
    exact."""
    return 4 * (k * 16 * x_scale(k) + 8 + 64)


# ---------------------------------------------------------------------------------------------- bf16
def rne_bits(v):
    """f32 tensor (finite) -> bf16 bits (int16), round to nearest even, in integer arithmetic."""
    b = v.float().contiguous().view(torch.int32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).to(torch.int16)


def trunc_bits(v):
    return (v.float().contiguous().view(torch.int32) >> 16).to(torch.int16)


def bf2f(b16):
    """bf16 bits (int16) -> f32."""
    return (b16.to(torch.int32) << 16).view(torch.float32)


def to_bf16(v):
    """f32 tensor of bf16-exact values -> torch.bfloat16 (asserted exact)."""
    t = v.to(torch.bfloat16)
    assert torch.equal(t.float(), v.float()), "operand not exact in bf16"
    return t


def half_ulp(a):
    """Half a bf16 ulp (8 significand bits) at magnitude a >= 0 (f64): 2^(floor(log2 a) - 8), from the exponent
    field (exact, no logarithm)."""
    e = (a.double().clamp(min=2.0 ** -126).contiguous().view(torch.int64) >> 52) & 0x7FF       # biased exponent
    return ((e - 8) << 52).view(torch.float64)


# ---------------------------------------------------------------------------------------------- expectations
def expected_exact(acc, b, r, res_model):
    """Exact family: the bf16 bits of (acc + b (+ r)) under a rounding model; acc f64 integers, b / r f32 or None.
    Every f32 operation below is exact (abs_term_bound)."""
    v = acc.float()
    if b is not None:
        v = v + b
    if r is None:
        return rne_bits(v)
    if res_model == "round2":
        return rne_bits(bf2f(rne_bits(v)) + r)
    return rne_bits(v + r)


def gelu_ref_tol(z, r, res_model):
    """gelu family: (ref, tol) f64 for z = acc + b exact (f64) and the residual r (or None)."""
    g = gelu_f64(z.double())
    e1 = FIT + SLACK
    if r is None:
        return g, e1 + half_ulp(g.abs() + e1)
    ref = g + r.double()
    if res_model == "round2":
        e1 = e1 + half_ulp(g.abs() + e1)                 # the staged bf16 value
    e2 = e1 + U24 * (ref.abs() + e1)                     # the f32 add of the residual
    return ref, e2 + half_ulp(ref.abs() + e2)


def verify_exact(buf, m, exp_bits):
    """buf (m + 2 GUARD, n) int16 -> (guard rows untouched, sentinels left inside, elements != expected)."""
    mid = buf[GUARD:GUARD + m]
    return (bool((buf[:GUARD] == SENT).all() and (buf[GUARD + m:] == SENT).all()), int((mid == SENT).sum()),
            int((mid != exp_bits).sum()))


def verify_gelu(buf, m, ref, tol):
    """-> (guard rows untouched, sentinels left inside, worst |got - ref| / tol; nan if a NaN came out)."""
    mid = buf[GUARD:GUARD + m]
    ratio = (bf2f(mid).double() - ref).abs() / tol
    worst = float("nan") if bool(torch.isnan(ratio).any()) else ratio.max().item()
    return (bool((buf[:GUARD] == SENT).all() and (buf[GUARD + m:] == SENT).all()), int((mid == SENT).sum()), worst)


def passes(res):
    ok_guard, n_sent, bad = res
    return ok_guard and n_sent == 0 and (bad == 0 if isinstance(bad, int) else bad <= 1.0)


# ---------------------------------------------------------------------------------------------- GELU forms
_P = (3.275317185739523e-06, -7.756018138382363e-05, -0.00016997469037563395, 0.07280746695679054,
      1.5957042563586181)
_L2E = 1.4426950408889634


def gelu_fast_np(v, form="fast", dtype=np.float32):
    """common.h gelu_fast / gelu_fast2 restated in numpy.  dtype float32: operation for operation (fmaf as one
    rounding of the f64 product-sum, exp2 and the reciprocal correctly rounded where the hardware's are within an
    ulp); float64: the same formula with the same f32 constants evaluated in f64."""
    f32 = np.float32
    v = np.asarray(v, dtype=dtype)
    if dtype == np.float32:
        def fma(a, b, c):
            return (np.float64(a) * np.float64(b) + np.float64(c)).astype(f32)
    else:
        def fma(a, b, c):
            return a * b + c
    one = dtype(1.0)
    with np.errstate(over="ignore", under="ignore"):
        x2 = v * v
        if form == "fast":
            c = [dtype(f32(t)) for t in _P]
            p = fma(c[0], x2, c[1])
            for t in c[2:]:
                p = fma(p, x2, t)
            e = np.exp2((dtype(f32(-_L2E)) * v) * p)
            return v * (one / (one + e))
        c = [dtype(f32(f32(t) * f32(-_L2E))) for t in _P]        # the constants folded in f32 at compile time
        p = fma(np.full_like(v, c[0]), x2, c[1])
        for t in c[2:]:
            p = fma(p, x2, t)
        e = np.exp2(v * p)
        return v * (one / (e + one))


def gelu_tanh_np(v):
    v = np.asarray(v, dtype=np.float32)
    f32 = np.float32
    return f32(0.5) * v * (f32(1) + np.tanh(f32(0.7978845608028654) * (v + f32(0.044715) * v * v * v)))


def z_grid():
    """Every multiple of 1/8 in [-ZMAX, ZMAX]: every pre-activation a gelu case can take."""
    return np.arange(-int(ZMAX * 8), int(ZMAX * 8) + 1, dtype=np.float64) / 8


def measure_fit(form, npoints=2_000_001):
    """(max |formula in f64 - erf GELU|, z of the maximum) over [-ZMAX, ZMAX]: a dense grid and z_grid."""
    z = np.concatenate([np.linspace(-ZMAX, ZMAX, npoints), z_grid()])
    err = np.abs(gelu_fast_np(z, form, np.float64) - gelu_f64(torch.from_numpy(z)).numpy())
    i = int(err.argmax())
    return float(err[i]), float(z[i])


def measure_slack(form):
    """max |f32 restatement - f64 evaluation of the same formula| over z_grid, and its z."""
    z = z_grid()
    err = np.abs(gelu_fast_np(z.astype(np.float32), form, np.float32).astype(np.float64)
                 - gelu_fast_np(z, form, np.float64))
    i = int(err.argmax())
    return float(err[i]), float(z[i])


# ---------------------------------------------------------------------------------------------- kernel model
def tiles_of(route, m, n):
    """[(row start, row end, column start, column end)] of the route's output tiles, row-major.  The w4 kernels
    shift their last row tile up to end at row m (m >= 256); the others clip it."""
    tm, tn, _ = TILE[route]
    w4 = route.startswith("w4")
    out = []
    for i in range(-(-m // tm)):
        r0 = min(i * tm, m - tm) if w4 else i * tm
        for j in range(-(-n // tn)):
            out.append((r0, min(r0 + tm, m), j * tn, min((j + 1) * tn, n)))
    return out


def model(route, x, w, b, r, act, mutant=None, inplace=False):
    """The route's kernel on the CPU: x (m, k), w (n, k), r (m, n) f32 tensors of bf16-exact values (r None: no
    residual), b (n,) f32 or None -> the (m + 2 GUARD, n) int16 buffer the launch leaves (bf16 bits; SENT where
    nothing was written; in place: the middle rows started as r)."""
    m, k = x.shape
    n = w.shape[0]
    tm, tn, kb = TILE[route]
    tiles = tiles_of(route, m, n)
    xd, wd = x.double(), w.double()
    keff = k // kb * kb if mutant == "ktail" else k
    acc = xd[:, :keff] @ wd[:, :keff].t()
    if mutant == "kchunk":
        r0, r1, c0, c1 = tiles[-1]
        q = 8 * min(1, k // 8 - 1)
        acc[r0:r1, c0:c1] -= xd[r0:r1, q:q + 8] @ wd[c0:c1, q:q + 8].t()
    bb = b
    if b is not None and mutant == "biascol":
        bb = b[(torch.arange(n) + tn) % n]
    res_model = RES_MODEL[route]
    if mutant == "round":
        res_model = "round1" if res_model == "round2" else "round2"

    def gelu(v):
        if mutant == "tanh":
            return torch.from_numpy(gelu_tanh_np(v.numpy()))
        return torch.from_numpy(gelu_fast_np(v.numpy(), GELU_FORM[route], np.float32))

    def epilogue(a, rr):
        v = a.float()
        if bb is not None:
            v = v + bb
        if act and mutant != "actlate":
            v = gelu(v)
        if rr is not None:
            v = (bf2f(rne_bits(v)) if res_model == "round2" else v) + rr
        if act and mutant == "actlate":
            v = gelu(v)
        return trunc_bits(v) if mutant == "trunc" else rne_bits(v)

    out = epilogue(acc, r)
    start = rne_bits(r) if inplace else torch.full((m, n), SENT, dtype=torch.int16)
    if mutant == "tileswap" and len(tiles) > 1:
        (a0, a1, b0, b1), (c0, c1, d0, d1) = tiles[0], tiles[-1]
        h, wd_ = min(a1 - a0, c1 - c0), min(b1 - b0, d1 - d0)
        t = out[a0:a0 + h, b0:b0 + wd_].clone()
        out[a0:a0 + h, b0:b0 + wd_] = out[c0:c0 + h, d0:d0 + wd_]
        out[c0:c0 + h, d0:d0 + wd_] = t
    if mutant == "skiptile":
        r0, r1, c0, c1 = tiles[-1]
        out[r0:r1, c0:c1] = start[r0:r1, c0:c1]
    buf = torch.full((m + 2 * GUARD, n), SENT, dtype=torch.int16)
    buf[GUARD:GUARD + m] = out
    if mutant == "overrun" and m % tm != 0 and not route.startswith("w4"):
        extra = min(GUARD, tm - m % tm)                 # rows of the last row tile past m: x rows of zeros
        buf[GUARD + m:GUARD + m + extra] = epilogue(torch.zeros(extra, n, dtype=torch.float64), None)
    return buf


def cut(c, res):
    """(rows, cols) of a case as the CPU tests run it: the first 256 rows plus the row tail (m % 256, so a last,
    clipped or shifted, row tile stays) and the first two tile columns of the route in use."""
    tn = TILE[route_of(c, res)][1]
    return (c.m if c.m <= 256 else 256 + c.m % 256), min(c.n, 2 * tn)
