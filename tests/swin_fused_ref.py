"""Plain-torch f64 references, input families, the two rules, the rounding-point model, its mutants and the
locality predicate for the fused Swin stage 1-2 kernels (csrc/swin_mlp.hip swin_mlp_sp / swin_mlp,
csrc/swin_attn.hip swin_attn_block, csrc/gemm_rw.hip gemm_rw, csrc/x3_sab.hip x3_swin_attn_block), shared by
test_swin_fused_cpu.py and test_swin_fused_gpu.py.

Reference R.  The chain in f64 on exactly the operands the kernel is given (bf16 tokens and weights widened, f32
biases / gamma / beta / rel-pos table widened), no intermediate rounding:
  MLP          x + fc2(GELU_erf(fc1(LN(x))))                                (mlp_chain)
  attention    x + proj(W-MSA(LN(x))) with roll, window partition, q * 32^-0.5, rel-pos bias, -100 shift mask,
               from oracle.towers' window_partition / shift_mask / relative_position_index   (attn_chain)
  linear_rw    x W^T + b + r                                                (rw_chain)
Model Mdl.  The same chain in f32 torch on the CPU (f32 matmuls, erf GELU) with the kernels' documented rounding
points to bf16: LN out and the GELU'd hidden for the MLP (swin_mlp.hip header); LN out, the scaled q, k, v, the
un-normalised P = exp(s - max) (the row sum is taken of the f32 values, 1 / sum applied to P V in f32) and O for the
attention block (swin_attn.hip header); none for linear_rw.  Mdl is kept in f32, before the output rounding.
sigma = RMS(Mdl - R) over the case: the noise the rounding points alone put on the output.

Rules (constants fixed by the issue, not fitted):
  rule 1, every element:        |y - R| <= 2^-8 |R| + 8 sigma
  rule 2, every output channel, cases of T >= 256 tokens:
                                |mean_t (y - R)[c]| <= 8 (sigma + 2^-9 rms_t R[:, c]) / sqrt(T)
The output rounding of a kernel may by itself use all of 2^-8 |R| (an element just above a power of two), so Mdl is
held to both rules before that rounding, at a worst ratio <= MODEL_MAX = 0.5 on every case the GPU file launches
(test_swin_fused_cpu.py): a kernel with another summation order and gelu_fast (|err| < 1.2e-5, common.h) then has
the output rounding plus half of 8 sigma.

Families of token rows (T, C), bf16.  Every family rides on BASE = 8: LayerNorm does not see a common offset, the
residual does, so R = x + branch stays away from 0 and rule 1's 2^-8 |R| term stands beside 8 sigma everywhere.
Without it the model cannot meet 0.5: its error is close to Gaussian, the worst of 10^5 elements lies 4.4 ... 5
sigma out (rows with a large LN output 7 ... 9 sigma out in the attention block), and where R passes through 0
nothing but 8 sigma stands against it (measured 0.50 ... 1.1 on zero-mean inputs).  The inputs were changed, not
the rules; the price is a rule 2 bound led by 2^-9 rms R = 0.016 instead of sigma = 0.002.
  gauss     1.5 N + 8
  offset    N + 20: mean 20 std, what bf16 keeps there is 2^-3, 3 bits of the spread
  spike     N + 8 with channel (7 i) mod C of row i raised or lowered by 6 ... 8: LN puts 4 ... 6 (times gamma)
            there.  A spike of 20 on 0.05 N (LN: sqrt(C - 1) = 9.7) was lowered: the rounding of that one LN
            output (ulp 2^-4) is shared by every q, k, v of the token and put single rows 9 ... 12 sigma out (model
            at 0.65 ... 1.1), and identical spikes round identically on every row that has them (rule 2 at 1.3 ...
            3.0).  With fc1 weights of 2 C^-0.5 N and b1 ~ N the pre-activations still pass +-7, the interval
            gelu_fast was fitted on (test_swin_fused_cpu.py counts them).
  constant  row i holds one bf16 value of [4, 12], all distinct (row sums exact in f32; LN gives beta)
  mixed     rows cycling through the four
Rule 2 takes the errors of the T tokens as independent.  Constant rows are not: LN gives every one of them beta, so
their branch fc2(GELU(fc1(beta))) and its error are one vector, and no rule that tightens as sqrt(T) can hold T
copies of it.  Again the input is changed, not the rule: where T >= 256 the `constant` family keeps
floor(sqrt(T) / 2) constant rows in front (15 of 1000) and fills up with gauss rows, and `mixed` caps its constant
rows at the same number.  Below 256 tokens (rule 1 only) every row of `constant` is constant.
Parameters: gamma = 1 + 0.3 N; beta, b1, b2, qkv_b, proj_b ~ N(0, 1) (a wrong bias entry is O(1), far above the
noise); rel-pos table ~ N(0, 1); fc1 2 C^-0.5 N, qkv C^-0.5 N, fc2 and proj 0.5 fan_in^-0.5 N (the branch at about
the residual's size); all weights rounded to bf16.

Mutants of Mdl (rounded to bf16 as a kernel would store it).  CAUGHT_BY names the kernel, rule and family each is
caught by at every size the GPU file launches.  Structural mutants (they move which tokens interact) are held to
the locality predicate of part B instead: allowed_region() from oracle.towers' partition and mask, not from the
kernels' index math.  BELOW_NOISE lists the three mutants whose effect is at or below the rounding noise the rules
must admit, with the reason; test_swin_fused_cpu.py measures them."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import towers as otw

U8 = 2.0 ** -8
MODEL_MAX = 0.5
BASE = 8.0      # every family rides on it (module docstring)
FAMILIES = ("gauss", "offset", "spike", "constant", "mixed")
WS, HEADS, DH, AC = 7, 3, 32, 96

# ---- the cases of part C (the GPU file launches them, the CPU file runs the model over the same lists)
MLP_T = (1, 31, 33, 257, 1000)
MLP_C = (96, 192)
ATTN_GEO = ((3, 14), (2, 21), (1, 56))      # (B, hw), each with shift 0 and 3
ATTN_SHIFTS = (0, 3)
# (N, K, bias, residual) of test_towers_gpu.py::test_linear_rw, M <= 1000
RW_CASES = ((96, 64, True, False), (576, 192, True, False), (192, 192, True, True), (192, 192, False, False),
            (384, 192, True, True), (576, 192, True, True), (32, 64, True, False), (160, 192, False, True))
RW_M = (1000, 31)
X3_GEO = ((2, 14, 0), (2, 14, 3), (2, 21, 0), (2, 21, 5))   # (B, hw, shift) added to the x3 block's 1e-5 rule

MLP_MUTANTS = ("b2drop", "tanh", "lncm1", "lnhalf", "nores_tail")
ATTN_MUTANTS = ("projb_shift", "lncm1", "lnhalf", "relpos_T", "mask_swap12", "roll_plus", "qscale_after", "pad_key")
RW_MUTANTS = ("rw_order",)
# mutant -> (kernel, rule, family)
CAUGHT_BY = {
    "b2drop": ("mlp", "rule1", "gauss"),
    "lnhalf": ("mlp", "rule1", "spike"),
    "nores_tail": ("mlp", "rule1", "offset"),
    "projb_shift": ("attn", "rule1", "gauss"),
    "relpos_T": ("attn", "rule1", "gauss"),
    "pad_key": ("attn", "rule1", "gauss"),        # on the shifted cases (shift 3) of every geometry
    "mask_swap12": ("attn", "locality", "gauss"),
    "roll_plus": ("attn", "locality", "gauss"),
    "rw_order": ("rw", "rule1", "gauss"),
}
# what rules 1 and 2 do not resolve at T <= 1000, and why (test_swin_fused_cpu.py asserts the measurements)
BELOW_NOISE = {
    "tanh": "tanh-GELU differs from erf-GELU by < 5e-4 per hidden unit, an even function of the pre-activation "
            "summed with random-sign fc2 weights: far below the rounding noise of the bf16 hidden",
    "lncm1": "variance / (C - 1) scales LN's output by sqrt(95 / 96) or sqrt(191 / 192), 0.5 % or 0.26 %: at the "
             "2^-9 rounding of that output; rule 2 sees it at C = 96, T = 1000 only",
    "qscale_after": "bf16(q) * scale and bf16(q * scale) both carry one 2^-9 rounding of q: the same noise",
}


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def bf(t):
    return t.to(torch.bfloat16)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def n_const(T):
    """Constant rows of a `constant` / `mixed` case of T tokens (module docstring)."""
    return T if T < 256 else int(math.sqrt(T) / 2)


def spike(n, i, g_):
    """N(0, 1) rows with channel (7 i) mod C of row i raised or lowered by 6 ... 8."""
    T, C = n.shape
    x = n + BASE
    sgn = torch.where(torch.rand(T, generator=g_) < 0.5, -1.0, 1.0)
    x[i, (7 * i) % C] += sgn * (6 + 2 * torch.rand(T, generator=g_))
    return x


def rows(fam, T, C, seed):
    """(T, C) bf16 token rows of one family."""
    g_ = _gen(11, FAMILIES.index(fam), C, T, seed)
    n = torch.randn(T, C, generator=g_)
    i = torch.arange(T)
    gauss = 1.5 * n + BASE
    if fam == "gauss":
        x = gauss
    elif fam == "offset":
        x = n + 20.0
    elif fam == "spike":
        x = spike(n, i, g_)
    elif fam in ("constant", "mixed"):
        vals = bf(torch.linspace(BASE - 4, BASE + 4, T + 2)[1:-1])[torch.randperm(T, generator=g_)].float()
        const = vals[:, None].expand(T, C)
        if fam == "constant":
            x = torch.where((i < n_const(T))[:, None], const, gauss)
        else:
            kind = i % 4
            kind = torch.where((kind == 3) & (i // 4 >= n_const(T)), i // 4 % 3, kind)   # cap the constant rows
            sp = spike(n, i, g_)
            x = torch.where((kind == 0)[:, None], gauss, torch.where((kind == 1)[:, None], n + 20.0,
                            torch.where((kind == 2)[:, None], sp, const)))
    else:
        raise ValueError(fam)
    return bf(x)


def perturb(x, idx):
    """x with channels 5, 40 and C - 1 of the token at `idx` (an index tuple) moved by +1, -1.5, +2 (bf16)."""
    x2 = x.clone()
    C = x.shape[-1]
    for c, d in ((5, 1.0), (40, -1.5), (C - 1, 2.0)):
        x2[idx + (c,)] = (x2[idx + (c,)].float() + d).to(x.dtype)
    assert not torch.equal(x2[idx], x[idx])
    return x2


# ------------------------------------------------------------------------------------------------ parameters
def mlp_params(C, seed=0):
    g_ = _gen(21, C, seed)
    r = lambda *s: torch.randn(*s, generator=g_)  # noqa: E731
    return {"g": 1 + 0.3 * r(C), "b": r(C), "w1": bf(2 * C ** -0.5 * r(4 * C, C)), "b1": r(4 * C),
            "w2": bf(0.5 * (4 * C) ** -0.5 * r(C, 4 * C)), "b2": r(C)}


def attn_params(seed=0, dtype=torch.bfloat16):
    """dtype: the weights' (bf16 for swin_attn_block; f32 for the x3 block)."""
    g_ = _gen(22, seed)
    r = lambda *s: torch.randn(*s, generator=g_)  # noqa: E731
    C = AC
    return {"g": 1 + 0.3 * r(C), "b": r(C), "wqkv": (C ** -0.5 * r(3 * C, C)).to(dtype), "bqkv": r(3 * C),
            "wp": (0.5 * C ** -0.5 * r(C, C)).to(dtype), "bp": r(C), "table": r((2 * WS - 1) ** 2, HEADS)}


def rw_params(N, K, bias, seed=0):
    g_ = _gen(23, N, K, seed)
    return {"w": bf(K ** -0.5 * torch.randn(N, K, generator=g_)), "b": torch.randn(N, generator=g_) if bias else None}


def rw_channel(row):
    """gemm_rw.hip's image row -> channel order (the mutant leaves the output in it)."""
    u, rho = row >> 5, row & 31
    i, h, rr = rho >> 3, (rho >> 2) & 1, rho & 3
    return 32 * u + 16 * (i >> 1) + 8 * h + 4 * (i & 1) + rr


# ------------------------------------------------------------------------------------------------ the chains
def _rd(t, rounded):
    return t.to(torch.bfloat16).to(t.dtype) if rounded else t


def _ln(x, g, b, eps, mutant):
    C = x.shape[-1]
    if mutant == "lnhalf":      # the sum of lane half 0 alone (channels 16 ks + 0..7), taken for the row's
        half = ((torch.arange(C) >> 3) & 1) == 0
        mean = x[..., half].mean(-1, keepdim=True)
    else:
        mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / (C - 1 if mutant == "lncm1" else C)
    return d / torch.sqrt(var + eps) * g + b


def mlp_chain(x, p, dt=torch.float64, rounded=False, mutant=None, eps=1e-5):
    """x (T, C) bf16 -> (T, C) of dt: R (dt f64, not rounded) or Mdl (dt f32, rounded)."""
    assert mutant in (None,) + MLP_MUTANTS
    xd = x.to(dt)
    q = {k: v.to(dt) for k, v in p.items()}
    h = _rd(_ln(xd, q["g"], q["b"], eps, mutant), rounded)
    a = h @ q["w1"].T + q["b1"]
    hid = _rd(F.gelu(a, approximate="tanh" if mutant == "tanh" else "none"), rounded)
    b2 = q["b2"].clone()
    if mutant == "b2drop":
        b2[int(b2.abs().argmax())] = 0
    res = xd.clone()
    if mutant == "nores_tail" and x.shape[0] % 32:
        res[x.shape[0] // 32 * 32:] = 0
    return hid @ q["w2"].T + b2 + res


def mlp_preact(x, p, eps=1e-5):
    q = {k: v.double() for k, v in p.items()}
    return _ln(x.double(), q["g"], q["b"], eps, None) @ q["w1"].T + q["b1"]


def window_types(hw):
    """type of every window in partition order: 2 (last window row) + (last window column)."""
    nw = hw // WS
    wy, wx = torch.arange(nw)[:, None].expand(nw, nw), torch.arange(nw)[None, :].expand(nw, nw)
    return (2 * (wy == nw - 1) + (wx == nw - 1)).reshape(-1)


def attn_chain(x, p, shift, dt=torch.float64, rounded=False, mutant=None, eps=1e-5):
    """x (B, hw, hw, 96) -> same shape of dt."""
    assert mutant in (None,) + ATTN_MUTANTS
    B, hw, _, C = x.shape
    N = WS * WS
    xd = x.to(dt)
    q_ = {k: v.to(dt) for k, v in p.items()}
    h = _rd(_ln(xd, q_["g"], q_["b"], eps, mutant), rounded)
    qkv = h @ q_["wqkv"].T + q_["bqkv"]
    sh = (-shift, shift) if mutant == "roll_plus" else (-shift, -shift)
    if shift:
        qkv = torch.roll(qkv, shifts=sh, dims=(1, 2))
    win = otw.window_partition(qkv, WS).view(-1, N, 3, HEADS, DH).permute(2, 0, 3, 1, 4)
    scale = DH ** -0.5
    q = _rd(win[0], rounded) * scale if mutant == "qscale_after" else _rd(win[0] * scale, rounded)
    k, v = _rd(win[1], rounded), _rd(win[2], rounded)
    a = q @ k.transpose(-2, -1)
    bias = q_["table"][otw.relative_position_index(WS).view(-1)].view(N, N, HEADS).permute(2, 0, 1)
    if mutant == "relpos_T":
        bias = bias.transpose(-1, -2)
    a = a + bias[None]
    if shift:
        m = otw.shift_mask(hw, hw, WS, shift).to(dt)
        if mutant == "mask_swap12":
            ty = window_types(hw)
            first = {int(t): int((ty == t).nonzero()[0]) for t in ty.unique()}
            m = torch.stack([m[first.get({1: 2, 2: 1}.get(int(t), int(t)), int(w))] for w, t in enumerate(ty)])
        a = (a.view(-1, m.shape[0], HEADS, N, N) + m[None, :, None]).view(-1, HEADS, N, N)
    if mutant == "pad_key":     # token 49 of the padded window (LN of a zero row = beta) admitted with bias 0
        hp = _rd(q_["b"], rounded)
        kvp = (hp @ q_["wqkv"].T + q_["bqkv"]).view(3, HEADS, DH)
        kp, vp = _rd(kvp[1], rounded), _rd(kvp[2], rounded)
        a = torch.cat([a, (q * kp[None, :, None, :]).sum(-1, keepdim=True)], -1)
        v = torch.cat([v, vp[None, :, None, :].expand(v.shape[0], HEADS, 1, DH)], 2)
    pu = torch.exp(a - a.max(-1, keepdim=True).values)
    o = _rd((_rd(pu, rounded) @ v) / pu.sum(-1, keepdim=True), rounded)
    o = o.transpose(1, 2).reshape(-1, N, C)
    bp = q_["bp"]
    if mutant == "projb_shift":
        bp = bp[(torch.arange(C) + 8) % C]
    o = o @ q_["wp"].T + bp
    o = otw.window_reverse(o.view(-1, WS, WS, C), WS, hw, hw)
    if shift:
        o = torch.roll(o, shifts=(-sh[0], -sh[1]), dims=(1, 2))
    return xd + o


def rw_chain(x, p, r=None, dt=torch.float64, mutant=None):
    assert mutant in (None,) + RW_MUTANTS
    y = x.to(dt) @ p["w"].to(dt).T
    if p["b"] is not None:
        y = y + p["b"].to(dt)
    if r is not None:
        y = y + r.to(dt)
    if mutant == "rw_order":
        y = y[:, torch.tensor([rw_channel(i) for i in range(y.shape[1])])]
    return y


# ------------------------------------------------------------------------------------------------ the rules
def sigma(mdl, R):
    return (mdl.double() - R).pow(2).mean().sqrt().item()


def rule1(y, R, sig):
    """worst |y - R| / (2^-8 |R| + 8 sigma)."""
    err = (y.detach().double().cpu() - R).abs()
    tol = (U8 * R.abs() + 8 * sig).clamp(min=1e-300)
    ra = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float("nan") if bool(torch.isnan(ra).any()) else ra.max().item()


def rule2(y, R, sig):
    """worst per-channel |mean_t (y - R)| / (8 (sigma + 2^-9 rms_t R) / sqrt(T)); None below 256 tokens."""
    C = R.shape[-1]
    d = (y.detach().double().cpu() - R).reshape(-1, C)
    T = d.shape[0]
    if T < 256:
        return None
    tol = 8 * (sig + 2.0 ** -9 * R.reshape(-1, C).pow(2).mean(0).sqrt()) / math.sqrt(T)
    ra = d.mean(0).abs() / tol.clamp(min=1e-300)
    return float("nan") if bool(torch.isnan(ra).any()) else ra.max().item()


def judge(y, R, sig):
    """(rule 1 ratio, rule 2 ratio or 0.0 where it does not apply)."""
    r2 = rule2(y, R, sig)
    return rule1(y, R, sig), (0.0 if r2 is None else r2)


# ------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def mlp_case(fam, T, C, seed=0):
    p = mlp_params(C, seed)
    x = rows(fam, T, C, seed)
    R = mlp_chain(x, p)
    mdl = mlp_chain(x, p, torch.float32, True)
    return {"x": x, "p": p, "R": R, "mdl": mdl, "sigma": sigma(mdl, R)}


@functools.lru_cache(maxsize=None)
def attn_case(fam, B, hw, shift, seed=0):
    p = attn_params(seed)
    x = rows(fam, B * hw * hw, AC, seed + hw).view(B, hw, hw, AC)
    R = attn_chain(x, p, shift)
    mdl = attn_chain(x, p, shift, torch.float32, True)
    return {"x": x, "p": p, "R": R, "mdl": mdl, "sigma": sigma(mdl, R)}


@functools.lru_cache(maxsize=None)
def rw_case(fam, M, N, K, bias, res, seed=0):
    p = rw_params(N, K, bias, seed)
    x = rows(fam, M, K, seed)
    r = rows("gauss", M, N, seed + 1) if res else None
    R = rw_chain(x, p, r)
    mdl = rw_chain(x, p, r, torch.float32)
    return {"x": x, "p": p, "r": r, "R": R, "mdl": mdl, "sigma": sigma(mdl, R)}


# ------------------------------------------------------------------------------------------------ locality
def locality_tokens(hw, shift):
    """(row, col) in the image of the tokens part B perturbs: one in an interior (type 0) window, one in a
    right-edge, a bottom-edge and the corner window, one that the roll wraps round the image (shift > 0), and at
    hw >= 21 one in a window that touches no edge; picked in rolled coordinates, returned in the image's."""
    rc = [(3, 3), (3, hw - 4), (hw - 4, 3), (hw - 4, hw - 4), (hw - 1, hw - 2)]
    if hw >= 21:
        rc.append((10, 9))
    return [((r + shift) % hw, (c + shift) % hw) for r, c in rc]


def allowed_region(hw, shift, row, col):
    """(hw, hw) bool: the tokens whose output may depend on token (row, col): its window after the roll, cut to
    the queries whose shift mask admits it as a key.  From oracle.towers' roll / partition / mask alone."""
    ids = torch.arange(hw * hw).view(1, hw, hw, 1)
    if shift:
        ids = torch.roll(ids, shifts=(-shift, -shift), dims=(1, 2))
    win = otw.window_partition(ids, WS).view(-1, WS * WS)
    w, pos = (win == row * hw + col).nonzero()[0].tolist()
    ok = torch.ones(WS * WS, dtype=torch.bool)
    if shift:
        ok = otw.shift_mask(hw, hw, WS, shift)[w][:, pos] == 0
    out = torch.zeros(hw * hw, dtype=torch.bool)
    out[win[w][ok]] = True
    return out.view(hw, hw)


def changed_tokens(y, y2):
    """(..., ) bool over tokens: any channel differs bit for bit."""
    return (bits(y.detach().cpu()) != bits(y2.detach().cpu())).any(-1)


def locality_verdict(changed, hw, shift, b, row, col):
    """Part B's predicate on changed (B, hw, hw) for a perturbation of token (b, row, col): None if it holds, else
    what broke."""
    allow = torch.zeros_like(changed)
    allow[b] = allowed_region(hw, shift, row, col)
    if bool((changed & ~allow).any()):
        return f"{int((changed & ~allow).sum())} tokens outside the allowed region changed"
    if not bool(changed[b, row, col]):
        return "the perturbed token's own output did not change"
    if int(changed.sum()) < 2:
        return "no other token of the region changed"
    return None
