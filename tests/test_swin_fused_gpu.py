"""GPU: persistent-walk, locality and per-element tests of the fused Swin stage 1-2 kernels (mmr_swin_mlp at C = 96
swin_mlp_sp and C = 192 swin_mlp, mmr_swin_attn_block, mmr_x3_swin_attn_block, mmr_linear_rw; locality also for
mmr_x3_swin_mlp and mmr_x3_rowlin) against swin_fused_ref.py.

A  walk invariance.  The persistent kernels launch min(CUs, units / waves) workgroups and every wave walks its
   units with a stride of G = grid * waves.  One launch of n = 2 G + G / 2 + 3 units (every wave takes two, the
   first G / 2 + 3 a third: the last round is partial) must equal, bit for bit, the same outputs computed in
   launches of at most CUs units (no wave takes a second unit: the regime test_towers_gpu.py / test_x3_gpu.py
   cover).  About 64 units of the first, a middle and the last round are also held to the f64 reference by the
   rules of part C.  The streamed C = 192 MLP is not persistent; it gets the same identity over 300 workgroups.
B  locality.  One token of the input is moved by O(1) in three channels; outputs are compared bit for bit.  Token
   kernels: exactly that token's row changes.  Attention blocks: the changed tokens lie inside the perturbed
   token's window after the roll and, shifted, inside its mask region (swin_fused_ref.allowed_region, from
   oracle.towers), the token itself and at least one more change, everything else is bit-identical.
C  rules 1 and 2 of swin_fused_ref.py against f64 for the three bf16 kernels on the five input families; the x3
   attention block keeps its 1e-5 of max|ref| rule and gains the hw = 14 and hw = 21 geometries.
test_zz_report prints the worst measured ratios per kernel.

Measured on an MI355X (256 CUs).  Part A launches, units = 2 G + G / 2 + 3 (rounded up to whole images), every wave
2 or 3 rounds:
  swin_mlp_sp          5124 tiles (T = 163955) and 5123 tiles (T = 163905), G = 2048
  swin_attn_block      5124 windows (hw = 14, shift 3) and 5123 windows (hw = 7), G = 2048
  x3_swin_attn_block   2564 and 2563 windows, G = 1024
  gemm_rw 576 x 192    2563 tiles (M = 82007), 2 parts, 1 workgroup per CU, G = 1024
  gemm_rw 96 x 64      20483 tiles (M = 655447), 1 part, 4 workgroups per CU, G = 8192
Every bitwise expectation of parts A and B held.  Worst ratios (rule 1, rule 2), part A's samples included:
  swin_mlp C = 96 0.798, 0.387;  swin_mlp C = 192 0.826, 0.315;  swin_attn_block 0.898, 0.427;
  linear_rw 0.996, 0.399 (rule 1 there is the output rounding alone);  x3 block <= 4.2e-6 of max|ref|.
The file runs in 4 s (58 tests, the slowest 0.6 s).
Scratch wrong-kernel builds, not committed, whole GPU suite run against each:
  swin_attn_block, the next window's gather not issued before a wave's last round (its last window then reads the
      previous window's rows from LDS): both test_walk_swin_attn_block cases fail (100352 tokens differ at
      hw = 14), no other test of the suite does, the B = 256 end-to-end tests included.
  swin_mlp_sp, b2 read one 8-channel chunk further on: 7 tests here fail (both resident walks through their f64
      samples, test_rules_swin_mlp at C = 96 and every T), and 8 older ones (test_swin_mlp_fused at C = 96, the
      full-size tower, fusion and end-to-end tests).
  swin_attn_block, the loop-top s_waitcnt vmcnt(12) relaxed to vmcnt(22) (the gather no longer counted): nothing
      fails, old or new, and rightly: hipcc itself waits vmcnt(0) before the epilogue's first use of the residual
      rows, after the gather is issued, so in this build the gather has always landed before the loop top and the
      hand-written count is not what orders it."""
import json

import pytest
import torch

import swin_fused_ref as S
from mmr_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}          # kernel -> [rule 1, rule 2], filled by part A's samples and part C
WALKS = {}          # part A: kernel -> units, G, rounds


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _note(kernel, r1, r2):
    w = WORST.setdefault(kernel, [0.0, 0.0])
    w[0], w[1] = max(w[0], r1), max(w[1], r2)


def _hold(kernel, y, R, mdl, tag, model_too=False):
    """Rules 1 and 2 for kernel output y against R with sigma = RMS(mdl - R)."""
    sig = S.sigma(mdl, R)
    if model_too:      # part A's samples are drawn on the GPU: the model's own margin is checked here
        m1, m2 = S.judge(mdl, R, sig)
        assert m1 <= S.MODEL_MAX and m2 <= S.MODEL_MAX, (tag, "model", m1, m2)
    r1, r2 = S.judge(y, R, sig)
    print(json.dumps({"kernel": kernel, "case": tag, "sigma": sig, "rule1": round(r1, 4), "rule2": round(r2, 4)}))
    _note(kernel, r1, r2)
    assert r1 <= 1.0, (tag, "rule 1", r1)
    assert r2 <= 1.0, (tag, "rule 2", r2)


def _units(G):
    return 2 * G + G // 2 + 3


def _sample(n, G, per_round=21):
    """~64 unit indices: first round, second round, the partial last round."""
    assert n > 2 * G
    last = n - 2 * G
    pick = lambda lo, cnt: [lo + (j * cnt) // per_round for j in range(per_round)]  # noqa: E731
    return sorted(set(pick(0, G) + pick(G, G) + pick(2 * G, last) + [n - 1]))


def _big_rows(T, C, seed, dtype=torch.bfloat16):
    """gauss rows of swin_fused_ref (1.5 N + 8), drawn on the GPU: distinct data for every token."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (1.5 * torch.randn(T, C, generator=g, device=DEV) + S.BASE).to(dtype)


def _dev(p):
    return {k: (v.to(DEV) if v is not None else None) for k, v in p.items()}


# ------------------------------------------------------------------------------------------------ launchers
def _mlp_fn(C):
    p = S.mlp_params(C)
    d = _dev(p)
    pack = ops.swin_mlp_pack(d["w1"], d["w2"])
    assert pack is not None
    return p, lambda x: ops.swin_mlp(x, d["g"], d["b"], pack, d["b1"], d["b2"], 1e-5)


def _attn_fn(hw, shift):
    p = S.attn_params(0)
    d = _dev(p)
    pack = ops.swin_attn_block_pack(d["wqkv"], d["bqkv"], d["wp"], d["bp"], d["g"], d["b"])
    assert pack is not None
    bias = ops.swin_attn_bias(d["table"], S.HEADS, S.WS, hw, shift)
    return p, lambda x: ops.swin_attn_block(x, pack, bias, S.WS, shift, 1e-5)


def _x3_attn_fn(hw, shift):
    p = S.attn_params(1, torch.float32)
    d = _dev(p)
    pack = ops.x3_swin_attn_block_pack(d["wqkv"], d["bqkv"], d["wp"], d["bp"], d["g"], d["b"])
    assert pack is not None
    bias = ops.swin_attn_bias(d["table"], S.HEADS, S.WS, hw, shift)
    return p, lambda x: ops.x3_swin_attn_block(x, pack, bias, S.WS, shift, 1e-5)


def _rw_fn(N, K, bias):
    p = S.rw_params(N, K, bias)
    d = _dev(p)
    pack = ops.rw_pack(d["w"])
    assert pack is not None
    return p, lambda x, r=None: ops.linear_rw(x, pack, d["b"], r)


def _chunks(fn, x, rows, *more):
    """fn over consecutive slices of `rows` leading entries, concatenated."""
    out = [fn(x[a:a + rows], *(m[a:a + rows] if m is not None else None for m in more))
           for a in range(0, x.shape[0], rows)]
    return torch.cat(out)


# ------------------------------------------------------------------------------------------------ A: walks
@pytest.mark.parametrize("odd", [False, True])
def test_walk_swin_mlp_resident(odd):
    """swin_mlp_sp (C = 96): launch_sp's grid = min(CUs, ceil(ceil(T / 32) / 8)), 8 waves, wave stride grid * 8
    tiles of 32 tokens.  T is no multiple of 32; `odd`: an odd tile count."""
    C, NW, cus = 96, 8, _cus()
    n = _units(cus * NW)
    n += (n % 2 == 0) if odd else (n % 2 == 1)
    T = 32 * n - (31 if odd else 13)
    ntile = -(-T // 32)
    G = min(cus, -(-ntile // NW)) * NW
    assert ntile == n and ntile % 2 == int(odd) and T % 32 and n > 2 * G
    WALKS[f"swin_mlp_sp T={T}"] = {"units": n, "G": G, "rounds": [n // G, -(-n // G)]}
    p, fn = _mlp_fn(C)
    x = _big_rows(T, C, 11 + odd)
    big = fn(x)
    small = _chunks(fn, x, 32 * cus)
    torch.cuda.synchronize()
    assert torch.equal(big, small), int((S.bits(big) != S.bits(small)).any(1).sum())
    tiles = _sample(n, G)
    idx = torch.cat([torch.arange(32 * t, min(32 * t + 32, T)) for t in tiles])
    xs = x[idx.to(DEV)].cpu()
    _hold("swin_mlp C=96", big[idx.to(DEV)], S.mlp_chain(xs, p), S.mlp_chain(xs, p, torch.float32, True),
          f"walk T={T}", model_too=True)


def test_walk_swin_mlp_streamed():
    """swin_mlp (C = 192): one workgroup per 256 tokens, no loop; 300 workgroups and a ragged tail against launches
    of 8192 tokens."""
    C, T = 192, 256 * 300 + 77
    p, fn = _mlp_fn(C)
    x = _big_rows(T, C, 13)
    big = fn(x)
    small = _chunks(fn, x, 8192)
    torch.cuda.synchronize()
    assert torch.equal(big, small), int((S.bits(big) != S.bits(small)).any(1).sum())
    idx = torch.cat([torch.arange(a, a + 32) for a in (0, 256 * 150 + 96, T - 32)])
    xs = x[idx.to(DEV)].cpu()
    _hold("swin_mlp C=192", big[idx.to(DEV)], S.mlp_chain(xs, p), S.mlp_chain(xs, p, torch.float32, True),
          f"walk T={T}")


def _walk_attention(kernel, NW, hw, shift, make, dtype):
    """Shared by the two attention blocks: grid = min(CUs, ceil(windows / NW)), one window per wave and round."""
    cus = _cus()
    per_img = (hw // S.WS) ** 2
    B = -(-_units(cus * NW) // per_img)
    n = B * per_img
    G = min(cus, -(-n // NW)) * NW
    assert n > 2 * G and n % G and n - 2 * G < G
    WALKS[f"{kernel} hw={hw} shift={shift}"] = {"units": n, "G": G, "rounds": [n // G, -(-n // G)]}
    p, fn = make(hw, shift)
    x = _big_rows(B * hw * hw, S.AC, 17 + hw, dtype).view(B, hw, hw, S.AC)
    big = fn(x)
    small = _chunks(fn, x, max(1, cus // per_img))
    torch.cuda.synchronize()
    assert torch.equal(big, small), int((S.bits(big) != S.bits(small)).any(-1).sum())
    imgs = torch.tensor(sorted({w // per_img for w in _sample(n, G, 21 if per_img == 1 else 6)}))
    return p, x[imgs.to(DEV)].cpu(), big[imgs.to(DEV)], n


@pytest.mark.parametrize("hw,shift", [(14, 3), (7, 0)])
def test_walk_swin_attn_block(hw, shift):
    """swin_attn_block: 8 waves; the next window's gather into the wave's LDS buffer, the vmcnt(12) at the loop
    top and the residual rows kept across it all run from the second window of a wave on."""
    p, xs, ys, n = _walk_attention("swin_attn_block", 8, hw, shift, _attn_fn, torch.bfloat16)
    _hold("swin_attn_block", ys, S.attn_chain(xs, p, shift), S.attn_chain(xs, p, shift, torch.float32, True),
          f"walk hw={hw} shift={shift} windows={n}", model_too=True)


@pytest.mark.parametrize("hw,shift", [(14, 3), (7, 0)])
def test_walk_x3_swin_attn_block(hw, shift):
    """x3_swin_attn_block: 4 waves; the sampled images keep the block's 1e-5 of max|ref| rule."""
    p, xs, ys, n = _walk_attention("x3_swin_attn_block", 4, hw, shift, _x3_attn_fn, torch.float32)
    ref = S.attn_chain(xs, p, shift)
    err = (ys.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(json.dumps({"kernel": "x3_swin_attn_block", "case": f"walk hw={hw} windows={n}", "rel": err}))
    assert err <= 1e-5


@pytest.mark.parametrize("N,K", [(576, 192), (96, 64)])
def test_walk_linear_rw(N, K):
    """gemm_rw: launch_rw's grid.x = max(1, min(CUs * per_cu / parts, ceil(tiles / 8))) with parts =
    mmr_linear_rw_parts(N, K), per_cu = max(1, min(4, 160 KiB / (N / parts * K * 2 + N / parts * 4))), 8 waves,
    wave stride grid.x * 8 tiles of 32 rows; (576, 192): 2 parts, 1 per CU; (96, 64): 1 part, 4 per CU.  With bias
    and residual, M ragged."""
    NW, cus = 8, _cus()
    parts = int(_lib.lib().mmr_linear_rw_parts(N, K))
    assert parts > 0
    no = N // parts
    per_cu = max(1, min(4, (160 * 1024) // (no * K * 2 + no * 4)))
    assert (parts, per_cu) == {(576, 192): (2, 1), (96, 64): (1, 4)}[(N, K)]
    n = _units(max(1, cus * per_cu // parts) * NW)
    M = 32 * n - 9
    tiles = -(-M // 32)
    G = max(1, min(cus * per_cu // parts, -(-tiles // NW))) * NW
    assert tiles == n and n > 2 * G and M % 32
    WALKS[f"gemm_rw {N}x{K} M={M}"] = {"units": n, "G": G, "rounds": [n // G, -(-n // G)], "parts": parts,
                                        "per_cu": per_cu}
    p, fn = _rw_fn(N, K, True)
    x, r = _big_rows(M, K, 19 + N), _big_rows(M, N, 23 + N)
    big = fn(x, r)
    small = _chunks(fn, x, 32 * cus, r)
    torch.cuda.synchronize()
    assert torch.equal(big, small), int((S.bits(big) != S.bits(small)).any(1).sum())
    idx = torch.cat([torch.arange(32 * t, min(32 * t + 32, M)) for t in _sample(n, G)]).to(DEV)
    xs, rs = x[idx].cpu(), r[idx].cpu()
    _hold("linear_rw", big[idx], S.rw_chain(xs, p, rs), S.rw_chain(xs, p, rs, torch.float32), f"walk {N}x{K} M={M}",
          model_too=True)


# ------------------------------------------------------------------------------------------------ B: locality
def _token_kernel(name):
    """(fn, x) of a token kernel at a ragged row count spanning more than one workgroup."""
    T = 32 * 9 + 7
    if name.startswith("swin_mlp"):
        C = int(name[-3:].strip("_"))
        return _mlp_fn(C)[1], S.rows("gauss", T, C, 3).to(DEV)
    if name.startswith("rw"):
        N, K = {"rw_576x192": (576, 192), "rw_96x64": (96, 64)}[name]
        fn = _rw_fn(N, K, True)[1]
        r = S.rows("gauss", T, N, 4).to(DEV)
        return (lambda x: fn(x, r)), S.rows("gauss", T, K, 3).to(DEV)
    C = 192 if name.endswith("192") else 96
    g_ = torch.Generator().manual_seed(5)
    x = (1.5 * torch.randn(T, C, generator=g_) + 0.3).to(DEV)
    p = {k: v.float().to(DEV) for k, v in S.mlp_params(C).items()}
    if name.startswith("x3_swin_mlp"):
        pack = ops.x3_swin_mlp_pack(p["w1"], p["w2"])
        assert pack is not None
        return (lambda t: ops.x3_swin_mlp(t, p["g"], p["b"], pack, p["b1"], p["b2"], 1e-5)), x
    w = p["w1"][:3 * C].contiguous()                      # x3_rowlin: LN + (3C x C) linear, the norm1 + qkv shape
    pack = ops.x3_rowlin_pack(w)
    assert pack is not None
    return (lambda t: ops.x3_rowlin(t, pack, p["b1"][:3 * C].contiguous(), 3 * C, ln=(p["g"], p["b"], 1e-5))), x


@pytest.mark.parametrize("name", ["swin_mlp_96", "swin_mlp_192", "rw_576x192", "rw_96x64", "x3_swin_mlp_96",
                                  "x3_swin_mlp_192", "x3_rowlin_96", "x3_rowlin_192"])
def test_locality_token_kernels(name):
    """Exactly the perturbed token's row changes: the first token, one of the last ragged tile, the last."""
    fn, x = _token_kernel(name)
    T = x.shape[0]
    y = fn(x)
    for t in (0, T - 5, T - 1):
        ch = S.changed_tokens(y, fn(S.perturb(x, (t,))))
        assert ch.nonzero().flatten().tolist() == [t], (name, t, ch.nonzero().flatten().tolist())


@pytest.mark.parametrize("kernel", ["swin_attn_block", "x3_swin_attn_block"])
@pytest.mark.parametrize("hw,shift", [(14, 0), (14, 3), (14, 5), (21, 0), (21, 3), (21, 5)])
def test_locality_attention(kernel, hw, shift):
    B = 2
    if kernel == "swin_attn_block":
        fn = _attn_fn(hw, shift)[1]
        x = S.rows("gauss", B * hw * hw, S.AC, 7 * hw + shift).view(B, hw, hw, S.AC).to(DEV)
    else:
        fn = _x3_attn_fn(hw, shift)[1]
        x = S.rows("gauss", B * hw * hw, S.AC, 7 * hw + shift).float().view(B, hw, hw, S.AC).to(DEV)
    y = fn(x)
    bad = []
    for row, col in S.locality_tokens(hw, shift):
        y2 = fn(S.perturb(x, (1, row, col)))
        ch = S.changed_tokens(y, y2)
        v = S.locality_verdict(ch, hw, shift, 1, row, col)
        if v is not None:      # which tokens moved, and by how much
            d = (y2.double() - y.double()).abs().amax(-1).cpu()
            allow = torch.zeros_like(ch)
            allow[1] = S.allowed_region(hw, shift, row, col)
            out = (ch & ~allow).nonzero().tolist()
            bad.append({"token": (row, col), "verdict": v, "outside": out[:20], "max_moved": d[ch & ~allow].max().item()
                        if out else 0.0})
    assert not bad, json.dumps(bad)


# ------------------------------------------------------------------------------------------------ C: rules
@pytest.mark.parametrize("T", S.MLP_T)
@pytest.mark.parametrize("C", S.MLP_C)
def test_rules_swin_mlp(C, T):
    _, fn = _mlp_fn(C)
    for fam in S.FAMILIES:
        k = S.mlp_case(fam, T, C)
        _hold(f"swin_mlp C={C}", fn(k["x"].to(DEV)), k["R"], k["mdl"], f"T={T} {fam}")


@pytest.mark.parametrize("shift", S.ATTN_SHIFTS)
@pytest.mark.parametrize("B,hw", S.ATTN_GEO)
def test_rules_swin_attn_block(B, hw, shift):
    _, fn = _attn_fn(hw, shift)
    for fam in S.FAMILIES:
        k = S.attn_case(fam, B, hw, shift)
        _hold("swin_attn_block", fn(k["x"].to(DEV)), k["R"], k["mdl"], f"B={B} hw={hw} shift={shift} {fam}")


@pytest.mark.parametrize("N,K,bias,res", S.RW_CASES)
def test_rules_linear_rw(N, K, bias, res):
    _, fn = _rw_fn(N, K, bias)
    for M in S.RW_M:
        for fam in S.FAMILIES:
            k = S.rw_case(fam, M, N, K, bias, res)
            y = fn(k["x"].to(DEV), k["r"].to(DEV) if res else None)
            _hold("linear_rw", y, k["R"], k["mdl"], f"{N}x{K} M={M} {fam}")


@pytest.mark.parametrize("B,hw,shift", S.X3_GEO)
def test_x3_swin_attn_block_geometries(B, hw, shift):
    """The block's existing rule (max|err| <= 1e-5 max|ref| against f64, test_x3_gpu.py) at hw = 14 and hw = 21."""
    p, fn = _x3_attn_fn(hw, shift)
    g_ = torch.Generator().manual_seed(hw + shift)
    x = torch.randn(B, hw, hw, S.AC, generator=g_)
    y = fn(x.to(DEV))
    ref = S.attn_chain(x, p, shift)
    err = (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(json.dumps({"kernel": "x3_swin_attn_block", "case": f"B={B} hw={hw} shift={shift}", "rel": err}))
    assert torch.isfinite(y).all() and err <= 1e-5


def test_zz_report():
    """Worst measured ratios (rule 1, rule 2) per kernel and the part-A walks, for the record."""
    print(json.dumps({"worst": WORST, "walks": WALKS}))
