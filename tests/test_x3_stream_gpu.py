"""GPU: grid-stride walk, locality, per-element and refusal tests of the streamed x3 kernels of csrc/x3_mlp.hip
(mmr_x3_swin_mlp, mmr_x3_rowlin, mmr_x3_patch_embed_ln, mmr_patch_embed_ln_bf16) against x3_stream_ref.py.

A  stem walk.  patch_embed_ln() launches min(2048, tiles / 4) workgroups of 4 waves, one 32-token tile per wave and
   round (stride G = 8192 tiles).  One launch of B = 1139 images of 96 x 96 (18 tiles each, tiles straddling patch
   rows; 20502 tiles >= 2 G + G / 2 + 3: every wave takes two tiles, the first 4118 a third, and 20502 = 2 mod 4
   leaves the last workgroup half idle) must equal, bit for bit, the same images in launches of 455 (8190 tiles: no
   wave takes a second).  About 64 tiles of the first, the second and the partial last round are held to the f64
   reference by the rules of part C (x3) or the bf16 stem's per-element rule; one pixel of an image of the second
   round is moved and exactly its token changes.
B  stem locality, both forms, hw = 32 and 96: one pixel moved by 1 changes exactly the token (yy // 4, xx // 4) of
   its image, every other output stays bit-identical (patch corners, last row and column, each input channel);
   an all-zero image gives one token, LN(bias), everywhere.  (The MLP and rowlin keep their locality tests in
   test_swin_fused_gpu.py.)
C  rules 1-4 of x3_stream_ref.py for x3_swin_mlp (C = 96 in both workgroup forms, bit-identical, and C = 192),
   x3_rowlin and the x3 stem over the case lists of x3_stream_ref.py; the bf16 stem on the same images under
   |y - R| <= 2^-8 |R| + 2e-3.
D  refusals: a non-zero status (None from the ops pack helpers) and a poisoned output buffer left untouched;
   tokens = 0 and b = 0 return OK and write nothing.
test_zz_report prints the worst measured ratios per kernel and part A's counts.

Measured on an MI355X.  Part A: 20502 tiles, G = 8192, every wave 2 or 3 rounds, 4118 tiles in the third; both
forms bit-identical to the launches of 455 images, the moved pixel of image 682 (second round) changed its token
alone.  Every bitwise expectation of part B and every refusal of part D held; no defect was found in x3_mlp.hip.
Worst ratios (max|e|, rule 2, rule 3, rule 4; in s), part A's sample included:
  x3_swin_mlp C = 96     0.0045, 5.40, 1.57, 1.42        (the model on the CPU: 0.0044, 5.43, 1.60, 1.40)
  x3_swin_mlp C = 192    0.0019, 4.99, 1.31, 1.51        (0.0019, 5.12, 1.31, 1.51)
  x3_rowlin              0.090, 6.56, 1.48, 1.46         (0.089, 5.95, 1.49, 1.45)
  x3_patch_embed_ln      0.074, 5.98, 1.61, 2.00         (0.074, 5.97, 1.61, 2.00)
  patch_embed_ln_bf16    0.88 of 2^-8 |R| + 2e-3
The file runs in 3.6 s (112 tests; the slowest, test_walk_stem[True], 0.6 s).
Scratch wrong-kernel builds, wrong in value only, not committed, whole GPU suite run against each (with plain
1.5 N pixels in the hw = 224 gauss and constant cases, which no outcome below rests on):
  x3_swin_mlp, the w_lo . h_hi MFMA left out of fc2's last k-step: all 32 test_rules_x3_swin_mlp cases fail
      (T = 1000 gauss: rule 2 at 292 s, rule 3 at 89 s, rule 4 at 141 s, while max|e| = 0.25 stays inside rule 1:
      the worst-case bound alone does not see it), and of the older tests the 4 cases of
      test_x3_gpu.py::test_x3_swin_mlp_vs_f64 (2e-4 ... 3e-4 of max|ref| against 1e-5); nothing else, the x3
      tower and B = 256 end-to-end tests included.
  the stem, gamma read 4 channels further on for the tiles of the second and later rounds: both test_walk_stem
      cases fail (393920 tokens differ: the 12310 tiles past the first round), and no other test of the suite,
      old or new."""
import json

import pytest
import torch
import torch.nn.functional as F

import rowwise_ref as RW
import x3_stream_ref as S
from mmr_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}          # kernel -> [max|e|, rule 2, rule 3, rule 4]
WALKS = {}
POISON = 777.0


def _dev(p):
    return {k: v.to(DEV) for k, v in p.items()}


def _hold(kernel, y, k, tag):
    """Rules 1-4 for a kernel's output y on case k (R, W, and s from the model on the CPU)."""
    j = S.judge(y, k["R"], k["W"], k["s"])
    print(json.dumps({"kernel": kernel, "case": tag, "s": round(k["s"], 5), "max|e|": round(j[0], 4),
                      "rule2": round(j[1], 3), "rule3": round(j[2], 3), "rule4": round(j[3], 3)}))
    w = WORST.setdefault(kernel, [0.0] * 4)
    for i in range(4):
        w[i] = max(w[i], j[i])
    assert S.verdict(j) is None, (tag, S.verdict(j), j)


def _hold_bf16(y, R, tag):
    err = (y.double().cpu() - R).abs()
    ra = (err / S.stem_bf16_tol(R)).max().item()
    w = WORST.setdefault("patch_embed_ln_bf16", [0.0])
    w[0] = max(w[0], ra)
    assert y.dtype == torch.bfloat16 and ra <= 1.0, (tag, ra)


# ------------------------------------------------------------------------------------------------ launchers
def _mlp_fn(C, form=None):
    """form: None (the default launch) or the PIN_X3_MLP value (0: 8-wave, 1: 4-wave workgroups at C = 96)."""
    d = _dev(S.mlp_params(C))
    pack = ops.x3_swin_mlp_pack(d["w1"], d["w2"])
    assert pack is not None

    def fn(x):
        if form is None:
            return ops.x3_swin_mlp(x, d["g"], d["b"], pack, d["b1"], d["b2"], S.EPS)
        with ops.pinned(ops.PIN_X3_MLP, form):
            return ops.x3_swin_mlp(x, d["g"], d["b"], pack, d["b1"], d["b2"], S.EPS)
    return fn


def _row_run(k, c, n, mode):
    d = _dev(k["p"])
    pack = ops.x3_rowlin_pack(d["w"])
    assert pack is not None
    res = k["res"].to(DEV) if k["res"] is not None else None
    if mode.startswith("ln"):
        return ops.x3_rowlin(k["x"].to(DEV), pack, d["bias"], n, ln=(d["g"], d["b"], S.EPS), residual=res)
    kp = int(_lib.lib().mmr_x3_p8_kpad(c))
    xr = ops.X3Rows(S.split_rows(k["x"], kp).to(DEV), c, kp, (k["x"].shape[0],))
    return ops.x3_rowlin(xr, pack, d["bias"], n, residual=res)


def _stem_fn(p, x3):
    d = _dev(p)
    w = d["w"] if x3 else S.bf(d["w"]).float()
    pack = ops.x3_patch_embed_pack(w.reshape(96, 48).contiguous())
    assert pack is not None
    op = ops.x3_patch_embed_ln if x3 else ops.patch_embed_ln_bf16
    return lambda img: op(img, pack, d["bias"], d["g"], d["b"], S.EPS)


# ------------------------------------------------------------------------------------------------ A: the walk
def _sample(n, G, per_round=21):
    """~64 tile indices: first round, second round, the partial last round."""
    last = n - 2 * G
    pick = lambda lo, cnt: [lo + (j * cnt) // per_round for j in range(per_round)]  # noqa: E731
    return sorted(set(pick(0, G) + pick(G, G) + pick(2 * G, last) + [n - 1]))


@pytest.mark.parametrize("x3", [True, False])
def test_walk_stem(x3):
    hw, B, small, NW = 96, 1139, 455, 4
    per_img = (hw // 4) ** 2 // 32
    n = B * per_img
    G = min(2048, -(-n // NW)) * NW
    assert per_img == 18 and n == 20502 and G == 8192 and n >= 2 * G + G // 2 + 3 and n % NW == 2
    assert small * per_img <= min(2048, -(-small * per_img // NW)) * NW         # no second tile in the small launches
    WALKS[f"stem x3={x3}"] = {"tiles": n, "G": G, "rounds": [n // G, -(-n // G)], "third_round_tiles": n - 2 * G}
    p = S.stem_params()
    fn = _stem_fn(p, x3)
    g_ = torch.Generator(device=DEV).manual_seed(29 + x3)
    img = 1.5 * torch.randn(B, 3, hw, hw, generator=g_, device=DEV)
    big = fn(img)
    parts = torch.cat([fn(img[a:a + small]) for a in range(0, B, small)])
    torch.cuda.synchronize()
    assert torch.equal(big, parts), int((S.bits(big) != S.bits(parts)).any(-1).sum())
    del parts
    # f64 sample: the tokens of ~64 tiles from the three rounds
    tiles = _sample(n, G)
    assert tiles[0] < G <= tiles[len(tiles) // 2] < 2 * G <= tiles[-1]
    imgs = sorted({t // per_img for t in tiles})
    sub = img[torch.tensor(imgs, device=DEV)].cpu()
    R, W = S.stem_R(sub, p, x3)
    pos = {b: i for i, b in enumerate(imgs)}
    idx = torch.cat([torch.arange(32) + 32 * (per_img * pos[t // per_img] + t % per_img) for t in tiles])
    ys = big[torch.tensor(imgs, device=DEV)].reshape(-1, 96)[idx.to(DEV)]
    Rs, Ws = R.reshape(-1, 96)[idx], W.reshape(-1, 96)[idx]
    if x3:
        mdl = S.stem_M(sub, p).reshape(-1, 96)[idx]
        _hold("x3_patch_embed_ln", ys, {"R": Rs, "W": Ws, "s": S.noise(mdl, Rs, Ws)}, f"walk tiles={n}")
    else:
        _hold_bf16(ys, Rs, f"walk tiles={n}")
    # locality inside the second round: image 682 holds tiles 12276 .. 12293
    b, ch, yy, xx = (G + G // 2) // per_img, 1, 50, 43
    assert G <= b * per_img < 2 * G - per_img
    img[b, ch, yy, xx] += 1.0
    ch_tok = (S.bits(fn(img)) != S.bits(big)).any(-1).nonzero().tolist()
    assert ch_tok == [[b, yy // 4, xx // 4]], ch_tok[:8]


# ------------------------------------------------------------------------------------------------ B: locality
def _pixels(hw):
    """(b, ch, yy, xx): patch corners (xx % 4 in {0, 3}), the last row and column, every input channel."""
    return [(0, 0, 0, 0), (1, 1, 5, 7), (1, 2, hw - 1, hw - 1), (0, 0, hw - 1, 4), (1, 1, 6, hw - 1), (0, 2, 3, 3),
            (1, 0, hw // 2 + 1, hw // 2 - 4)]


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("hw", [32, 96])
def test_locality_stem(hw, x3):
    fn = _stem_fn(S.stem_params(), x3)
    img = S.images("gauss", 2, hw, 5).to(DEV)
    y = fn(img)
    for b, ch, yy, xx in _pixels(hw):
        img2 = img.clone()
        img2[b, ch, yy, xx] += 1.0
        changed = (S.bits(fn(img2)) != S.bits(y)).any(-1).nonzero().tolist()
        assert changed == [[b, yy // 4, xx // 4]], ((b, ch, yy, xx), changed[:8])


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("hw", [32, 96])
def test_zero_image_gives_ln_of_the_bias(hw, x3):
    p = S.stem_params()
    y = _stem_fn(p, x3)(torch.zeros(2, 3, hw, hw, device=DEV))
    flat = y.reshape(-1, 96)
    assert torch.equal(S.bits(flat), S.bits(flat[:1].expand_as(flat)))
    q = {k: v.double() for k, v in p.items()}
    R, xhat, kappa, _ = RW.ln_f64(q["bias"][None], q["g"], q["b"], S.EPS)
    err = (y.double().cpu().reshape(-1, 96)[:1] - R).abs()
    tol = RW.f32_term(xhat, kappa, q["g"], q["b"]) + 2 * S.U * R.abs() if x3 else S.stem_bf16_tol(R)
    assert torch.allclose(R, F.layer_norm(q["bias"][None], (96,), q["g"], q["b"], S.EPS), rtol=0, atol=1e-12)
    assert bool((err <= tol).all()), (err / tol).max().item()


# ------------------------------------------------------------------------------------------------ C: the rules
@pytest.mark.parametrize("fam,T", S.MLP_CASES)
@pytest.mark.parametrize("C", S.MLP_C)
def test_rules_x3_swin_mlp(C, fam, T):
    k = S.mlp_case(fam, T, C)
    x = k["x"].to(DEV)
    y = _mlp_fn(C)(x)
    if C == 96:     # the 8-wave and the 4-wave workgroups: the same products in the same order
        y0, y1 = _mlp_fn(C, 0)(x), _mlp_fn(C, 1)(x)
        torch.cuda.synchronize()
        assert torch.equal(y0, y1) and torch.equal(y, y1)
    _hold(f"x3_swin_mlp C={C}", y, k, f"T={T} {fam}")


@pytest.mark.parametrize("c,n,mode,fam,T", S.ROW_CASES)
def test_rules_x3_rowlin(c, n, mode, fam, T):
    k = S.row_case(c, n, mode, fam, T)
    y = _row_run(k, c, n, mode)
    assert y.shape == (T, n)
    _hold("x3_rowlin", y, k, f"{c}x{n} {mode} T={T} {fam}")


@pytest.mark.parametrize("fam,B,hw", S.STEM_CASES)
def test_rules_stem(fam, B, hw):
    k = S.stem_case(fam, B, hw)
    img = k["img"].to(DEV)
    y = _stem_fn(k["p"], True)(img)
    assert y.shape == (B, hw // 4, hw // 4, 96)
    _hold("x3_patch_embed_ln", y, k, f"B={B} hw={hw} {fam}")
    _hold_bf16(_stem_fn(k["p"], False)(img), k["Rb"], f"B={B} hw={hw} {fam}")


# ------------------------------------------------------------------------------------------------ D: refusals
def _st():
    return _lib.stream_ptr(torch.device(DEV))


def _untouched(buf):
    torch.cuda.synchronize()
    return bool((buf == POISON).all())


@pytest.mark.parametrize("entry", ["mmr_x3_patch_embed_ln", "mmr_patch_embed_ln_bf16"])
def test_refusals_stem(entry):
    L, P = _lib.lib(), _lib.ptr
    d = _dev(S.stem_params())
    pack = ops.x3_patch_embed_pack(d["w"])
    assert ops.x3_patch_embed_pack(torch.zeros(96, 3, 2, 2, device=DEV)) is None
    call = getattr(L, entry)
    y = torch.full((2 * 24 * 24 * 96,), POISON, device=DEV)
    for hw in (28, 30):     # 49 tokens per image: no multiple of 32; 30: no multiple of 4
        img = torch.ones(2, 3, hw, hw, device=DEV)
        assert call(P(img), 2, hw, P(pack), P(d["bias"]), P(d["g"]), P(d["b"]), S.EPS, P(y), _st()) != 0
        assert L.mmr_last_error() and _untouched(y)
    img = torch.ones(2, 3, 32, 32, device=DEV)
    assert call(P(img), 0, 32, P(pack), P(d["bias"]), P(d["g"]), P(d["b"]), S.EPS, P(y), _st()) == 0
    assert _untouched(y)
    assert call(P(img), -1, 32, P(pack), P(d["bias"]), P(d["g"]), P(d["b"]), S.EPS, P(y), _st()) != 0
    assert _untouched(y)


def test_refusals_x3_rowlin():
    L, P = _lib.lib(), _lib.ptr
    T = 40
    for n, c in ((48, 96), (4128, 96), (64, 96), (96, 128), (48, 192), (4128, 192)):
        assert ops.x3_rowlin_pack(torch.zeros(n, c, device=DEV)) is None, (n, c)
    assert L.mmr_x3_rowlin_pack_elems(48, 96) == 0 and L.mmr_x3_rowlin_pack_elems(4128, 192) == 0
    assert L.mmr_x3_rowlin_pack_elems(96, 128) == 0
    d = _dev(S.row_params(96, 96))
    pack = ops.x3_rowlin_pack(d["w"])
    big = torch.zeros(64 * 128 * 192 + 4128, dtype=torch.bfloat16, device=DEV)     # a pack image large enough for all
    bias = torch.zeros(4128, device=DEV)
    x = S.rows("gauss", T, 192, 1).to(DEV)
    y = torch.full((T * 4128,), POISON, device=DEV)

    def call(xp, n, c, yp=None, res=None, tokens=T, pk=big, xs=None):
        return L.mmr_x3_rowlin(xp, P(xs), P(d["g"]) if c == 96 else P(x), P(d["b"]) if c == 96 else P(x), P(pk),
                               P(bias), P(res), P(y) if yp is None else yp, tokens, n, c, S.EPS, _st())

    for n, c in ((48, 96), (4128, 96), (64, 96), (96, 128), (48, 192), (4128, 192)):
        assert call(P(x), n, c) != 0, (n, c)
        assert L.mmr_last_error() and _untouched(y)
    # y aliasing x, y aliasing the residual (n = c = 96: same row shape)
    xa = torch.full((T * 96,), POISON, device=DEV)
    assert call(P(xa), 96, 96, yp=P(xa), pk=pack) != 0 and _untouched(xa)
    assert call(P(x), 96, 96, yp=P(xa), res=xa, pk=pack) != 0 and _untouched(xa)
    # a row view that is not 16-B aligned: f32 rows, split rows, the residual
    buf = torch.zeros(T * 4128 + 4, device=DEV)
    assert call(P(buf[1:]), 96, 96, pk=pack) != 0 and _untouched(y)
    xs = torch.zeros(T * 2 * 128 + 8, dtype=torch.bfloat16, device=DEV)
    assert call(_lib.ptr(None), 96, 96, pk=pack, xs=xs[2:]) != 0 and _untouched(y)
    assert call(P(x), 96, 96, res=buf[1:], pk=pack) != 0 and _untouched(y)
    assert call(P(x), 96, 96, yp=P(y[1:]), pk=pack) != 0 and _untouched(y)
    # both or neither of x / xs; f32 rows without their LayerNorm
    assert call(P(x), 96, 96, pk=pack, xs=xs) != 0 and call(_lib.ptr(None), 96, 96, pk=pack) != 0 and _untouched(y)
    assert L.mmr_x3_rowlin(P(x), None, None, None, P(pack), P(bias), None, P(y), T, 96, 96, S.EPS, _st()) != 0
    assert _untouched(y)
    # tokens = 0: OK, nothing written; tokens < 0 refused
    assert call(P(x), 96, 96, tokens=0, pk=pack) == 0 and _untouched(y)
    assert call(P(x), 96, 96, tokens=-1, pk=pack) != 0 and _untouched(y)


def test_refusals_x3_swin_mlp():
    L, P = _lib.lib(), _lib.ptr
    T = 40
    assert ops.x3_swin_mlp_pack(torch.zeros(512, 128, device=DEV), torch.zeros(128, 512, device=DEV)) is None
    assert L.mmr_x3_swin_mlp_pack_elems(128) == 0
    d = _dev(S.mlp_params(96))
    pack = ops.x3_swin_mlp_pack(d["w1"], d["w2"])
    x = S.rows("gauss", T, 128, 1).to(DEV)
    y = torch.full((T * 128,), POISON, device=DEV)
    b1 = torch.zeros(512, device=DEV)

    def call(xp, c, yp, tokens=T):
        return L.mmr_x3_swin_mlp(xp, P(d["g"]), P(d["b"]), P(pack), P(b1), P(d["b2"]), yp, tokens, c, S.EPS, _st())

    assert call(P(x), 128, P(y)) != 0 and L.mmr_last_error() and _untouched(y)
    assert call(P(y), 96, P(y)) != 0 and _untouched(y)                    # in place
    assert call(P(x[0, 1:]), 96, P(y)) != 0 and _untouched(y)             # x not 16-B aligned
    assert call(P(x), 96, P(y[1:])) != 0 and _untouched(y)
    assert call(P(x), 96, P(y), tokens=0) == 0 and _untouched(y)
    assert call(P(x), 96, P(y), tokens=-1) != 0 and _untouched(y)


def test_zz_report():
    """Worst measured ratios per kernel (max|e|, rule 2, rule 3, rule 4; the bf16 stem: share of its tolerance) and
    part A's tile and round counts, for the record."""
    print(json.dumps({"worst": {k: [round(v, 4) for v in w] for k, w in WORST.items()}, "walks": WALKS}))
