"""GPU: the attention explanations (csrc/explain.hip), the map alignment (csrc/map_align.hip) and the model layer
over them (explain_attention, predict(explain="attention"), evaluate_explanations, attention_layers).

Bars (explain_ref.py derives them): raw vectors 2 eps relative to the f64 restatement, normalised vectors
(4 c + 4) eps, heat-map pixels the vector bound + (2 G + 1) 2^-22; chosen offsets, doubled ranks, thresholds,
inter / union and the rank sums equal; pearson HW 2^-50, spearman 2^-50 (exactly 1 for a self-pair), IoU equal."""
import json
import math
import os

import numpy as np
import pytest
import torch

import explain_ref as er
from attn_maps_ref import towers_mini
from mmr_amd import _lib, metrics, ops, synthetic
from mmr_amd.model import Backbones, MultiModalRetrievalModel
from mmr_amd.retrieval import DLSRetrievalEngine, MI355XRetrievalEngine
from mmr_amd.towers import BERT_BASE, SWIN_T

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.5


def stochastic(g, b, rows, cols, sharp=3.0, row_scale=False):
    """row-stochastic f32 maps (softmax of sharp logits); row_scale: rows scaled by distinct factors in [0.5, 1.5]
    (a row-stochastic map's row sums are all 1: its row-window search would be decided by rounding noise)"""
    m = torch.softmax(torch.randn(b, rows, cols, generator=g, dtype=torch.float64) * sharp, -1)
    if row_scale:
        m = m * (0.5 + torch.rand(b, rows, 1, generator=g, dtype=torch.float64))
    return m.float()


def below_ratio_comb(b, lc=30):
    """comb whose every window of 4 columns sums to 1 x (row factor) while the total is 108 x: column pairs
    alternate (+50.5, +50.5), (-50, -50) — max window / total = 1 / 108 < 0.06.  Needs negative entries: with
    non-negative ones 8 windows cover all 30 columns, so the best holds >= 1 / 8 of the mass."""
    pat = torch.tensor([50.5 if (j // 2) % 2 == 0 else -50.0 for j in range(lc)])
    rows = 1.0 + torch.arange(lc, dtype=torch.float32) / 64.0
    return (rows[:, None] * pat[None, :]).expand(b, lc, lc).contiguous()


# name -> (B, Np, Lt, Lc, T, image_size)
EX_CASES = {
    "mini":      (2, 49, 51, 51, 51, (28, 28)),    # Lc > Np: 3 windows; Lc == T: column mean
    "search":    (3, 4, 5, 30, 5, (8, 8)),         # both window searches
    "lt1":       (2, 9, 1, 11, 1, (30, 20)),       # Lt = 1 (default text token); windows of one row
    "short":     (2, 9, 128, 9, 128, (28, 28)),    # Lc == Np; Lc < T: normalised row means, token trim to 9
    "wide":      (4, 49, 128, 51, 128, (8, 8)),    # the model's shape with text
    "full":      (1, 49, 128, 51, 128, (224, 224)),
    "odd":       (1, 9, 5, 9, 9, (5, 3)),          # H W = 15: not a multiple of 4 (scalar stores)
}


def make_case(name):
    B, Np, Lt, Lc, T, size = EX_CASES[name]
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    return {"txt2img": stochastic(g, B, Lt, Np), "img2txt": stochastic(g, B, Np, Lt),
            "comb": stochastic(g, B, Lc, Lc, row_scale=True), "T": T, "size": size}


def check_explain(r, case, use=("txt2img", "img2txt", "comb"), token_cond=64.0):
    """every output of ops.explain_attention against the restatement, sample by sample (token_cond: the bound on the
    token vector's max / (max - min); the mini model's t_img is nearly uniform over its 128 tokens: 73.4)"""
    maps = {k: (case[k] if k in use else None) for k in ("txt2img", "img2txt", "comb")}
    torch.cuda.synchronize()
    assert int(r["nonfinite"].item()) == 0
    B = next(v for v in maps.values() if v is not None).shape[0]
    worst = {}
    for b in range(B):
        ref = er.explain_sample(*(None if maps[k] is None else maps[k][b].numpy() for k in maps), case["T"])
        # the fixture conditions: the searches are decided well above rounding, the normalisations well conditioned
        # (a below-ratio sample is all zeros whichever window wins)
        assert min(math.inf if ref["below_p"] else ref["gap_p"], ref["gap_t"]) >= 1e-3, (b, ref["gap_p"], ref["gap_t"])
        assert r["offsets"][b].tolist() == [ref["off_p"], ref["off_t"]]
        for k in ("p_txt", "t_img", "p_comb"):
            if ref[k] is None:
                assert r[k] is None, k
                continue
            got = r[k][b].double().cpu().numpy()
            assert got.shape == ref[k].shape, k
            err = np.abs(got - ref[k]) - er.tol_raw(ref[k])
            worst[k] = max(worst.get(k, -1.0), float(err.max()))
        if ref["t_comb"] is not None:
            got = r["t_comb"][b].double().cpu().numpy()
            assert got.shape == ref["t_comb"].shape
            tol = er.tol_raw(ref["t_comb"]) if ref["t_comb_src"] is None else er.tol_norm(ref["t_comb_src"])
            if ref["t_comb_src"] is not None and np.ptp(ref["t_comb_src"]) < 1e-8:  # the uniform vector, exactly
                assert np.array_equal(got, np.full(len(got), np.float32(1.0) / np.float32(len(got)), np.float64))
            worst["t_comb"] = max(worst.get("t_comb", -1.0), float((np.abs(got - ref["t_comb"]) - tol).max()))
            assert abs(float(r["comb_absmax"][b, 1]) - np.abs(got).max()) == 0.0
        else:
            assert r["t_comb"] is None
        vec_tol = {}
        for k in ("final_patch", "final_token"):
            if ref[k] is None:
                assert r[k] is None, k
                continue
            got = r[k][b].double().cpu().numpy()
            assert got.shape == ref[k].shape, k
            if len(ref[k]) == 1:  # one element: (x - x) / 1e-8, exactly 0
                assert got.tolist() == [0.0], k
                continue
            lim = 64.0 if k == "final_patch" else token_cond
            assert er.cond(ref[k + "_src"]) <= lim, (k, er.cond(ref[k + "_src"]))
            vec_tol[k] = er.tol_norm(ref[k + "_src"])
            worst[k] = max(worst.get(k, -1.0), float(np.abs(got - ref[k]).max() - vec_tol[k]))
        if case["size"] is None:
            assert r["map_txt2img"] is None and r["map_comb"] is None and r["map_final"] is None
            continue
        G = math.isqrt(len(ref["p_txt"] if ref["p_txt"] is not None else ref["p_comb"]))
        for k, src, renorm in (("map_txt2img", "p_txt", False), ("map_comb", "p_comb", False),
                               ("map_final", "final_patch", True)):
            if ref[src] is None:
                assert r[k] is None, k
                continue
            if src == "p_comb" and not np.any(ref[src]):
                assert torch.equal(r[k][b], torch.zeros_like(r[k][b]))  # zeros normalise to zeros
                continue
            want = er.heat_map(ref[src], case["size"])
            vt = vec_tol["final_patch"] if renorm else er.tol_norm(ref[src])
            got = r[k][b].double().cpu().numpy()
            assert got.shape == want.shape, k
            worst[k] = max(worst.get(k, -1.0), float(np.abs(got - want).max() - er.tol_pixel(vt, G, renorm)))
    print(json.dumps({"max(err - tol)": worst}))
    assert all(v <= 0.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", list(EX_CASES))
def test_explain_kernel_vs_restatement(name):
    case = make_case(name)
    args = [case[k].to(DEV) for k in ("txt2img", "img2txt", "comb")]
    r = ops.explain_attention(*args, text_len=case["T"], image_size=case["size"])
    r2 = ops.explain_attention(*args, text_len=case["T"], image_size=case["size"])
    check_explain(r, case)
    for k, v in r.items():  # fixed-order sums: two runs, the same bytes
        assert v is None or torch.equal(v, r2[k]), k


def test_explain_kernel_vs_reference_golden():
    """the reference's own recorded dictionaries (explain_mini.npz: attn_mini's last-layer maps with and without
    text, the synthetic Np x Lc x T grid), at the bound for f32-recorded values; (224, 224) for the two text samples"""
    g = np.load(os.path.join(GOLDEN, "explain_mini.npz"), allow_pickle=False)
    a = np.load(os.path.join(GOLDEN, "attn_mini.npz"), allow_pickle=False)
    worst = {}
    for name in er.record_names(g):
        t2i, i2t, comb, T, size = er.record_inputs(g, a, name)
        r = ops.explain_attention(*(torch.from_numpy(x)[None].to(DEV) for x in (t2i, i2t, comb)), text_len=T,
                                  image_size=size)
        vec = er.sample_with_lc(t2i, i2t, comb, T)
        assert r["offsets"][0, 0].item() == vec["off_p"]
        if not name.startswith("notext"):  # a row-stochastic comb's rows all tie
            assert r["offsets"][0, 1].item() == vec["off_t"]
        got = {"txt2img": r["map_txt2img"], "img2txt": r["t_img"], "comb_img": r["map_comb"], "comb_txt": r["t_comb"],
               "final_patch_map": r["map_final"], "final_token_map": r["final_token"]}
        w = er.check_against_record(g, name, vec, size, {k: v[0].cpu().numpy() for k, v in got.items()})
        worst = {k: max(v, worst.get(k, -1.0)) for k, v in w.items()}
        if name.startswith("text"):
            big = ops.explain_attention(*(torch.from_numpy(x)[None].to(DEV) for x in (t2i, i2t, comb)), text_len=T,
                                        image_size=(224, 224))["map_final"][0].double().cpu().numpy()
            tol = er.tol_pixel(er.tol_norm(vec["final_patch_src"], 128), 7, True)
            assert np.abs(big - g[f"{name}:final224"]).max() <= tol
    print(json.dumps({"max(err - tol)": worst}))


def test_map_alignment_vs_reference_golden():
    """compare_maps' recorded values (scipy / numpy on the host): pearson HW 2^-50 of the f64-copy record and HW eps
    of the f32 as-run record, spearman 2^-50 of both, IoU equal"""
    g = np.load(os.path.join(GOLDEN, "explain_mini.npz"), allow_pickle=False)
    maps, pairs = g["al_maps"], g["al_pairs"]
    hw = maps.shape[1]
    r = ops.map_alignment(torch.from_numpy(maps).to(DEV), pairs[:, 0], pairs[:, 1])
    pe, sp = r["pearson"].cpu().numpy(), r["spearman"].cpu().numpy()
    iu = r["inter_union"].cpu().numpy().astype(np.float64)
    assert int(r["nonfinite"].item()) == 0 and not r["skipped"].any()
    for p in range(len(pairs)):
        for j in range(2):
            f32, f64 = g["al_f32"][p, j], g["al_f64"][p, j]
            assert abs(pe[p] - f64[0]) <= hw * 2.0 ** -50 and abs(pe[p] - f32[0]) <= hw * er.EPS, (p, pe[p], f64[0])
            assert abs(sp[p] - f64[1]) <= 2.0 ** -50 and abs(sp[p] - f32[1]) <= 2.0 ** -50, (p, sp[p], f64[1])
            assert iu[p, j, 0] / (iu[p, j, 1] + 1e-8) == f64[2] == f32[2], (p, j)
        if pairs[p, 0] == pairs[p, 1] and pairs[p, 0] != 4:
            assert sp[p] == 1.0
    for j, frac in enumerate((0.05, 0.20)):  # the public wrapper, one pair and a stack
        one = metrics.compare_maps(torch.from_numpy(maps[0]).to(DEV).view(28, 28),
                                   torch.from_numpy(maps[1]).to(DEV).view(28, 28), topk_frac=frac)
        assert list(one) == ["pearson", "spearman", er.iou_key(frac)]
        assert one["pearson"] == pe[0] and one["spearman"] == sp[0] and one[er.iou_key(frac)] == g["al_f64"][0, j, 2]


def test_explain_below_ratio_zeroes_comb_img():
    case = make_case("search")
    case["comb"] = below_ratio_comb(3)
    r = ops.explain_attention(*(case[k].to(DEV) for k in ("txt2img", "img2txt", "comb")), text_len=5,
                              image_size=case["size"])
    torch.cuda.synchronize()
    ref = er.explain_sample(case["txt2img"][0].numpy(), case["img2txt"][0].numpy(), case["comb"][0].numpy(), 5)
    assert ref["below_p"] and not np.any(ref["p_comb"])
    assert torch.equal(r["p_comb"], torch.zeros_like(r["p_comb"]))
    assert torch.equal(r["comb_absmax"][:, 0], torch.zeros(3, device=DEV))  # <= 1e-8: the host drops comb_img
    assert torch.equal(r["map_comb"], torch.zeros_like(r["map_comb"]))
    check_explain(r, case)  # final_patch = minmax(0.6 p_txt + 0)


@pytest.mark.parametrize("use", [("txt2img",), ("img2txt",), ("img2txt", "comb"), ("txt2img", "comb"),
                                 ("txt2img", "img2txt")])
def test_explain_null_maps(use):
    case = make_case("search")
    if "txt2img" not in use and "comb" not in use:
        case["size"] = None
    r = ops.explain_attention(*(case[k].to(DEV) if k in use else None for k in ("txt2img", "img2txt", "comb")),
                              text_len=case["T"], image_size=case["size"])
    check_explain(r, case, use)


def test_explain_strided_inputs_equal_contiguous():
    case = make_case("mini")
    dense = [case[k].to(DEV) for k in ("txt2img", "img2txt", "comb")]
    want = ops.explain_attention(*dense, text_len=case["T"], image_size=case["size"])
    strided = []
    for t in dense:
        B, R, C = t.shape
        buf = torch.full((B + 1, R + 3, C + 5), float("nan"), device=DEV)  # NaN around the views
        buf[1:, 2:2 + R, 4:4 + C] = t
        strided.append(buf[1:, 2:2 + R, 4:4 + C])
    got = ops.explain_attention(*strided, text_len=case["T"], image_size=case["size"])
    torch.cuda.synchronize()
    for k, v in want.items():
        assert v is None or torch.equal(v, got[k]), k


def _raw_explain(t2i, i2t, comb, lt, npatch, lcr, lcc, T, H, W, outs, work):
    """mmr_explain_attention itself on dense maps; outs: the 12 output tensors (or None) in the ABI's order"""
    def p(t):
        return _lib.ptr(t)
    L = _lib.lib()
    B = next(t for t in (t2i, i2t, comb) if t is not None).shape[0]
    st = L.mmr_explain_attention(p(t2i), lt * npatch, npatch, p(i2t), npatch * lt, lt, p(comb), lcr * lcc, lcc, B, lt,
                                 npatch, lcr, lcc, T, H, W, *(p(o) for o in outs), p(work),
                                 _lib.stream_ptr(torch.device(DEV)))
    return st, L.mmr_last_error().decode()


def test_explain_guard_padded_outputs_untouched():
    B, Np, Lt, Lc, T, (H, W) = 2, 9, 5, 11, 5, (5, 3)
    g = torch.Generator().manual_seed(5)
    t2i, i2t = stochastic(g, B, Lt, Np).to(DEV), stochastic(g, B, Np, Lt).to(DEV)
    comb = stochastic(g, B, Lc, Lc, row_scale=True).to(DEV)
    sizes = [B * Np, B * Lt, B * Np, B * T, B * Np, B * T, B * H * W, B * H * W, B * H * W]
    pad = 64
    bufs = [torch.full((n + 2 * pad,), SENTINEL, device=DEV) for n in sizes]
    outs = [b[pad:] for b in bufs]  # 256-B offset: the heat maps stay 16-B aligned
    offsets = torch.full((B * 2 + 2 * pad,), -99, dtype=torch.int32, device=DEV)
    absmax = torch.full((B * 2 + 2 * pad,), SENTINEL, device=DEV)
    nonfinite = torch.full((3,), -99, dtype=torch.int64, device=DEV)
    work = torch.empty(int(_lib.lib().mmr_explain_attention_work_bytes(B, Lt, Np, Lc)), dtype=torch.uint8, device=DEV)
    st, msg = _raw_explain(t2i, i2t, comb, Lt, Np, Lc, Lc, T, H, W,
                           outs + [offsets[pad:], absmax[pad:], nonfinite[1:]], work)
    torch.cuda.synchronize()
    assert st == 0, msg
    for b, n in zip(bufs, sizes):
        assert bool((b[:pad] == SENTINEL).all()) and bool((b[pad + n:] == SENTINEL).all())
        assert not bool((b[pad:pad + n] == SENTINEL).any())
    assert bool((offsets[:pad] == -99).all()) and bool((offsets[pad + 2 * B:] == -99).all())
    assert bool((absmax[:pad] == SENTINEL).all()) and bool((absmax[pad + 2 * B:] == SENTINEL).all())
    assert nonfinite.tolist() == [-99, 0, -99]
    want = ops.explain_attention(t2i, i2t, comb, text_len=T, image_size=(H, W))
    for o, k in zip(outs, ("p_txt", "t_img", "p_comb", "t_comb", "final_patch", "final_token", "map_txt2img",
                           "map_comb", "map_final")):
        assert torch.equal(o[:want[k].numel()], want[k].reshape(-1)), k


@pytest.mark.parametrize("what,kw,match", [
    ("np not square", dict(npatch=8), "perfect square"),
    ("np too large", dict(npatch=1089), "Np = 1089"),
    ("lt too large", dict(lt=4097), "Lt = 4097"),
    ("lc too large", dict(lcr=4097, lcc=4097), "Lc = 4097"),
    ("comb not square", dict(lcr=11, lcc=12), "not square"),
    ("no pixels", dict(H=0, W=8), "pixels"),
    ("too many pixels", dict(H=257, W=256), "pixels"),
])
def test_explain_refusals(what, kw, match):
    """every refusal is MMR_ERR_INVALID with a message, before any launch (the buffers are one float each)"""
    a = dict(lt=5, npatch=9, lcr=11, lcc=11, T=5, H=8, W=8)
    a.update(kw)
    one = [torch.zeros(4, device=DEV) for _ in range(12)]
    i32, i64 = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    outs = one[3:12] + [i32, one[0], i64]
    t = torch.zeros(1, 1, 4, device=DEV)
    st, msg = _raw_explain(t, t, t, a["lt"], a["npatch"], a["lcr"], a["lcc"], a["T"], a["H"], a["W"], outs, one[1])
    assert st == 1 and match in msg, (what, st, msg)
    assert all(bool((o == 0).all()) for o in outs)


def test_explain_nonfinite_counted():
    case = make_case("search")
    case["txt2img"][1, 2, 3] = float("nan")
    case["comb"][0, 0, 0] = float("inf")
    r = ops.explain_attention(*(case[k].to(DEV) for k in ("txt2img", "img2txt", "comb")), text_len=5)
    assert int(r["nonfinite"].item()) >= 2
    assert r["map_final"] is None and bool((r["offsets"] >= 0).all()) and bool((r["offsets"] <= 26).all())


# ------------------------------------------------------------------------------------------------ alignment
def align_maps(hw, seed):
    """8 maps: gaussian (negative values), its negation, heavy ties, a constant, +-0 with plateaus, gaussian,
    two-valued, a ramp"""
    g = np.random.default_rng(seed)
    m = np.empty((8, hw), np.float32)
    m[0] = g.standard_normal(hw)
    m[1] = -m[0]
    m[2] = g.integers(0, 4, hw)
    m[3] = 0.25
    m[4] = np.where(g.random(hw) < 0.5, 0.0, -0.0)
    m[4, ::5] = 1.5
    m[4, 1::7] = -2.0
    m[5] = g.standard_normal(hw) * 1e-3 + 0.5
    m[6] = (g.random(hw) < 0.1)
    m[7] = np.arange(hw, dtype=np.float32) / hw
    return m


PAIRS = ([0, 0, 0, 2, 3, 4, 4, 5, 6, 7, 1, -1, 8, 2, 5, 3], [0, 1, 5, 2, 0, 4, 2, 7, 2, 0, 1, 0, 3, 6, 5, 3])


@pytest.mark.parametrize("hw,fracs", [(16, (0.05, 0.20)), (1024, (0.05, 0.20, 0.29, 1.0)), (50176, (0.05, 0.20))])
def test_map_alignment_vs_restatement(hw, fracs):
    m = align_maps(hw, hw)
    pa, pb = (np.array(p, np.int64) for p in PAIRS)
    if hw == 50176:  # once at the evaluation's size: fewer pairs, the same kinds
        pa, pb = pa[[0, 1, 3, 4, 6, 11]], pb[[0, 1, 3, 4, 6, 11]]
    r = ops.map_alignment(torch.from_numpy(m).to(DEV), pa, pb, fracs=fracs)
    r2 = ops.map_alignment(torch.from_numpy(m).to(DEV).view(8, -1, 4), torch.from_numpy(pa), torch.from_numpy(pb).to(DEV),
                           fracs=fracs)
    torch.cuda.synchronize()
    ks = [er.topk_count(hw, f) for f in fracs]
    assert r["k"] == ks and int(r["nonfinite"].item()) == 0
    for k, v in r.items():
        assert k == "k" or torch.equal(v, r2[k]), k
    for i in range(8):
        s = er.map_stats(m[i], ks)
        assert np.array_equal(r["ranks2"][i].cpu().numpy(), s["ranks2"]), i
        assert np.array_equal(r["thresholds"][i].cpu().numpy(), s["thresholds"]), i
        assert bool(r["constant"][i]) == s["constant"], i
        assert abs(float(r["mean"][i]) - s["mean"]) <= hw * 2.0 ** -50 * max(1.0, abs(s["mean"])), i
    got = {k: r[k].cpu().numpy() for k in ("pearson", "spearman", "rank_sums", "inter_union", "skipped")}
    for p, (a, b) in enumerate(zip(pa, pb)):
        if not (0 <= a < 8 and 0 <= b < 8):
            assert got["skipped"][p] == 1 and got["pearson"][p] == 0 and not got["inter_union"][p].any(), p
            continue
        ref = er.compare_pair(m[a], m[b], ks)
        assert got["skipped"][p] == 0
        assert tuple(got["rank_sums"][p]) == ref["rank_sums"], p
        assert [tuple(x) for x in got["inter_union"][p]] == ref["inter_union"], p
        assert abs(got["pearson"][p] - ref["pearson"]) <= hw * 2.0 ** -50, (p, got["pearson"][p], ref["pearson"])
        assert abs(got["spearman"][p] - ref["spearman"]) <= 2.0 ** -50, (p, got["spearman"][p], ref["spearman"])
        if a == b and not ref["rank_sums"][1] == 0:
            assert got["spearman"][p] == 1.0 and abs(got["pearson"][p] - 1.0) <= hw * 2.0 ** -50
        if a in (3,) or b in (3,):
            assert got["pearson"][p] == 0.0 and got["spearman"][p] == 0.0  # a constant map
        iou = got["inter_union"][p][:, 0] / (got["inter_union"][p][:, 1] + 1e-8)
        assert iou.tolist() == ref["iou"]
    assert got["pearson"][1] < -0.999999 and got["spearman"][1] == -1.0  # a map against its negation


def test_map_alignment_nan_count_strided_and_refusals():
    m = torch.from_numpy(align_maps(64, 3))
    wide = torch.full((8, 80), float("nan"))
    wide[:, :64] = m
    r = ops.map_alignment(wide.to(DEV)[:, :64], [0, 2], [1, 4])          # row stride 80
    want = ops.map_alignment(m.to(DEV), [0, 2], [1, 4])
    for k in ("pearson", "spearman", "rank_sums", "inter_union", "ranks2"):
        assert torch.equal(r[k], want[k]), k
    assert int(r["nonfinite"].item()) == 0
    m[1, 5], m[6, 0] = float("nan"), float("-inf")
    assert int(ops.map_alignment(m.to(DEV), [0], [1])["nonfinite"].item()) == 2
    with pytest.raises(ValueError, match="NaN"):
        metrics.compare_maps(m[1].to(DEV).view(8, 8), m[0].to(DEV).view(8, 8))
    L = _lib.lib()
    assert L.mmr_map_alignment_work_bytes(65537, 16) == 0 and L.mmr_map_alignment_work_bytes(8, 65537) == 0
    assert L.mmr_map_alignment_work_bytes(65536, 32768) == 0 and L.mmr_map_alignment_work_bytes(8, 65536) > 0
    z = torch.zeros(64, device=DEV)
    p = _lib.ptr(z)
    for n, hw, k0, match in ((65537, 16, 1, "N = 65537"), (8, 65537, 1, "HW = 65537"), (65536, 32768, 1, "2^31"),
                             (8, 16, 17, "k[0] = 17"), (8, 16, 0, "k[0] = 0")):
        st = L.mmr_map_alignment(p, hw, n, hw, p, p, 1, 1, k0, 1, 1, 1, p, p, p, p, p, p, p, p, p, p, p, p,
                                 _lib.stream_ptr(torch.device(DEV)))
        assert st == 1 and match in L.mmr_last_error().decode(), (n, hw, k0, L.mmr_last_error())
    assert bool((z == 0).all())


def test_compare_maps_single_and_stack():
    m = align_maps(28 * 28, 9).reshape(8, 28, 28)
    d = torch.from_numpy(m).to(DEV)
    one = metrics.compare_maps(d[0], d[5], topk_frac=0.29)
    assert list(one) == ["pearson", "spearman", "iou_top28pct"]  # int(0.29 * 100) == 28, as the reference names it
    assert all(isinstance(v, float) for v in one.values())
    ref = er.compare_pair(m[0], m[5], [er.topk_count(784, 0.29)])
    assert abs(one["pearson"] - ref["pearson"]) <= 784 * 2.0 ** -50 and abs(one["spearman"] - ref["spearman"]) <= 2.0 ** -50
    assert one["iou_top28pct"] == ref["iou"][0]
    st = metrics.compare_maps(d[[0, 2, 3]], d[[5, 4, 0]])
    assert list(st) == ["pearson", "spearman", "iou_top5pct"] and all(v.shape == (3,) for v in st.values())
    for j, (a, b) in enumerate(((0, 5), (2, 4), (3, 0))):
        ref = er.compare_pair(m[a], m[b], [er.topk_count(784, 0.05)])
        assert abs(st["pearson"][j] - ref["pearson"]) <= 784 * 2.0 ** -50
        assert abs(st["spearman"][j] - ref["spearman"]) <= 2.0 ** -50 and st["iou_top5pct"][j] == ref["iou"][0]


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module", params=["x3", "bf16"])
def mini(request):
    """the mini model in both tower modes: the x3 and the bf16 path of FusionStack.forward"""
    f, w = towers_mini()
    cfg = json.loads(bytes(f["cfg"]).decode())
    scfg = dict(SWIN_T, embed_dim=cfg["swin"]["embed_dim"], depths=cfg["swin"]["depths"],
                num_heads=cfg["swin"]["num_heads"])
    bb = Backbones(swin_state=w["swin"], bert_state=w["bert"], swin_cfg=scfg, bert_cfg=dict(BERT_BASE, **cfg["bert"]),
                   device=DEV, tower_dtype=request.param)
    image = torch.from_numpy(synthetic.image_from_u8(f["img_u8"])).to(DEV)
    ids = torch.from_numpy(f["input_ids"]).to(DEV)
    mask = torch.from_numpy(f["attention_mask"]).to(DEV)
    kw = dict(joint_dim=cfg["joint_dim"], num_heads=cfg["num_heads"], backbones=bb, head_state=w["head"], device=DEV,
              use_shared_ffn=False)
    return MultiModalRetrievalModel(model_type="multimodal", **kw), kw, (image, ids, mask)


@pytest.mark.parametrize("text", [True, False])
def test_model_explain_attention(mini, text):
    """explain_attention = ops.explain_attention's restatement on the model's own last-layer maps; the forward it
    runs leaves joint_emb's bits alone; attention_layers=[last] returns the all-layers call's bytes."""
    m, _, (image, ids, mask) = mini
    args = (image, ids, mask) if text else (image, None, None)
    o = m(*args, return_attention=True)
    nl = len(m.fusion.layers)
    e = m.explain_attention(*args, image_size=(28, 28))
    torch.cuda.synchronize()
    assert torch.equal(e["joint_emb"], o["joint_emb"])
    last = {k: o["attn"][f"layer_{nl - 1}_{k}"] for k in ("txt2img", "img2txt", "comb")}
    Lt = 128 if text else 1
    assert last["txt2img"].shape == (2, Lt, 49)
    case = dict(last, T=Lt, size=(28, 28))
    want = ops.explain_attention(*(last[k].to(DEV) for k in ("txt2img", "img2txt", "comb")), text_len=Lt,
                                 image_size=(28, 28))
    for mine, theirs in (("txt2img", "map_txt2img"), ("img2txt", "t_img"), ("comb_img", "map_comb"),
                         ("comb_txt", "t_comb"), ("final_patch_map", "map_final"), ("final_token_map", "final_token")):
        assert torch.equal(e[mine], want[theirs]), mine
    assert e["comb_img_valid"].tolist() == [True, True] and e["txt2img"].shape == (2, 28, 28)
    assert e["img2txt"].shape == (2, Lt) and e["comb_txt"].shape == (2, min(Lt, 51))
    if text:  # row sums of a stochastic comb are all 1: only the Lc < T branch is decided above rounding
        check_explain(want, case, token_cond=128.0)
    # attention_layers: only the asked layer's keys, the same bytes
    img_global, patches, _ = m.backbones.encode_image(image, want_patches=True)
    txt = m.backbones.encode_text(ids, mask) if text else None
    _, every = m.fusion.forward(img_global, patches, txt, return_attention=True)
    j1, only = m.fusion.forward(img_global, patches, txt, return_attention=True, attention_layers=[-1])
    assert list(only) == [f"layer_{nl - 1}_{k}" for k in ("comb", "txt2img", "img2txt")]
    for k, v in only.items():
        assert torch.equal(v, every[k]), k
    assert torch.equal(j1, o["joint_emb"])
    with pytest.raises(ValueError, match="attention_layers"):
        m.fusion.forward(img_global, patches, txt, return_attention=True, attention_layers=[nl])


def test_model_predict_explain_attention_schema(mini):
    m, kw, args = mini
    with pytest.raises(NotImplementedError, match="Grad-CAM") as ei:
        m.predict(*args, explain=True)
    assert '"attention"' in str(ei.value)
    m.set_retriever(None)
    with pytest.raises(ValueError, match="retriever"):
        m.predict(*args, explain="attention")
    G = synthetic.gauss_gallery(300, kw["joint_dim"], 17)
    eng = MI355XRetrievalEngine(embs=G, ids=[f"r{i}" for i in range(len(G))])
    m.set_retriever(eng)
    try:
        plain = m.predict(*args, K=4, retrieve=True)
        p = m.predict(*args, K=4, explain="attention")
        assert list(p) == ["probs", "preds", "topk_idx", "topk_vals", "retrieval_ids", "retrieval_dists",
                           "attention_map", "ig_maps", "gradcam_maps"]
        assert p["ig_maps"] is None and p["gradcam_maps"] is None
        for k in plain:
            assert np.array_equal(p[k], plain[k]) if isinstance(plain[k], np.ndarray) else p[k] == plain[k], k
        am = p["attention_map"]
        assert list(am) == ["txt2img", "img2txt", "comb_img", "comb_txt", "final_patch_map", "final_token_map"]
        e = m.explain_attention(*args)
        for k, shape in (("txt2img", (224, 224)), ("img2txt", (128,)), ("comb_img", (224, 224)), ("comb_txt", (51,)),
                         ("final_patch_map", (224, 224)), ("final_token_map", (51,))):
            assert isinstance(am[k], np.ndarray) and am[k].dtype == np.float32 and am[k].shape == shape, k
            assert np.array_equal(am[k], e[k][0].cpu().numpy()), k
        assert list(m.predict(*args, explain=False)) == ["probs", "preds", "topk_idx", "topk_vals"]
        mt = MultiModalRetrievalModel(model_type="text", **kw)
        mt.set_retriever(eng)
        with pytest.raises(ValueError, match="multimodal"):
            mt.predict(*args, explain="attention")
        with pytest.raises(ValueError, match="multimodal"):
            mt.explain_attention(*args)
    finally:
        m.set_retriever(None)
        eng.close()


@pytest.mark.parametrize("exclude_self", [False, True])
def test_model_evaluate_explanations(mini, exclude_self):
    """= compare_maps pair by pair on explain_attention's own maps, with the engine's own top-K"""
    m, kw, (image, ids, mask) = mini
    size = (28, 28)
    g = torch.Generator().manual_seed(3)
    images = [image, image.flip(0) * 0.5, torch.randn(image.shape, generator=g).to(DEV)]
    batches = [(im, ids, mask) for im in images]
    ex = [m.explain_attention(*b, image_size=size) for b in batches]
    maps, embs = torch.cat([e["final_patch_map"] for e in ex]), torch.cat([e["joint_emb"] for e in ex])
    n = maps.shape[0]
    eng = MI355XRetrievalEngine(embs=embs.cpu().numpy(), ids=[f"q{i}" for i in range(n)])
    m.set_retriever(eng)
    try:
        out = m.evaluate_explanations(batches, K=3, image_size=size, exclude_self=exclude_self, return_per_query=True)
        idx = eng.search(embs, K=3 + exclude_self)[0].cpu().numpy()
        nb = [next(int(j) for j in row if not (exclude_self and j == q)) for q, row in enumerate(idx)]
        assert out["n_pairs"] == n and out["query_index"].tolist() == list(range(n))
        assert out["neighbor_index"].tolist() == nb
        if not exclude_self:
            assert nb == list(range(n)) and out["spearman_mean"] == 1.0  # test -> test: each query finds itself
        for frac, name in ((0.05, "iou05"), (0.20, "iou20")):
            ref = metrics.compare_maps(maps, maps[nb], topk_frac=frac)
            assert np.array_equal(out[name], ref[metrics.iou_key(frac)])
            assert np.array_equal(out["pearson"], ref["pearson"]) and np.array_equal(out["spearman"], ref["spearman"])
            assert out[name + "_mean"] == float(ref[metrics.iou_key(frac)].mean())
        assert out["pearson_mean"] == float(out["pearson"].mean())
        assert sorted(m.evaluate_explanations(batches, K=3, image_size=size)) == [
            "iou05_mean", "iou20_mean", "n_pairs", "pearson_mean", "spearman_mean"]
        empty = m.evaluate_explanations([], K=3)
        assert empty == {"pearson_mean": 0.0, "spearman_mean": 0.0, "iou05_mean": 0.0, "iou20_mean": 0.0, "n_pairs": 0}
        with pytest.raises(ValueError, match="gallery"):
            m.evaluate_explanations(batches[:2], K=3, image_size=size)
    finally:
        m.set_retriever(None)
        eng.close()


def test_model_evaluate_explanations_dls_engine(mini):
    """the retrieve_batch branch: a DLS walk's lists (seeds drawn afresh, -1 past the candidate set) — whatever
    neighbour the walk returns first, the scores are compare_maps of that pair"""
    m, kw, (image, ids, mask) = mini
    size = (28, 28)
    batches = [(image, ids, mask), (image.flip(0) * 0.5, ids, mask), (image.flip(2), ids, mask)]
    ex = [m.explain_attention(*b, image_size=size) for b in batches]
    maps, embs = torch.cat([e["final_patch_map"] for e in ex]), torch.cat([e["joint_emb"] for e in ex])
    n = maps.shape[0]
    eng = DLSRetrievalEngine(embs=embs.cpu().numpy(), ids=[f"q{i}" for i in range(n)], link_threshold=0.5, max_links=10)
    m.set_retriever(eng)
    try:
        lists = eng.retrieve_batch(embs, K=n)[0]
        assert bool((lists == -1).any()) or lists.shape[1] == n  # 5 seeds of 6 rows: lists may end in -1
        for exclude_self in (False, True):
            out = m.evaluate_explanations(batches, K=n, image_size=size, exclude_self=exclude_self,
                                          return_per_query=True)
            q, nb = out["query_index"], out["neighbor_index"]
            assert out["n_pairs"] == len(q) >= n - 1 and ((nb >= 0) & (nb < n)).all()
            if exclude_self:
                assert (nb != q).all()
            ref = metrics.compare_maps(maps[q], maps[nb], topk_frac=0.20)
            assert np.array_equal(out["pearson"], ref["pearson"]) and np.array_equal(out["spearman"], ref["spearman"])
            assert np.array_equal(out["iou20"], ref["iou_top20pct"])
    finally:
        m.set_retriever(None)
        eng.close()


def test_model_degenerate_comb(mini, monkeypatch):
    """model level, with the last layer's comb replaced: a below-ratio comb leaves comb_img out of predict's
    attention_map (comb_img_valid False, explain.py:865); a comb_txt that is all <= 1e-7 raises, naming the sample"""
    m, kw, (image, ids, mask) = mini
    real, nl = m.fusion.forward, len(m.fusion.layers)

    def swap(comb):
        def fwd(*a, **k):
            joint, maps = real(*a, **k)
            return joint, dict(maps, **{f"layer_{nl - 1}_comb": comb.to(DEV)})
        monkeypatch.setattr(m.fusion, "forward", fwd)
    # columns 0, 1, 49, 50 hold +10, column 2 holds -19: each of the 3 windows of 49 columns sums to 1 (x the row
    # factors), the total to 21: 1 / 21 < 0.06
    pat = torch.zeros(51)
    pat[[0, 1, 49, 50]], pat[2] = 10.0, -19.0
    low = ((1.0 + torch.arange(51.0) / 64.0)[:, None] * pat[None, :]).expand(2, 51, 51).contiguous()
    swap(low)
    e = m.explain_attention(image, ids, mask, image_size=(28, 28))
    assert e["comb_img_valid"].tolist() == [False, False]
    assert torch.equal(e["comb_img"], torch.zeros_like(e["comb_img"])) and bool((e["comb_txt"] > 1e-7).any())
    eng = MI355XRetrievalEngine(embs=synthetic.gauss_gallery(50, kw["joint_dim"], 17), ids=[f"r{i}" for i in range(50)])
    m.set_retriever(eng)
    try:
        am = m.predict(image, ids, mask, K=3, explain="attention")["attention_map"]
        assert list(am) == ["txt2img", "img2txt", "comb_txt", "final_patch_map", "final_token_map"]
        assert am["final_patch_map"].shape == (224, 224)
    finally:
        m.set_retriever(None)
        eng.close()
    # no text: T = 1 < Lc = 51, so comb_txt is the chosen row's mean — of an all-zero comb, zero
    swap(torch.zeros(2, 51, 51))
    with pytest.raises(ValueError, match="comb_txt of sample 0"):
        m.explain_attention(image, None, None, image_size=(28, 28))
