"""CPU: the restatement of the attention explanations and of the map alignment (explain_ref.py) against the
reference's recorded values (tests/golden/explain_mini.npz, written by tests/golden/make_golden_explain.py), the
public signatures, the IoU key naming, the k formula and the C entry points' refusals (no GPU: every refusal comes
before the first HIP call)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import explain_ref as er
from mmr_amd import _lib, metrics, ops
from mmr_amd.fusion import FusionStack
from mmr_amd.model import MultiModalRetrievalModel

from conftest import GOLDEN

EPS = er.EPS


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(GOLDEN, "explain_mini.npz"), allow_pickle=False)
    a = np.load(os.path.join(GOLDEN, "attn_mini.npz"), allow_pickle=False)
    return g, a


def test_fixture_covers_the_cases(gold):
    g, _ = gold
    names = er.record_names(g)
    assert [n for n in names if not n.startswith("syn_")] == ["notext_0", "notext_1", "text_0", "text_1"]
    want = {f"syn_{n}_{lc}_{t}" for n in (4, 9) for lc in (n, n + 2, 30) for t in {1, 5, lc, 128}}
    assert {n for n in names if n.startswith("syn_")} == want
    assert os.path.getsize(os.path.join(GOLDEN, "explain_mini.npz")) <= 600 * 1024
    assert g["text_0:final224"].shape == (224, 224) and g["text_1:final224"].shape == (224, 224)


def test_restatement_matches_the_reference_record(gold):
    g, a = gold
    for name in er.record_names(g):
        t2i, i2t, comb, T, size = er.record_inputs(g, a, name)
        vec = er.sample_with_lc(t2i, i2t, comb, T)
        er.fixture_conditions(vec, name, row_search=not name.startswith("notext"),
                              token_cond=128.0 if name.startswith("text") else 64.0)
        er.check_against_record(g, name, vec, size)
        if name.startswith("text"):
            want = er.heat_map(vec["final_patch"], (224, 224))
            tol = er.tol_pixel(er.tol_norm(vec["final_patch_src"], 128), 7, True)
            assert np.abs(want - g[f"{name}:final224"]).max() <= tol


def test_alignment_restatement_matches_the_record(gold):
    g, _ = gold
    maps, pairs = g["al_maps"], g["al_pairs"]
    hw = maps.shape[1]
    assert any(a == b for a, b in pairs) and hw == 784
    assert np.all(maps[4] == maps[4, 0]) and np.signbit(maps[5][maps[5] == 0]).any() and (maps[5] == 0).sum() > 50
    ks = [er.topk_count(hw, f) for f in (0.05, 0.20)]
    for p, (a, b) in enumerate(pairs):
        r = er.compare_pair(maps[a], maps[b], ks)
        for j in range(2):
            f32, f64 = g["al_f32"][p, j], g["al_f64"][p, j]
            assert abs(r["pearson"] - f64[0]) <= hw * 2.0 ** -50, (p, r["pearson"], f64[0])
            assert abs(r["pearson"] - f32[0]) <= hw * EPS, (p, r["pearson"], f32[0])
            assert abs(r["spearman"] - f64[1]) <= 2.0 ** -50 and abs(r["spearman"] - f32[1]) <= 2.0 ** -50, p
            assert r["iou"][j] == f64[2] == f32[2], (p, j)
        if a == b and not np.all(maps[a] == maps[a, 0]):
            assert r["spearman"] == 1.0
        if 4 in (a, b):
            assert r["pearson"] == 0.0 and r["spearman"] == 0.0


def test_ranks_and_heat_map_restatements():
    """A check of the yardstick, not of the feature (it runs only explain_ref.py and torch, so it passes without the
    kernels): the rank restatement against a brute-force count, the heat-map restatement against F.interpolate, and
    the identity that lets the kernel skip the reference's second upscale_heatmap."""
    g = np.random.default_rng(5)
    a = g.integers(0, 6, 40).astype(np.float32)
    a[3], a[7] = 0.0, -0.0
    brute = np.array([2 * (a < x).sum() + (a == x).sum() + 1 for x in a])  # 2 x the average of ranks lo+1 .. lo+cnt
    assert np.array_equal(er.ranks2(a), brute)
    for gsz, size in ((2, (8, 8)), (3, (30, 20)), (7, (28, 28)), (7, (224, 224)), (3, (5, 3))):
        v = g.random(gsz * gsz).astype(np.float32)
        n = torch.from_numpy(v)
        n = (n - n.min()) / (n.max() - n.min() + 1e-8)
        ref = F.interpolate(n.view(1, 1, gsz, gsz), size=size, mode="bilinear", align_corners=False)[0, 0].numpy()
        # twice through it is the identity (the reference's upscale_heatmap to the same size is not run)
        again = F.interpolate(torch.from_numpy(ref)[None, None], size=size, mode="bilinear", align_corners=False)
        assert torch.equal(again[0, 0], torch.from_numpy(ref))
        assert np.abs(er.heat_map(v, size) - ref).max() <= er.tol_pixel(er.tol_norm(v), gsz)


def test_signatures_and_key_names():
    sig = inspect.signature(MultiModalRetrievalModel.predict)
    assert list(sig.parameters)[:7] == ["self", "image", "input_ids", "attention_mask", "threshold", "K", "explain"]
    assert sig.parameters["explain"].default is False and sig.parameters["K"].default == 5
    sig = inspect.signature(MultiModalRetrievalModel.explain_attention)
    assert list(sig.parameters) == ["self", "image", "input_ids", "attention_mask", "layer", "image_size"]
    assert sig.parameters["layer"].default == -1 and sig.parameters["image_size"].default == (224, 224)
    sig = inspect.signature(MultiModalRetrievalModel.evaluate_explanations)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [
        ("K", 10), ("fracs", (0.05, 0.20)), ("image_size", (224, 224)), ("exclude_self", False),
        ("return_per_query", False)]
    sig = inspect.signature(metrics.compare_maps)
    assert list(sig.parameters) == ["map_a", "map_b", "topk_frac"] and sig.parameters["topk_frac"].default == 0.05
    sig = inspect.signature(ops.map_alignment)
    assert list(sig.parameters) == ["maps", "pa", "pb", "fracs"] and sig.parameters["fracs"].default == (0.05, 0.20)
    sig = inspect.signature(FusionStack.forward)
    assert sig.parameters["attention_layers"].default is None and sig.parameters["return_attention"].default is False
    for frac, key in ((0.05, "iou_top5pct"), (0.20, "iou_top20pct"), (0.29, "iou_top28pct"), (0.07, "iou_top7pct"),
                      (1.0, "iou_top100pct")):
        assert metrics.iou_key(frac) == er.iou_key(frac) == key == f"iou_top{int(frac * 100)}pct"
    for n, frac, k in ((784, 0.05, 39), (784, 0.20, 156), (16, 0.05, 1), (50176, 0.05, 2508), (50176, 0.20, 10035),
                       (784, 0.29, 227), (10, 1.0, 10)):
        assert ops.topk_count(n, frac) == er.topk_count(n, frac) == k == max(1, int(n * frac))


def test_entry_points_refuse_before_touching_the_device():
    L = _lib.lib()
    P = ctypes.c_void_p(4096)  # never dereferenced: every case is refused first

    def explain(lt=5, npatch=9, lcr=11, lcc=11, T=5, H=8, W=8, maps=P):
        st = L.mmr_explain_attention(P, lt * npatch, npatch, P, npatch * lt, lt, P, lcr * lcc, lcc, 1, lt, npatch, lcr,
                                     lcc, T, H, W, P, P, P, P, P, P, maps, maps, maps, P, P, P, P, None)
        return st, L.mmr_last_error().decode()
    for kw, match in ((dict(npatch=8), "perfect square"), (dict(npatch=1089), "Np = 1089"), (dict(npatch=0), "Np = 0"),
                      (dict(lt=4097), "Lt = 4097"), (dict(lcr=4097, lcc=4097), "Lc = 4097"),
                      (dict(lcr=11, lcc=12), "not square"), (dict(H=0), "pixels"), (dict(H=257, W=256), "pixels"),
                      (dict(maps=ctypes.c_void_p(4100)), "16-B aligned")):
        st, msg = explain(**kw)
        assert st == 1 and match in msg, (kw, st, msg)
    assert L.mmr_explain_attention_work_bytes(2, 128, 49, 51) >= 2 * 51 * 8
    assert L.mmr_explain_attention_work_bytes(2, 4097, 49, 51) == 0
    assert L.mmr_explain_attention_work_bytes(2, 128, 1025, 51) == 0
    assert L.mmr_explain_attention_work_bytes(2, 128, 49, 4097) == 0
    for n, hw, nf, k0, match in ((65537, 16, 1, 1, "N = 65537"), (0, 16, 1, 1, "N = 0"), (8, 65537, 1, 1, "HW = 65537"),
                                 (65536, 32768, 1, 1, "2^31"), (8, 16, 1, 17, "k[0] = 17"), (8, 16, 1, 0, "k[0] = 0"),
                                 (8, 16, 5, 1, "5 fractions")):
        st = L.mmr_map_alignment(P, hw, n, hw, P, P, 1, nf, k0, 1, 1, 1, P, P, P, P, P, P, P, P, P, P, P, P, None)
        assert st == 1 and match in L.mmr_last_error().decode(), (n, hw, nf, k0, L.mmr_last_error())
    assert L.mmr_map_alignment_work_bytes(65537, 16) == 0 and L.mmr_map_alignment_work_bytes(8, 65537) == 0
    assert L.mmr_map_alignment_work_bytes(65536, 32768) == 0
    assert L.mmr_map_alignment_work_bytes(8, 784) >= 2 * 8 * 784 * 8
