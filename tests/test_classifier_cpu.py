"""CPU: the classifier head / predict() boundary without a GPU.

* classifier_ref (the f64 restatement the GPU test compares against) reproduces the reference's own logits and
  predict() outputs (tests/golden/predict_mini.npz, written by the reference on the towers_mini.npz weights and
  stored joint embeddings): logits within the head's bound, preds equal outside the threshold band, top-K
  tie-aware equal, at both recorded (threshold, K) settings and for all three model_types;
* predict's signature is the reference's parameter list (model.py:491-498), plus keyword-only extras;
* mmr_classifier_head / _pack reject invalid arguments before the device is touched;
* for every case of the GPU test the two sets it leaves out of its exact comparisons are small on the reference
  alone: at most 1 % of the (b, c) entries lie in the threshold band, and no tie group touching the top-K holds
  more than K + 2 classes."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import classifier_ref as cr
from attn_maps_ref import towers_mini
from mmr_amd.model import MultiModalRetrievalModel, init_classifier_state, init_head_state

from conftest import GOLDEN

# model.py:491-498 (names in order, default)
REF_PREDICT = [("image", inspect.Parameter.empty), ("input_ids", inspect.Parameter.empty),
               ("attention_mask", inspect.Parameter.empty), ("threshold", 0.5), ("K", 5), ("explain", False)]
SETTINGS = (("t50_k5", 0.5, 5), ("t30_k43", 0.3, 43))


@pytest.fixture(scope="module")
def mini():
    f, w = towers_mini()
    h = w["head"]
    cls = (h["classifier.0.weight"], h["classifier.0.bias"], h["classifier.3.weight"], h["classifier.3.bias"])
    gold = np.load(os.path.join(GOLDEN, "predict_mini.npz"), allow_pickle=False)
    return f, cls, gold


@pytest.mark.parametrize("mt", ["text", "image", "multimodal"])
def test_ref_reproduces_reference_fixture(mini, mt):
    f, cls, gold = mini
    assert cls[0].shape == (256, 64) and cls[2].shape == (43, 256)
    logits, probs, bound, pbound = cr.head_f64(torch.from_numpy(f[f"{mt}_joint_emb"]), *cls)
    g = torch.from_numpy(gold[f"{mt}_logits"]).double()
    assert g.shape == (2, 43)
    assert ((g - logits).abs() <= bound).all(), ((g - logits).abs() - bound).max().item()
    for tag, thr, k in SETTINGS:
        gp = torch.from_numpy(gold[f"{mt}_{tag}_probs"]).double()
        assert ((gp - probs).abs() <= pbound).all()
        out = ~cr.band(probs, pbound, thr)
        assert torch.equal(torch.from_numpy(gold[f"{mt}_{tag}_preds"])[out], cr.preds_of(probs, thr)[out])
        assert gold[f"{mt}_{tag}_preds"].dtype == np.int32
        gi = gold[f"{mt}_{tag}_topk_idx"]
        assert gi.shape == (2, k)
        assert cr.topk_mismatches(gi, probs, pbound) == []
        gv = torch.from_numpy(gold[f"{mt}_{tag}_topk_vals"]).double()
        assert ((gv - torch.gather(probs, 1, torch.from_numpy(gi))).abs() <= torch.gather(pbound, 1, torch.from_numpy(gi))).all()


def test_tie_aware_comparison_rejects_and_accepts():
    """The comparison itself: a swap inside a tie group passes, a swap across groups or a repeated class fails."""
    p = torch.tensor([[0.9, 0.5, 0.5 + 1e-7, 0.1]], dtype=torch.float64)
    e = torch.full_like(p, 1e-6)
    assert cr.order_of(p).tolist() == [[0, 2, 1, 3]]
    assert cr.topk_mismatches([[0, 2, 1]], p, e) == [] and cr.topk_mismatches([[0, 1, 2]], p, e) == []
    assert cr.topk_mismatches([[0, 1]], p, e) == []            # the group straddles K
    assert cr.topk_mismatches([[1, 0, 2]], p, e) == [0]
    assert cr.topk_mismatches([[0, 1, 1]], p, e) == [0]
    assert cr.topk_mismatches([[0, 2, 3]], p, e) == [0]
    assert cr.max_tie_group_in_topk(p, e, 1) == 1 and cr.max_tie_group_in_topk(p, e, 2) == 2
    eq = torch.tensor([[0.5, 0.75, 0.5, 0.75]])
    assert cr.order_of(eq).tolist() == [[1, 3, 0, 2]]          # equal probabilities: the lower class first
    v, i = cr.exact_topk(eq, 3)
    assert i.tolist() == [[1, 3, 0]] and v.tolist() == [[0.75, 0.75, 0.5]]
    # the threshold is compared as f32: 0.3 in f64 lies below float32(0.3)
    assert cr.preds_of(torch.tensor([[0.3, float(np.float32(0.3)), 0.31]], dtype=torch.float64), 0.3).tolist() == \
        [[0, 1, 1]]


def test_predict_signature_mirrors_reference():
    ps = [p for p in inspect.signature(MultiModalRetrievalModel.predict).parameters.values() if p.name != "self"]
    pos = [(p.name, p.default) for p in ps if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert pos == REF_PREDICT
    extra = [p for p in ps if p.kind != p.POSITIONAL_OR_KEYWORD]
    assert [(p.name, p.kind, p.default) for p in extra] == [("retrieve", inspect.Parameter.KEYWORD_ONLY, False)]


def test_init_classifier_state_is_separate():
    """init_classifier_state has its own keys and RNG stream: init_head_state is what it was (no classifier keys:
    the bench model and smoke() build no classifier)."""
    hs = init_head_state(32, 48, 16, 3)
    assert not any(k.startswith("classifier.") for k in hs)
    cs = init_classifier_state(16, 7, 5)
    assert {k: tuple(v.shape) for k, v in cs.items()} == {
        "classifier.0.weight": (64, 16), "classifier.0.bias": (64,), "classifier.3.weight": (7, 64),
        "classifier.3.bias": (7,)}
    again = init_classifier_state(16, 7, 5)
    assert all(torch.equal(cs[k], again[k]) for k in cs)
    hs2 = init_head_state(32, 48, 16, 3)
    assert all(torch.equal(hs[k], hs2[k]) for k in hs)


def test_invalid_arguments_without_gpu():
    from mmr_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected on the host
    N = None

    def head(x=p, logits=p, tv=N, ti=N, b=4, d=128, h=512, c=43, k=5, ldx=128, images=p):
        return L.mmr_classifier_head(x, ldx, images, p, p, p, logits, N, N, tv, ti, b, d, h, c, k, 0.5, N)

    assert head(x=N) == 1 and b"NULL" in L.mmr_last_error()
    assert head(logits=N) == 1 and b"NULL" in L.mmr_last_error()
    assert head(images=N) == 1
    assert head(c=0) == 1 and b"c=0" in L.mmr_last_error()
    assert head(tv=p, k=44) == 1 and b"k=44" in L.mmr_last_error()
    assert head(ti=p, k=0) == 1
    assert head(ldx=100) == 1 and head(ldx=130) == 1
    assert head(c=257) == 4 and b"not built" in L.mmr_last_error()       # MMR_ERR_UNSUPPORTED
    assert head(d=100, h=400) == 4
    assert head(x=ctypes.c_void_p(260)) == 1                               # misaligned rows
    assert head(b=-1) == 1
    assert head(b=0) == 0 and head(b=0, k=99) == 0                         # nothing to do; k unread without top-K
    assert L.mmr_classifier_pack(N, p, p, 128, 512, 43, N) == 1
    assert L.mmr_classifier_pack(p, p, p, 128, 512, 300, N) == 4
    # sizes: fused geometry NS slabs of (b, Cp) f32; chain geometry one (b, Cp) partial + the (b, H) hidden
    assert L.mmr_classifier_work_bytes(256, 768, 3072, 43) == 32 * 256 * 64 * 4
    assert L.mmr_classifier_work_bytes(2048, 1024, 4096, 43) == 32 * 2048 * 64 * 4
    assert L.mmr_classifier_work_bytes(33, 96, 384, 43) == 33 * 64 * 4 + 33 * 384 * 4
    assert L.mmr_classifier_work_bytes(4, 100, 400, 43) == 0 and L.mmr_classifier_pack_bytes(100, 400, 43) == 0
    assert L.mmr_classifier_pack_bytes(768, 3072, 43) == (3072 * 768 * 2 + 3072 * 64 * 2) * 2
    # the slab partition is a function of D alone: the same workspace per row at any b
    for d in (128, 256, 384, 512, 640, 768, 896, 1024):
        per_row = L.mmr_classifier_work_bytes(1, d, 4 * d, 43)
        assert per_row > 0 and L.mmr_classifier_work_bytes(257, d, 4 * d, 43) == 257 * per_row


@pytest.mark.parametrize("B,D,H,C", cr.CASES)
def test_left_out_sets_are_small(B, D, H, C):
    _, (logits, probs, bound, pbound) = cr.case(B, D, H, C)
    share = cr.band(probs, pbound, cr.THRESHOLD).double().mean().item()
    assert share <= 0.01, share
    assert pbound.max().item() < 1e-3  # the bound itself stays far below the spacing of the probabilities
    for k in cr.case_ks(C):
        assert cr.max_tie_group_in_topk(probs, pbound, k) <= k + 2, k
