"""GPU: the classifier head and predict() (csrc/cls_head.hip, ops.classifier_head, MultiModalRetrievalModel).

Bars (classifier_ref.py derives them): logits within `bound`, probs within `pbound` of the f64 restatement, per
element; preds == (returned probs >= float32(threshold)) exactly and == the reference's outside the threshold
band; the top-K is exactly the (prob desc, class asc) prefix of the RETURNED probs and tie-aware equal to the
reference's.  test_classifier_cpu.py caps the band and the tie groups for the same cases on the reference alone.
Outputs are dense (the C ABI has no output strides), so "columns past C" of row r are row r + 1's first entries,
which the per-element comparisons cover; guard rows after the last row cover the rest."""
import json
import os

import numpy as np
import pytest
import torch

import classifier_ref as cr
from attn_maps_ref import towers_mini
from mmr_amd import MI355XRetrievalEngine, ops, synthetic
from mmr_amd.model import Backbones, MultiModalRetrievalModel
from mmr_amd.towers import BERT_BASE, SWIN_T

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ("logits", "probs", "preds", "topk_vals", "topk_idx")
SENT_F, SENT_I = -7.5, -77


def _cw(w1, b1, w2, b2):
    return ops.ClassifierW(w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV))


def _check_outputs(res, ref, threshold, k, tag):
    """Every property of one classifier_head result (CPU tensors) against the f64 reference."""
    logits, probs, bound, pbound = ref
    el = (res["logits"].double() - logits).abs()
    ep = (res["probs"].double() - probs).abs()
    print(json.dumps({tag: {"logit_err": el.max().item(), "bound_min": bound.min().item(),
                            "prob_err": ep.max().item(), "pbound_min": pbound.min().item()}}))
    assert (el <= bound).all(), (el - bound).max().item()
    assert (ep <= pbound).all(), (ep - pbound).max().item()
    assert res["preds"].dtype == torch.int32
    assert torch.equal(res["preds"], cr.preds_of(res["probs"], threshold))           # bit-exact on the returned probs
    out = ~cr.band(probs, pbound, threshold)
    assert torch.equal(res["preds"][out], cr.preds_of(probs, threshold)[out])
    ev, ei = cr.exact_topk(res["probs"], k)
    assert res["topk_idx"].dtype == torch.int32 and tuple(res["topk_idx"].shape) == (probs.shape[0], k)
    assert torch.equal(res["topk_idx"].long(), ei) and torch.equal(res["topk_vals"], ev)
    assert cr.topk_mismatches(res["topk_idx"], probs, pbound) == []


@pytest.mark.parametrize("B,D,H,C", cr.CASES)
def test_shapes_vs_f64(B, D, H, C):
    (x, w1, b1, w2, b2), ref = cr.case(B, D, H, C)
    cw, xd = _cw(w1, b1, w2, b2), x.to(DEV)
    for k in cr.case_ks(C):
        # guard rows after (B, C) / (B, k): the outputs are the first B rows of larger dense buffers
        bufs = {n: torch.full((B + 2, k if n.startswith("topk") else C), SENT_I if n in ("preds", "topk_idx") else SENT_F,
                              dtype=torch.int32 if n in ("preds", "topk_idx") else torch.float32, device=DEV)
                for n in ALL}
        res = ops.classifier_head(xd, cw, k=k, threshold=cr.THRESHOLD, want=ALL, out={n: t[:B] for n, t in bufs.items()})
        again = ops.classifier_head(xd, cw, k=k, threshold=cr.THRESHOLD, want=ALL)
        torch.cuda.synchronize()
        for n in ALL:
            assert res[n].data_ptr() == bufs[n].data_ptr()
            assert (bufs[n][B:] == (SENT_I if n in ("preds", "topk_idx") else SENT_F)).all(), f"{n}: guard rows overwritten"
            assert torch.equal(res[n], again[n]), f"{n}: two runs differ"
        _check_outputs({n: t.cpu() for n, t in res.items()}, ref, cr.THRESHOLD, k, f"B{B}_D{D}_H{H}_C{C}_k{k}")
    only = ops.classifier_head(xd, cw)  # logits alone: the other outputs NULL
    assert list(only) == ["logits"] and torch.equal(only["logits"], res["logits"])


@pytest.mark.parametrize("B,D,H,C", cr.SPARSE_CASES)
def test_sparse_weights_tight_bound(B, D, H, C):
    """One-hot W1 rows and 4-sparse W2 rows: the same bound formula, here within 4x of the split's own error
    (classifier_ref.make_sparse_inputs), per element on logits and probs."""
    x, w1, b1, w2, b2 = cr.make_sparse_inputs(B, D, H, C)
    logits, probs, bound, pbound = cr.head_f64(x, w1, b1, w2, b2)
    res = {n: t.cpu() for n, t in ops.classifier_head(x.to(DEV), _cw(w1, b1, w2, b2), want=("logits", "probs")).items()}
    el, ep = (res["logits"].double() - logits).abs(), (res["probs"].double() - probs).abs()
    print(json.dumps({f"sparse_B{B}_D{D}_C{C}": {"logit_err_over_bound": (el / bound).max().item(),
                                                  "bound_median": bound.median().item()}}))
    assert (el <= bound).all(), (el / bound).max().item()
    assert (ep <= pbound).all()


def test_strided_rows_and_argument_errors():
    (x, w1, b1, w2, b2), _ = cr.case(33, 128, 512, 43)
    cw = _cw(w1, b1, w2, b2)
    wide = torch.zeros(33, 128 + 8, device=DEV)
    wide[:, :128] = x.to(DEV)
    a = ops.classifier_head(x.to(DEV), cw)["logits"]
    b = ops.classifier_head(wide[:, :128], cw)["logits"]  # ldx = 136
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="k="):
        ops.classifier_head(x.to(DEV), cw, want=("topk_idx",))
    with pytest.raises(ValueError, match="k=44"):
        ops.classifier_head(x.to(DEV), cw, k=44, want=("topk_idx",))
    with pytest.raises(ValueError, match="columns"):
        ops.classifier_head(x.to(DEV)[:, :64].contiguous(), cw)
    with pytest.raises(Exception, match="not built"):
        _cw(torch.zeros(512, 128), torch.zeros(512), torch.zeros(257, 512), torch.zeros(257))


@pytest.mark.parametrize("D,H", [(128, 512), (96, 384)])
def test_constructed_edges(D, H):
    """Exact values: a zero W2 row with b2 = 0 is logit 0, prob exactly 0.5, pred 1 at threshold 0.5; b2 = +-40 /
    +-100 saturate to exactly 1.0 / at most 1e-17, finite, equal probabilities ordered by the lower class; x = 0
    gives W2 GELU(b1) + b2."""
    B, C = 5, 12
    g = torch.Generator().manual_seed(D)
    x = torch.randn(B, D, generator=g)
    w1 = torch.randn(H, D, generator=g) * D ** -0.5
    b1 = torch.randn(H, generator=g) * 0.5
    w2 = torch.randn(C, H, generator=g) * (0.05 * H ** -0.5)
    b2 = torch.randn(C, generator=g)
    w2[3] = 0.0
    b2[3] = 0.0
    for c, v in ((1, 40.0), (7, 40.0), (4, -40.0), (9, 100.0), (10, -100.0), (0, 100.0)):
        w2[c] = 0.0  # the logit is exactly b2
        b2[c] = v
    cw = _cw(w1, b1, w2, b2)
    res = {n: t.cpu() for n, t in ops.classifier_head(x.to(DEV), cw, k=C, threshold=0.5, want=ALL).items()}
    assert torch.isfinite(res["logits"]).all() and torch.isfinite(res["probs"]).all()
    assert (res["logits"][:, 3] == 0).all() and (res["probs"][:, 3] == 0.5).all() and (res["preds"][:, 3] == 1).all()
    for c in (0, 1, 7, 9):
        assert (res["logits"][:, c] == b2[c]).all() and (res["probs"][:, c] == 1.0).all()
    for c in (4, 10):
        assert (res["logits"][:, c] == b2[c]).all()
        assert (res["probs"][:, c] >= 0).all() and (res["probs"][:, c] <= 1e-17).all() and (res["preds"][:, c] == 0).all()
    # the four saturated classes tie at exactly 1.0: lower class first; the two smallest come last
    assert res["topk_idx"][:, :4].tolist() == [[0, 1, 7, 9]] * B
    assert (res["topk_vals"][:, :4] == 1.0).all()
    assert {tuple(sorted(r)) for r in res["topk_idx"][:, -2:].tolist()} == {(4, 10)}
    ev, ei = cr.exact_topk(res["probs"], C)
    assert torch.equal(res["topk_idx"].long(), ei) and torch.equal(res["topk_vals"], ev)
    # x = 0
    z = ops.classifier_head(torch.zeros(B, D, device=DEV), cw)["logits"].cpu()
    logits, _, bound, _ = cr.head_f64(torch.zeros(B, D), w1, b1, w2, b2)
    hb = 0.5 * b1.double() * (1.0 + torch.erf(b1.double() / 2.0 ** 0.5))
    assert torch.allclose(logits[0], w2.double() @ hb + b2.double(), rtol=0, atol=1e-12)
    assert ((z.double() - logits).abs() <= bound).all()
    assert all(torch.equal(z[0], z[r]) for r in range(1, B))


def test_batch_independence():
    """A row's logits have the same bits computed alone, in B = 33 and in B = 257 (the slab partition depends
    on (D, H) only; rows of a tile do not mix)."""
    (x, w1, b1, w2, b2), _ = cr.case(257, 768, 3072, 43)
    cw, xd = _cw(w1, b1, w2, b2), x.to(DEV)
    full = ops.classifier_head(xd, cw, k=5, want=ALL)
    part = ops.classifier_head(xd[:33], cw, k=5, want=ALL)
    for n in ALL:
        assert torch.equal(full[n][:33], part[n]), n
    for r in (0, 5, 31, 32, 200, 256):
        one = ops.classifier_head(xd[r:r + 1], cw, k=5, want=ALL)
        for n in ALL:
            assert torch.equal(one[n][0], full[n][r]), (n, r)


SETTINGS = (("t50_k5", 0.5, 5), ("t30_k43", 0.3, 43))


@pytest.mark.parametrize("mt", ["text", "image", "multimodal"])
def test_reference_golden(mt):
    """The reference's own logits and predict() outputs (predict_mini.npz) from the mini weights on the stored
    joint embeddings, at both recorded (threshold, K) settings."""
    f, w = towers_mini()
    h = w["head"]
    cls = (h["classifier.0.weight"], h["classifier.0.bias"], h["classifier.3.weight"], h["classifier.3.bias"])
    gold = np.load(os.path.join(GOLDEN, "predict_mini.npz"), allow_pickle=False)
    joint = torch.from_numpy(f[f"{mt}_joint_emb"])
    logits, probs, bound, pbound = cr.head_f64(joint, *cls)
    cw = _cw(*cls)
    for tag, thr, k in SETTINGS:
        res = {n: t.cpu() for n, t in ops.classifier_head(joint.to(DEV), cw, k=k, threshold=thr, want=ALL).items()}
        _check_outputs(res, (logits, probs, bound, pbound), thr, k, f"{mt}_{tag}")
        assert ((res["logits"].double() - torch.from_numpy(gold[f"{mt}_logits"]).double()).abs() <= bound).all()
        assert ((res["probs"].double() - torch.from_numpy(gold[f"{mt}_{tag}_probs"]).double()).abs() <= pbound).all()
        out = ~cr.band(probs, pbound, thr)
        assert torch.equal(res["preds"][out], torch.from_numpy(gold[f"{mt}_{tag}_preds"])[out])
        # the reference's list and ours are both tie-aware equal to the f64 order (test_classifier_cpu.py: the
        # fixture's is); where no tie group is larger than one class they are the same list
        if cr.max_tie_group_in_topk(probs, pbound, k) == 1:
            gi = torch.from_numpy(gold[f"{mt}_{tag}_topk_idx"])
            assert torch.equal(res["topk_idx"].long(), gi)
            assert ((res["topk_vals"].double() - torch.from_numpy(gold[f"{mt}_{tag}_topk_vals"]).double()).abs()
                    <= torch.gather(pbound, 1, gi)).all()


@pytest.fixture(scope="module")
def mini_inputs():
    f, w = towers_mini()
    cfg = json.loads(bytes(f["cfg"]).decode())
    scfg = dict(SWIN_T, embed_dim=cfg["swin"]["embed_dim"], depths=cfg["swin"]["depths"],
                num_heads=cfg["swin"]["num_heads"])
    image = torch.from_numpy(synthetic.image_from_u8(f["img_u8"])).to(DEV)
    ids = torch.from_numpy(f["input_ids"]).to(DEV)
    mask = torch.from_numpy(f["attention_mask"]).to(DEV)
    return f, w, cfg, scfg, (image, ids, mask)


@pytest.mark.parametrize("tower_dtype", ["bf16", "x3"])
def test_forward_wiring(mini_inputs, tower_dtype):
    """forward's logits are classifier_head(joint_emb), bit for bit; without classifier.* keys logits is None and
    joint_emb keeps its bits; the weights decide num_classes."""
    f, w, cfg, scfg, args = mini_inputs
    bb = Backbones(swin_state=w["swin"], bert_state=w["bert"], swin_cfg=scfg, bert_cfg=dict(BERT_BASE, **cfg["bert"]),
                   device=DEV, tower_dtype=tower_dtype)
    bare = {k: v for k, v in w["head"].items() if not k.startswith("classifier.")}
    for mt in ("multimodal", "text"):
        kw = dict(joint_dim=cfg["joint_dim"], num_heads=cfg["num_heads"], model_type=mt, backbones=bb, device=DEV,
                  use_shared_ffn=False)
        m = MultiModalRetrievalModel(head_state=w["head"], **kw)
        m0 = MultiModalRetrievalModel(head_state=bare, **kw)
        assert m.num_classes == 43 and m0.num_classes == 22 and m0.classifier is None
        o, o0 = m(*args), m0(*args)
        assert o0["logits"] is None and torch.equal(o["joint_emb"], o0["joint_emb"])
        assert o["logits"].shape == (2, 43) and o["logits"].dtype == torch.float32 and o["logits"].is_cuda
        assert torch.equal(o["logits"], ops.classifier_head(o["joint_emb"], m.classifier)["logits"])
        for k in ("img_emb", "txt_emb"):
            assert torch.equal(o[k], o0[k])
        with pytest.raises(ValueError, match="classifier"):
            m0.predict(*args)


def test_predict(mini_inputs):
    """predict(): the reference's output schema from one forward + one classifier_head call; retrieve=True returns
    per query what retriever.retrieve returns; explain=True raises."""
    f, w, cfg, scfg, args = mini_inputs
    bb = Backbones(swin_state=w["swin"], bert_state=w["bert"], swin_cfg=scfg, bert_cfg=dict(BERT_BASE, **cfg["bert"]),
                   device=DEV, tower_dtype="x3")
    m = MultiModalRetrievalModel(joint_dim=cfg["joint_dim"], num_heads=cfg["num_heads"], model_type="text",
                                 backbones=bb, head_state=w["head"], device=DEV, use_shared_ffn=False)
    joint = m(*args)["joint_emb"]
    for thr, k in ((0.5, 5), (0.3, 43)):
        p = m.predict(*args, threshold=thr, K=k)
        assert sorted(p) == ["preds", "probs", "topk_idx", "topk_vals"]
        want = ops.classifier_head(joint, m.classifier, k=k, threshold=thr, want=ALL)
        assert p["probs"].dtype == np.float32 and p["probs"].shape == (2, 43)
        assert p["preds"].dtype == np.int32 and p["preds"].shape == (2, 43)
        assert np.array_equal(p["probs"], want["probs"].cpu().numpy())
        assert np.array_equal(p["preds"], want["preds"].cpu().numpy())
        assert p["topk_idx"] == want["topk_idx"].cpu().tolist() and p["topk_vals"] == want["topk_vals"].cpu().tolist()
        assert all(isinstance(i, int) for r in p["topk_idx"] for i in r) and len(p["topk_idx"][0]) == k
        assert all(isinstance(v, float) for r in p["topk_vals"] for v in r)
    with pytest.raises(NotImplementedError, match="Grad-CAM"):
        m.predict(*args, explain=True)
    with pytest.raises(ValueError, match="retriever"):
        m.predict(*args, retrieve=True)
    G = synthetic.gauss_gallery(500, cfg["joint_dim"], 17)
    eng = MI355XRetrievalEngine(embs=G, ids=[f"r{i}" for i in range(len(G))])
    m.set_retriever(eng)
    pr = m.predict(*args, K=4, retrieve=True)
    q = joint.cpu().numpy()
    assert len(pr["retrieval_ids"]) == 2 and len(pr["topk_idx"][0]) == 4
    for i in range(2):
        ids, dists = eng.retrieve(q[i], K=4)
        assert pr["retrieval_ids"][i] == ids and pr["retrieval_dists"][i] == dists and len(ids) == 4
    eng.close()
