"""GPU: the classifier evaluation (mmr_cls_eval, csrc/cls_eval.hip) through ops.cls_eval,
metrics.classification_metrics / find_best_thresholds, MultiModalRetrievalModel.evaluate_classifier and predict's
per-class thresholds, against the numpy reference of cls_eval_ref.py (itself held to scikit-learn by
test_cls_eval_cpu.py).

Bars: n_pos, n_neg, A, n_distinct, the best thresholds (float32 bits), the best f1 (f64 bits: the same IEEE
expression, contraction off), tp / fp / fn and the AUROC are bit-equal; AP within N * 2^-52 (N * C * 2^-52 for the
micro AP), the bound cls_eval_ref.py derives; the aggregates within the same bounds.  Shapes: every N around the
64-key sort round, the 256-key scan chunk and the 1024-key curve tile with C = 1 / 43 / 64, and 70001 x 3, where
class boundaries fall inside sort chunks and a segment spans many workgroups."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import cls_eval_ref as R
from attn_maps_ref import towers_mini
from mmr_amd import metrics, ops, synthetic
from mmr_amd.model import Backbones, MultiModalRetrievalModel
from mmr_amd.towers import BERT_BASE, SWIN_T

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
NS, CS = (1, 2, 63, 64, 65, 255, 257, 1000, 4097), (1, 43, 64)


@functools.lru_cache(maxsize=None)
def _case(family, n, c):
    S, Y = R.scores(family, n, c, 1000 * c + n), R.labels(n, c, 2000 * c + n)
    for a in (S, Y):
        a.setflags(write=False)
    return S, Y, R.cls_eval_ref(S, Y), R.metrics_ref(S, Y)


def _run(S, Y, thresholds=None):
    bits = torch.from_numpy(R.pack_bits(Y).view(np.int64)).to(DEV)
    s = S if isinstance(S, torch.Tensor) else torch.tensor(np.asarray(S), device=DEV)
    t = None if thresholds is None else torch.from_numpy(np.asarray(thresholds, np.float32)).to(DEV)
    return {k: v.cpu().numpy() for k, v in ops.cls_eval(s, bits, Y.shape[1], t).items()}


def _check_raw(out, ref, n, c, tag):
    assert out["nonfinite"].tolist() == [0]
    assert np.array_equal(out["counts"], ref["counts"]), tag
    assert np.array_equal(out["best_thr"].view(np.uint32), ref["best_thr"].view(np.uint32)), tag
    assert np.array_equal(out["best_f1"].view(np.int64), ref["best_f1"].view(np.int64)), tag
    assert np.array_equal(out["confusion"], ref["confusion"]), tag
    P = np.maximum(ref["counts"][:, 0], 1).astype(np.float64)
    err = np.abs(out["ap_sum"] / P - ref["ap_sum"] / P)
    tol = np.r_[np.full(c, R.AP_TOL(n)), R.AP_TOL(n * c)]
    print(json.dumps({tag: {"ap_err": float(err.max()), "tol": float(tol.min())}}))
    assert (err <= tol).all(), (tag, err.max())


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(a.view(np.int64), b.view(np.int64)) or (np.array_equal(np.isnan(a), np.isnan(b))
                                                                   and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


def _near(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = ~np.isnan(a)
    return np.array_equal(np.isnan(a), np.isnan(b)) and bool((np.abs(a[ok] - b[ok]) <= tol).all())


def _check_metrics(m, ref, n, c):
    assert (m["num_samples"], m["num_classes"]) == (n, c)
    pc, rc = m["per_class"], ref["per_class"]
    assert _same(pc["auroc"], rc["auroc"])
    assert pc["thresholds"] == rc["thresholds"] and pc["n_pos"] == rc["n_pos"]
    for k in ("prec", "rec", "f1"):
        assert pc[k] == rc[k], k
    assert _near(pc["ap"], rc["ap"], R.AP_TOL(n))
    for k in ("macro_auc", "macro_ap", "macro_f1", "macro_prec", "macro_rec", "micro_prec", "micro_rec", "micro_f1"):
        assert _near(m[k], ref[k], R.AP_TOL(n)), k
    assert _near(m["micro_ap"], ref["micro_ap"], R.AP_TOL(n * c))


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_shapes_and_families(n, c):
    for family in R.FAMILIES:
        S, Y, ref, mref = _case(family, n, c)
        _check_raw(_run(S, Y), ref, n, c, f"{family}-{n}x{c}")
    S, Y, ref, mref = _case("distinct", n, c)
    _check_metrics(metrics.classification_metrics(Y, S), mref, n, c)


@pytest.mark.parametrize("family", ["distinct", "ties8"])
def test_many_workgroups_per_segment(family):
    n, c = 70001, 3
    S, Y, ref, mref = _case(family, n, c)
    _check_raw(_run(S, Y), ref, n, c, f"{family}-{n}x{c}")
    _check_metrics(metrics.classification_metrics(Y, S), mref, n, c)


@pytest.mark.parametrize("n,c", [(257, 43), (4097, 64), (1000, 1)])
def test_strided_scores_and_determinism(n, c):
    S, Y, ref, _ = _case("logits", n, c)
    wide = torch.full((n, c + 5), float("nan"), device=DEV)      # the columns past C are never read
    wide[:, :c] = torch.tensor(S).to(DEV)
    a, b, v = _run(S, Y), _run(S, Y), _run(wide[:, :c], Y)
    _check_raw(a, ref, n, c, f"strided-{n}x{c}")
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k     # two runs: identical bytes
        assert np.array_equal(a[k].view(np.uint8), v[k].view(np.uint8)), k     # the row stride changes nothing


@pytest.mark.parametrize("family,n,c", [("distinct", 4097, 43), ("ties8", 4097, 43), ("zeros", 1000, 64),
                                        ("ties8", 70001, 3)])
def test_row_permutation_invariance(family, n, c):
    """The sort and the scans see another arrangement; every integer, threshold and AUROC must not move."""
    S, Y, ref, mref = _case(family, n, c)
    perm = np.random.default_rng(n + c).permutation(n)
    a, b = _run(S, Y), _run(S[perm], Y[perm])
    for k in ("counts", "confusion", "best_thr", "best_f1", "nonfinite"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    ma, mb = metrics.classification_metrics(Y, S), metrics.classification_metrics(Y[perm], S[perm])
    assert _same(ma["per_class"]["auroc"], mb["per_class"]["auroc"])
    assert ma["per_class"]["thresholds"] == mb["per_class"]["thresholds"]


def test_golden_sklearn_values():
    g = np.load(os.path.join(GOLDEN, "cls_eval.npz"))
    S, Y = g["scores"], g["labels"]
    n, c = S.shape
    m = metrics.classification_metrics(Y, S, label_names=[f"l{i}" for i in range(c)])
    pc = m["per_class"]
    assert pc["labels"][:2] == ["l0", "l1"]
    assert np.array_equal(np.asarray(pc["thresholds"], np.float64).view(np.int64), g["best_ts"].view(np.int64))
    assert pc["n_pos"] == Y.sum(0).tolist()
    out = _run(S, Y)
    assert np.array_equal(out["counts"][:c, 3], np.diff(g["pr_offsets"]))
    for k, name in enumerate(("tp", "fp", "fn")):
        assert np.array_equal(out["confusion"][:c, k], g[name])
    assert _near(pc["auroc"], g["auroc"], R.AP_TOL(n)) and _near(pc["ap"], g["ap"], R.AP_TOL(n))
    assert _near(m["micro_ap"], g["micro_ap"], R.AP_TOL(n * c))
    for name in ("prec", "rec", "f1"):
        assert _near(pc[name], g[name], R.AP_TOL(n))
    assert _near([m["macro_prec"], m["macro_rec"], m["macro_f1"]], g["macro"], R.AP_TOL(n))
    assert _near([m["micro_prec"], m["micro_rec"], m["micro_f1"]], g["micro"], R.AP_TOL(n))
    assert np.array_equal(metrics.find_best_thresholds(Y, S).astype(np.float64), g["best_ts"])


def test_fixed_thresholds_and_label_forms():
    n, c = 1000, 43
    S, Y, ref, mref = _case("distinct", n, c)
    vec = np.random.default_rng(3).random(c).astype(np.float32)
    vec[4] = S[17, 4]                                             # a threshold equal to a score: strictly greater
    for thr in (0.5, vec):
        rref = R.cls_eval_ref(S, Y, thresholds=thr)
        out = _run(S, Y, np.broadcast_to(np.float32(thr), (c,)).copy())
        assert np.array_equal(out["confusion"], rref["confusion"])
        assert np.array_equal(out["counts"], ref["counts"])       # the curve sums do not depend on them
        _check_metrics(metrics.classification_metrics(Y, S, thresholds=thr), R.metrics_ref(S, Y, thresholds=thr), n, c)
    assert metrics.classification_metrics(Y, S, thresholds=torch.from_numpy(vec))["per_class"]["thresholds"] == \
        [float(x) for x in vec]
    # dense labels (numpy / device tensor / bool) and bitsets: one result
    base = metrics.classification_metrics(Y, S)
    bits = R.pack_bits(Y)
    for form in (torch.tensor(Y).to(DEV), Y.astype(bool), bits, torch.from_numpy(bits.view(np.int64)).to(DEV)):
        assert json.dumps(metrics.classification_metrics(form, torch.tensor(S).to(DEV))) == json.dumps(base)
    assert np.array_equal(metrics.find_best_thresholds(bits, S).view(np.uint32), ref["best_thr"][:c].view(np.uint32))


def test_argument_errors():
    n, c = 65, 5
    S, Y, _, _ = _case("distinct", n, c)
    for bad in (np.nan, np.inf, -np.inf):
        S2 = S.copy()
        S2[7, 3] = bad
        with pytest.raises(ValueError, match="NaN or infinite"):
            metrics.classification_metrics(Y, S2)
        with pytest.raises(ValueError, match="NaN or infinite"):
            metrics.find_best_thresholds(Y, S2)
    assert _run(np.where(np.arange(c)[None, :] == 3, np.float32(np.nan), S), Y)["nonfinite"].tolist() == [n]
    with pytest.raises(ValueError, match="65 classes"):
        metrics.classification_metrics(np.zeros((4, 65), np.uint8), np.zeros((4, 65), np.float32))
    with pytest.raises(ValueError, match="samples"):
        metrics.classification_metrics(Y[:-1], S)
    with pytest.raises(ValueError, match="labels must be"):
        metrics.classification_metrics(Y[:, :4], S)
    with pytest.raises(ValueError, match="labels must be 0 or 1"):
        metrics.classification_metrics(Y.astype(np.int64) * 2, S)
    with pytest.raises(ValueError, match="thresholds"):
        metrics.classification_metrics(Y, S, thresholds=np.zeros(c + 1, np.float32))
    with pytest.raises(ValueError, match="finite"):
        metrics.classification_metrics(Y, S, thresholds=np.nan)
    sd = torch.tensor(S).to(DEV)
    bits = torch.from_numpy(R.pack_bits(Y).view(np.int64)).to(DEV)
    with pytest.raises(ValueError, match="num_classes"):
        ops.cls_eval(sd, bits, c + 1)
    with pytest.raises(ValueError, match="label_bits"):
        ops.cls_eval(sd, bits[:-1], c)
    with pytest.raises(ValueError, match="float32"):
        ops.cls_eval(sd.double(), bits, c)
    with pytest.raises(ValueError, match="thresholds"):
        ops.cls_eval(sd, bits, c, torch.zeros(c - 1, device=DEV))


# ---------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def mini_model():
    f, w = towers_mini()
    cfg = json.loads(bytes(f["cfg"]).decode())
    scfg = dict(SWIN_T, embed_dim=cfg["swin"]["embed_dim"], depths=cfg["swin"]["depths"],
                num_heads=cfg["swin"]["num_heads"])
    args = (torch.from_numpy(synthetic.image_from_u8(f["img_u8"])).to(DEV), torch.from_numpy(f["input_ids"]).to(DEV),
            torch.from_numpy(f["attention_mask"]).to(DEV))
    bb = Backbones(swin_state=w["swin"], bert_state=w["bert"], swin_cfg=scfg, bert_cfg=dict(BERT_BASE, **cfg["bert"]),
                   device=DEV, tower_dtype="x3")
    kw = dict(joint_dim=cfg["joint_dim"], num_heads=cfg["num_heads"], model_type="text", backbones=bb, device=DEV,
              use_shared_ffn=False)
    bare = {k: v for k, v in w["head"].items() if not k.startswith("classifier.")}
    return MultiModalRetrievalModel(head_state=w["head"], **kw), MultiModalRetrievalModel(head_state=bare, **kw), args


def test_evaluate_classifier(mini_model):
    """The fixture's 2-sample batch as three batches with different label rows (dense, dense on the device, bitsets):
    the result is classification_metrics of the concatenated probabilities; return_outputs adds the CSV's columns."""
    m, m0, args = mini_model
    C = m.num_classes
    Y = R.labels(6, C, 77, prevalence=0.5)
    batches = [(*args, Y[0:2]), (*args, torch.from_numpy(Y[2:4]).to(DEV)), (*args, R.pack_bits(Y[4:6]))]
    out = m.evaluate_classifier(batches, return_outputs=True)
    probs = m.predict(*args)["probs"]
    assert out["probs"].dtype == np.float32 and np.array_equal(out["probs"], np.concatenate([probs] * 3))
    assert out["labels"].dtype == np.int32 and np.array_equal(out["labels"], Y)
    thr = np.asarray(out["per_class"]["thresholds"], np.float32)
    assert out["preds"].dtype == np.int32
    assert np.array_equal(out["preds"], (out["probs"] > thr[None, :]).astype(np.int32))
    want = metrics.classification_metrics(Y, out["probs"])
    plain = m.evaluate_classifier(batches)
    assert sorted(plain) == sorted(want) and "probs" not in plain
    for d in (plain, {k: v for k, v in out.items() if k in want}):
        assert json.dumps(d) == json.dumps(want)
    _check_metrics(want, R.metrics_ref(out["probs"], Y), 6, C)
    fixed = m.evaluate_classifier(batches, thresholds=0.5)
    assert json.dumps(fixed) == json.dumps(metrics.classification_metrics(Y, out["probs"], thresholds=0.5))
    with pytest.raises(ValueError, match="predict needs classifier"):
        m0.evaluate_classifier(batches)
    with pytest.raises(ValueError, match="label rows"):
        m.evaluate_classifier([(*args, Y[0:3])])
    with pytest.raises(RuntimeError, match="no batches"):
        m.evaluate_classifier([])


def test_predict_per_class_thresholds(mini_model):
    m, _, args = mini_model
    C = m.num_classes
    base = m.predict(*args, threshold=0.5, K=5)
    want = ops.classifier_head(m(*args)["joint_emb"], m.classifier, k=5, threshold=0.5,
                               want=("probs", "preds", "topk_vals", "topk_idx"))
    assert np.array_equal(base["preds"], want["preds"].cpu().numpy())          # the scalar path: the kernel's preds
    assert np.array_equal(base["probs"], want["probs"].cpu().numpy())
    vec = np.linspace(0.3, 0.7, C).astype(np.float32)
    vec[3] = base["probs"][1, 3]                                                # equality predicts 1 (>=)
    for form in (vec, torch.from_numpy(vec), torch.from_numpy(vec).to(DEV), vec.tolist()):
        p = m.predict(*args, threshold=form, K=5)
        assert np.array_equal(p["probs"], base["probs"]) and p["topk_idx"] == base["topk_idx"]
        assert p["topk_vals"] == base["topk_vals"]
        assert p["preds"].dtype == np.int32
        assert np.array_equal(p["preds"], (p["probs"] >= vec[None, :]).astype(np.int32))
    assert p["preds"][1, 3] == 1
    assert np.array_equal(m.predict(*args, threshold=np.float32(0.5))["preds"], base["preds"])
    for bad in (vec[:-1], np.zeros((2, C), np.float32)):
        with pytest.raises(ValueError, match="threshold must be"):
            m.predict(*args, threshold=bad)
