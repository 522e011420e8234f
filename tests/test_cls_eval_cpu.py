"""CPU: the numpy reference of the classifier evaluation (cls_eval_ref.py) against what scikit-learn recorded in
tests/golden/cls_eval.npz (make_golden_cls_eval.py), against a live scikit-learn where one is installed, and on the
edge cases the device kernels are held to (-0 / +0, denormals, N = 1) — before test_cls_eval_gpu.py relies on it.
Also the host-side plumbing that needs no GPU: label packing, the C ABI's argument checks.

Tolerances (derived in cls_eval_ref.py): thresholds bit-equal, counts equal, AUROC / AP within N * 2^-52 of
scikit-learn's (N * C * 2^-52 for the micro AP)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cls_eval_ref as R
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "cls_eval.npz"))


def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    assert (np.abs(a[ok] - b[ok]) <= tol).all(), np.abs(a[ok] - b[ok]).max()


def test_fixture_is_the_described_case(gold):
    S, Y = gold["scores"], gold["labels"]
    ties, tied, nopos, allpos = (int(v) for v in gold["special"])
    assert S.shape == (257, 43) and S.dtype == np.float32 and Y.shape == S.shape
    assert len(np.unique(S[:, ties])) == 8 and len(np.unique(S[:, tied])) == 1
    assert Y[:, nopos].sum() == 0 and Y[:, allpos].sum() == 257
    assert np.isnan(gold["auroc"][[nopos, allpos]]).all() and np.isnan(gold["auroc"]).sum() == 2


def test_reference_vs_recorded_sklearn(gold):
    S, Y = gold["scores"], gold["labels"]
    N, C = S.shape
    r, m = R.cls_eval_ref(S, Y), R.metrics_ref(S, Y)
    assert np.array_equal(r["best_thr"][:C].astype(np.float64).view(np.int64), gold["best_ts"].view(np.int64))
    off = gold["pr_offsets"]
    assert np.array_equal(r["counts"][:C, 3], np.diff(off))          # distinct scores = sklearn's thresholds
    assert np.array_equal(r["counts"][:C, 0], Y.sum(0)) and np.array_equal(r["counts"][:C, 1], N - Y.sum(0))
    for k, name in enumerate(("tp", "fp", "fn")):
        assert np.array_equal(r["confusion"][:C, k], gold[name])
    pc = m["per_class"]
    _close(pc["auroc"], gold["auroc"], R.AP_TOL(N))
    _close(pc["ap"], gold["ap"], R.AP_TOL(N))
    _close(m["micro_ap"], gold["micro_ap"], R.AP_TOL(N * C))
    for name in ("prec", "rec", "f1"):
        _close(pc[name], gold[name], R.AP_TOL(N))
    _close([m["macro_prec"], m["macro_rec"], m["macro_f1"]], gold["macro"], R.AP_TOL(N))
    _close([m["micro_prec"], m["micro_rec"], m["micro_f1"]], gold["micro"], R.AP_TOL(N))
    # a class without positives gets its minimum score (the reference's behaviour)
    nopos = int(gold["special"][2])
    assert r["best_thr"][nopos] == S[:, nopos].min()


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_reference_vs_live_sklearn(family, n):
    skm = pytest.importorskip("sklearn.metrics")
    import warnings
    c = 5
    S, Y = R.scores(family, n, c, 100 + n), R.labels(n, c, 200 + n)
    r, m = R.cls_eval_ref(S, Y), R.metrics_ref(S, Y)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j in range(c):
            p, rc, t = skm.precision_recall_curve(Y[:, j], S[:, j])
            f1 = 2 * p * rc / (p + rc + 1e-8)
            # -0 and +0 are one score: compared as values (sklearn returns whichever zero its sort met last)
            assert float(t[f1.argmax()]) == float(r["best_thr"][j])
            assert len(np.unique(t + 0.0)) == r["counts"][j, 3]
            if 0 < Y[:, j].sum() < n:
                assert abs(skm.roc_auc_score(Y[:, j], S[:, j]) - m["per_class"]["auroc"][j]) <= R.AP_TOL(n)
                assert abs(skm.average_precision_score(Y[:, j], S[:, j]) - m["per_class"]["ap"][j]) <= R.AP_TOL(n)
            else:
                assert np.isnan(m["per_class"]["auroc"][j]) and np.isnan(m["per_class"]["ap"][j])
        assert abs(skm.average_precision_score(Y, S, average="micro") - m["micro_ap"]) <= R.AP_TOL(n * c)
        pred = (S > r["best_thr"][None, :c]).astype(int)
        for avg, names in (("macro", ("macro_prec", "macro_rec", "macro_f1")),
                           ("micro", ("micro_prec", "micro_rec", "micro_f1"))):
            for fn, name in zip((skm.precision_score, skm.recall_score, skm.f1_score), names):
                assert abs(fn(Y, pred, average=avg, zero_division=0) - m[name]) <= R.AP_TOL(n)


def test_signed_zero_is_one_score():
    S = np.array([[0.0], [-0.0], [1e-3], [-1e-3]], np.float32)
    Y = np.array([[1], [0], [1], [0]])
    r = R.curve(S[:, 0], Y[:, 0])
    assert r["n_distinct"] == 3                      # {1e-3}, {+0, -0}, {-1e-3}
    assert r["A"] == 2 * 2 + (1 + 2)                 # 1e-3 beats both negatives; +0 ties with -0 and beats -1e-3
    assert r["best_thr"].view(np.uint32) == 0        # the canonical +0, whichever zero the data holds
    S2 = S.copy()
    S2[[0, 1]] = S2[[1, 0]]                          # the positive now carries -0
    r2 = R.curve(S2[:, 0], Y[:, 0])
    assert (r2["A"], r2["n_distinct"], int(r2["best_thr"].view(np.uint32))) == (r["A"], 3, 0)
    # score > threshold treats them alike too
    assert R.cls_eval_ref(S, Y, thresholds=np.float32(-0.0))["confusion"][0].tolist() == [1, 0, 1]


def test_denormals_are_distinct_and_ordered():
    bits = np.array([0x00000001, 0x00000002, 0x80000001, 0x80000002, 0x00000000, 0x00800000], np.uint32)
    s = bits.view(np.float32)
    img = R.order_image(s)
    assert len(set(img.tolist())) == 6
    assert img.argsort().tolist() == [3, 2, 4, 0, 1, 5]   # -2d < -1d < 0 < 1d < 2d < smallest normal
    assert np.array_equal(R.image_score(img).view(np.uint32), bits)
    r = R.curve(s, np.array([0, 1, 0, 0, 0, 1]))
    assert r["n_distinct"] == 6 and r["A"] == 2 * 8     # both positives outrank all four negatives
    assert r["best_thr"].view(np.uint32) == 0x00000002  # f1 = 1 at the denormal 2^-148, returned bit for bit


def test_single_sample():
    r = R.cls_eval_ref(np.array([[0.7, 0.2]], np.float32), np.array([[1, 0]]))
    assert r["counts"].tolist() == [[1, 0, 0, 1], [0, 1, 0, 1], [1, 1, 2, 2]]
    assert r["best_thr"][:2].tolist() == [np.float32(0.7), np.float32(0.2)]
    assert r["confusion"].tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 1]]   # score > its own value: nothing predicted
    m = R.metrics_ref(np.array([[0.7, 0.2]], np.float32), np.array([[1, 0]]))
    assert np.isnan(m["macro_auc"]) and np.isnan(m["macro_ap"]) and m["micro_ap"] == 1.0


def test_label_bits_packing():
    from mmr_amd import metrics
    Y = R.labels(37, 64, 5)
    Y[:, 63] = np.arange(37) % 2                        # the sign bit of the int64 carrier
    want = R.pack_bits(Y)
    for form in (Y, torch.from_numpy(Y), Y.astype(np.float32), Y.astype(bool)):
        bits, bad = metrics.label_bits(form, 64, "cpu")
        assert bits.dtype == torch.int64 and not bool(bad)
        assert np.array_equal(bits.numpy().view(np.uint64), want)
    for form in (want, want.view(np.int64), torch.from_numpy(want.view(np.int64))):
        bits, bad = metrics.label_bits(form, 64, "cpu")
        assert np.array_equal(bits.numpy().view(np.uint64), want) and not bool(bad)
    Y2 = Y.astype(np.int64)
    Y2[3, 4] = 2
    assert bool(metrics.label_bits(Y2, 64, "cpu")[1])
    with pytest.raises(ValueError, match="labels must be"):
        metrics.label_bits(Y[:, :10], 64, "cpu")


def test_capi_argument_checks():
    """mmr_cls_eval / mmr_cls_eval_work_bytes reject bad shapes and NULL pointers before the device is touched."""
    from mmr_amd import _lib
    L = _lib.lib()
    assert L.mmr_cls_eval_work_bytes(0, 43) == 0 and L.mmr_cls_eval_work_bytes(10, 65) == 0
    assert L.mmr_cls_eval_work_bytes(10, 0) == 0 and L.mmr_cls_eval_work_bytes(2 ** 31 // 43 + 1, 43) == 0
    small, big = L.mmr_cls_eval_work_bytes(257, 43), L.mmr_cls_eval_work_bytes(100000, 43)
    assert 2 * 8 * 257 * 43 <= small < big and big >= 2 * 8 * 100000 * 43    # two arrays of u64 keys at least
    p = ctypes.c_void_p(256)

    def call(n=10, c=4, lds=4, scores=p, bits=p, out=p, work=p):
        return L.mmr_cls_eval(scores, lds, bits, n, c, None, out, out, out, out, out, out, work, None)
    for kw, msg in ((dict(n=0), b"n = 0"), (dict(c=65, lds=65), b"outside 1..64"), (dict(c=0), b"outside 1..64"),
                    (dict(n=2 ** 30, c=4), b"2^31"), (dict(lds=3), b"row stride"), (dict(scores=None), b"NULL"),
                    (dict(bits=None), b"NULL"), (dict(out=None), b"NULL output"), (dict(work=None), b"work"),
                    (dict(work=ctypes.c_void_p(264)), b"16-B aligned")):
        assert call(**kw) == 1 and msg in L.mmr_last_error(), (kw, L.mmr_last_error())
