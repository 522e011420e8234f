"""CPU: the f64 restatement of the retrieval-diversity semantics (list_div_ref.py) and the host mirrors in
mmr_amd.metrics against what the reference's own functions recorded in tests/golden/list_diversity.npz
(make_golden_list_diversity.py) — before test_list_diversity_gpu.py relies on the restatement.  Also the plumbing
that needs no GPU: the C ABI's argument checks and the loader's prototypes.

Tolerances (derived in list_div_ref.py): label diversity bit-equal; embedding diversity within
TOL32(d, P) = (d + 4 + P) 2^-24 of the reference, which works in f32."""
import ctypes
import math
import os

import numpy as np
import pytest

import list_div_ref as R
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "list_diversity.npz"))


def _bits_eq(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def test_fixture_is_the_described_case(gold):
    lists = R.fixture_lists(gold)
    assert 35 <= len(lists) <= 45
    for d in (5, 16, 64):
        assert {len(ix) for dd, ix in lists if dd == d} >= {0, 1, 2, 3, 5, 10}
    assert sum(1 for d, ix in lists if d == 768 and len(ix) == 5) == 3
    G4, G16, b64 = gold["G_4"], gold["G_16"], gold["bits_64"]
    assert G4.dtype == np.float32 and np.linalg.norm(G4[0].astype(np.float64)) < 1e-8 and not G4[2].any()
    assert not G16[20].any() and np.array_equal(G16[3], G16[21])
    assert R.popcount(b64[[4, 5]]).tolist() == [43, 64] and not b64[:3].any()
    assert any(len(ix) != len(set(ix.tolist())) for _, ix in lists)       # a row listed twice
    assert float(gold["max_dev"]) <= R.TOL32(5, 1)                        # for the record: far inside the bound


def test_restatement_vs_recorded_reference(gold):
    for i, (d, ix) in enumerate(R.fixture_lists(gold)):
        if len(ix) == 0:
            assert gold["ref_emb"][i] == 0.0 and gold["ref_lab"][i] == 0.0
            continue
        r = R.list_diversity_ref(gold[f"G_{d}"], ix[None], gold[f"bits_{d}"])
        assert r["n_valid"][0] == len(ix)
        assert _bits_eq(r["label_div"][0], gold["ref_lab"][i]), (i, d, ix)
        assert abs(r["emb_div"][0] - gold["ref_emb"][i]) <= R.TOL32(d, int(r["pairs"][0])), (i, d, ix)


def test_restatement_semantics():
    G = np.array([[1e-9] * 4, [1e-9] * 4, [0, 0, 0, 0], [1, 0, 0, 0], [0, 2, 0, 0], [3, 0, 0, 0]], np.float32)
    bits = np.array([1, 0, 0, 6, 1 << 63, 3], np.uint64)
    idx = np.array([[1000, 1001, -1], [1003, -1, 1005], [-1, 2000, 999], [1004, -1, -1], [1003, 1004, 1002],
                    [1003, 1003, 1003]], np.int64)
    r = R.list_diversity_ref(G, idx, bits, idx_base=1000)
    assert r["n_valid"].tolist() == [2, 2, 0, 1, 3, 3]
    assert abs(r["emb_div"][0] - 0.96) <= 1e-8           # the 1e-8 clip: 4e-18 / 1e-16 (f32(1e-9) is 1e-9 (1 +- 2^-24))
    assert abs(r["emb_div"][1]) <= 1e-15                 # parallel rows
    assert r["emb_div"][2] == 0.0 and r["emb_div"][3] == 0.0 and r["emb_div"][4] == 1.0
    assert abs(r["emb_div"][5]) <= 1e-15                 # one row three times: three ordinary pairs of cosine 1
    assert r["label_div"].tolist() == [1.0, 3.0 / 2.0, 0.0, 1.0, 3.0 / 1.5, 2.0 / 2.0]
    assert not r["sim"][1][1].any() and not r["sim"][1][:, 1].any() and r["sim"][1][0, 2] == r["sim"][1][2, 0]
    assert R.list_diversity_ref(G, idx, None, 1000)["label_div"] is None


def test_host_mirrors_vs_recorded_reference(gold):
    from mmr_amd import metrics
    for i, (d, ix) in enumerate(R.fixture_lists(gold)):
        G, b = gold[f"G_{d}"], gold[f"bits_{d}"]
        emb = metrics.compute_embedding_diversity(G[ix] if len(ix) else np.array([]))
        lab = metrics.compute_label_diversity_from_labels([R.bits_to_names(x) for x in b[ix]])
        assert isinstance(emb, float) and isinstance(lab, float)
        assert _bits_eq(lab, gold["ref_lab"][i])
        pairs = len(ix) * (len(ix) - 1) // 2
        assert abs(emb - gold["ref_emb"][i]) <= R.TOL32(d, pairs), (i, d, ix)


def test_host_mirror_edge_cases():
    from mmr_amd import metrics
    one = np.ones((1, 8), np.float32)
    for e in (None, [], np.array([]), np.zeros((0, 8), np.float32), one):
        assert metrics.compute_embedding_diversity(e) == 0.0
    assert metrics.compute_embedding_diversity(np.zeros((3, 4), np.float32)) == 1.0     # zero rows: cosine 0
    assert abs(metrics.compute_embedding_diversity(np.full((2, 4), 1e-9, np.float32)) - 0.96) <= 1e-8
    for labs in (None, [], [[]], [[], []]):
        assert metrics.compute_label_diversity_from_labels(labs) == 0.0
    assert metrics.compute_label_diversity_from_labels([["a", "b"], [], ["b"]]) == 2 / 1.5


def _summary_close(got, want):
    assert list(got) == list(R.COLUMNS)
    for c, w in zip(R.COLUMNS, want):
        g = got[c]
        if math.isnan(w):
            assert math.isnan(g), (c, g)
        elif c in ("count_nonnull", "total_rows"):
            assert isinstance(g, int) and g == int(w), (c, g, w)
        else:   # a mean / std over <= 38 values of magnitude <= 8: summation order only
            assert abs(g - w) <= 64 * 2.0 ** -53 * max(1.0, abs(w)), (c, g, w)


@pytest.mark.parametrize("col", ["retrieval_diversity", "retrieval_label_diversity", "with_nan", "single", "all_nan"])
def test_diversity_summary_vs_recorded_pandas(gold, col):
    from mmr_amd import metrics
    import torch
    v, want = gold[f"col_{col}"], gold[f"summary_{col}"]
    _summary_close(metrics.diversity_summary(v), want)
    _summary_close(metrics.diversity_summary(torch.from_numpy(v)), want)
    _summary_close(metrics.diversity_summary([None if math.isnan(x) else float(x) for x in v]), want)
    _summary_close(R.summary_ref(v), want)


def test_diversity_summary_sample_std_and_empty():
    from mmr_amd import metrics
    s = metrics.diversity_summary([1.0, 2.0, 4.0, float("nan")])
    assert s["std"] == float(np.std([1.0, 2.0, 4.0], ddof=1)) and s["std"] != float(np.std([1.0, 2.0, 4.0]))
    assert (s["count_nonnull"], s["total_rows"], s["pct_missing"], s["median"]) == (3, 4, 25.0, 2.0)
    e = metrics.diversity_summary([])
    assert e["total_rows"] == 0 and e["count_nonnull"] == 0 and all(math.isnan(e[c]) for c in R.COLUMNS[:5])
    assert math.isnan(e["pct_missing"])


def test_loader_has_the_prototypes():
    from mmr_amd import _lib
    sig = _lib.SIGNATURES["mmr_index_list_diversity"]
    assert len(sig) == 11 and sig[2] is ctypes.c_int64 and sig[3] is ctypes.c_int32
    assert _lib.SIGNATURES["mmr_index_list_diversity_work_bytes"] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32]
    assert _lib._RESTYPES["mmr_index_list_diversity_work_bytes"] is ctypes.c_int64
    assert _lib.ABI_VERSION == 2                       # an additive change
    L = _lib.lib()
    assert L.mmr_index_list_diversity.argtypes == sig and L.mmr_version() == 2


def test_capi_argument_checks():
    """mmr_index_list_diversity rejects broken limits and NULL pointers before the index or the device is touched
    (the index handle here is a dummy that must never be dereferenced)."""
    from mmr_amd import _lib
    L = _lib.lib()
    wb = L.mmr_index_list_diversity_work_bytes
    assert wb(None, 256, 5) == 0 and wb(None, 256, 16) == 0 and wb(None, 0, 64) == 0 and wb(None, 4, 257) == 0
    assert wb(None, 7, 17) >= 7 * 3 * 8 and wb(None, 7, 256) >= 7 * 136 * 8 and wb(None, 7, 256) % 16 == 0
    p = ctypes.c_void_p(256)

    def call(index=p, idx=p, nq=4, k=5, g_labels=None, out_emb=p, out_lab=None, work=None):
        return L.mmr_index_list_diversity(index, idx, nq, k, g_labels, out_emb, out_lab, None, None, work, None)
    for kw, msg in ((dict(index=None), b"index is NULL"), (dict(k=0), b"k=0 outside"), (dict(k=257), b"k=257 outside"),
                    (dict(nq=-1), b"nq < 0"), (dict(idx=None), b"NULL idx"), (dict(out_emb=None), b"NULL idx / out_emb"),
                    (dict(g_labels=p), b"both NULL or both set"), (dict(out_lab=p), b"both NULL or both set"),
                    (dict(k=17), b"needs work"), (dict(k=17, work=ctypes.c_void_p(264)), b"16-B aligned")):
        assert call(**kw) == 1 and msg in L.mmr_last_error(), (kw, L.mmr_last_error())
    assert call(nq=0) == 0 and call(nq=0, idx=None, out_emb=None) == 0       # nothing to do, nothing touched
