"""GPU: retrieval diversity of retrieved lists (mmr_index_list_diversity, csrc/list_div.hip) through
GalleryIndex.list_diversity and the engines' diversity(), against the f64 restatement of list_div_ref.py and the
reference's recorded values (tests/golden/list_diversity.npz).

The bar (derived in list_div_ref.py): n_valid identical, label diversity bit-equal, embedding diversity and the
cosines of `sim` within TOL64(d, P) = 2 (d + 4 + P) 2^-53 absolute of the restatement (P = the list's valid pairs,
0 for a cosine); against the reference, which works in f32, TOL32(d, P) = (d + 4 + P) 2^-24.

Shapes: galleries of 300 rows (2000 x 64 for the engines); k on both sides of every 16-row tile edge and of the
one-wave / tiled switch (16 | 17), the largest list (256); d below one k step (5), zero-padded (100), 768 and 1024;
one list, a few, and more lists than fit one of anything (65, 70)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import list_div_ref as R
from conftest import GOLDEN
from mmr_amd import _lib, metrics, synthetic
from mmr_amd.retrieval import DLSRetrievalEngine, GalleryIndex, MI355XRetrievalEngine, drop_excluded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 300
KS = (1, 2, 3, 5, 15, 16, 17, 33, 64, 256)


def _gallery(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _bits(n, seed, empty_every=7):
    """1-3 of 64 labels per row, bit 63 on every 5th row, no labels on every `empty_every`-th."""
    rng = np.random.default_rng(seed)
    b = np.zeros(n, np.uint64)
    for i in range(n):
        for j in rng.choice(64, size=int(rng.integers(1, 4)), replace=False):
            b[i] |= np.uint64(1) << np.uint64(j)
    b[::5] |= np.uint64(1) << np.uint64(63)
    b[::empty_every] = 0
    return b


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(ix, G, idx, bits=None, idx_base=0):
    """One list_diversity call against the restatement at the bar of this file; -> (outputs as numpy, restatement)."""
    emb, lab, nv, sim = ix.list_diversity(_dev(idx), bits, want_sim=True)
    emb, nv, sim = emb.cpu().numpy(), nv.cpu().numpy(), sim.cpu().numpy()
    r = R.list_diversity_ref(G, idx, bits, idx_base)
    d = G.shape[1]
    assert emb.dtype == np.float64 and nv.dtype == np.int32 and sim.shape == idx.shape + (idx.shape[1],)
    np.testing.assert_array_equal(nv, r["n_valid"])
    if bits is None:
        assert lab is None
    else:
        lab = lab.cpu().numpy()
        assert np.array_equal(lab.view(np.int64), r["label_div"].view(np.int64)), (lab, r["label_div"])
    e_emb = np.abs(emb - r["emb_div"])
    e_sim = np.abs(sim - r["sim"]).max() if sim.size else 0.0
    tol = np.array([R.TOL64(d, int(p)) for p in r["pairs"]])
    print(f"d={d} k={idx.shape[1]} nq={idx.shape[0]}: max |emb - ref| = {e_emb.max():.3e} (bound "
          f"{tol[e_emb.argmax()]:.3e}), max |sim - ref| = {e_sim:.3e} (bound {R.TOL64(d):.3e})")
    assert np.all(e_emb <= tol), (e_emb.max(), tol.min())
    assert e_sim <= R.TOL64(d)
    assert np.array_equal(sim.view(np.int64), sim.transpose(0, 2, 1).view(np.int64)), "sim is not bitwise symmetric"
    bad = ~((idx >= idx_base) & (idx < idx_base + G.shape[0]))
    assert not sim[bad].any() and not sim.transpose(0, 2, 1)[bad].any(), "a skipped entry has a nonzero row / column"
    for q in range(len(idx)):        # the diversity again from the device's own cosines
        pos = np.nonzero(~bad[q])[0]
        if len(pos) >= 2:
            s = sim[q][np.ix_(pos, pos)][np.triu_indices(len(pos), k=1)]
            assert abs(emb[q] - (1.0 - s.sum() / len(s))) <= R.TOL64(d, len(s))
        else:
            assert emb[q] == 0.0
    return (emb, lab, nv, sim), r


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "list_diversity.npz"))


def test_golden_reference_values(gold):
    lists = R.fixture_lists(gold)
    for d in sorted({d for d, _ in lists}):
        sel = [i for i, (dd, _) in enumerate(lists) if dd == d]
        G, bits = gold[f"G_{d}"], gold[f"bits_{d}"]
        k = max(1, max(len(lists[i][1]) for i in sel))
        idx = np.full((len(sel), k), -1, np.int64)        # shorter lists (K = 0 too) padded as a walk pads them
        for row, i in enumerate(sel):
            idx[row, :len(lists[i][1])] = lists[i][1]
        ix = GalleryIndex(G, device=0)
        (emb, lab, nv, _), r = _check(ix, G, idx, bits)
        ix.close()
        assert np.array_equal(lab.view(np.int64), gold["ref_lab"][sel].view(np.int64))
        err = np.abs(emb - gold["ref_emb"][sel])
        tol = np.array([R.TOL32(d, int(p)) for p in r["pairs"]])
        print(f"d={d}: max |emb - reference| = {err.max():.3e}")
        assert np.all(err <= tol), (d, err.max())
        assert nv.tolist() == [len(lists[i][1]) for i in sel]


@pytest.mark.parametrize("d", [5, 100, 768, 1024])
def test_grid(d):
    G, bits = _gallery(N, d, 100 + d), _bits(N, 200 + d)
    ix = GalleryIndex(G, device=0)
    rng = np.random.default_rng(300 + d)
    dup = False
    for k in KS:
        for nq in (1, 7, 65):
            idx = rng.integers(0, N, size=(nq, k))          # with replacement: rows repeat within a list
            dup |= any(len(set(row.tolist())) < k for row in idx)
            _check(ix, G, idx, bits)
    assert dup
    ix.close()


@pytest.mark.parametrize("k", [5, 16, 17, 40])
def test_invalid_entries(k):
    d = 100
    G, bits = _gallery(N, d, 11), _bits(N, 12)
    rng = np.random.default_rng(13 + k)
    idx = rng.integers(0, N, size=(9, k))
    idx[0, 0] = -1                                           # head
    idx[1, k // 2] = -1                                      # middle
    idx[2, k - 1] = -1                                       # tail
    idx[3, ::2] = N                                          # first index past the gallery
    far = [2 ** 40, -2 ** 62, np.iinfo(np.int64).min, np.iinfo(np.int64).max]                # garbage, both signs
    idx[4, 1::2] = np.resize(np.array(far, np.int64), len(idx[4, 1::2]))
    idx[5, :] = -1                                           # nothing valid
    idx[6, :] = -1
    idx[6, k - 1] = 17                                       # one valid entry
    idx[7, :] = [-1, N + 5][k % 2]
    idx[7, 0] = N - 1                                        # the last row, alone
    ix = GalleryIndex(G, device=0)
    (emb, lab, nv, _), _ = _check(ix, G, idx, bits)
    assert nv[5] == 0 and emb[5] == 0.0 and lab[5] == 0.0
    assert nv[6] == 1 and emb[6] == 0.0 and nv[7] == 1 and emb[7] == 0.0
    ix.close()


@pytest.mark.parametrize("k", [5, 33])
def test_idx_base(k):
    d = 100
    G, bits = _gallery(N, d, 21), _bits(N, 22)
    idx = np.random.default_rng(23).integers(0, N, size=(7, k))
    idx[0, 1] = -1
    idx[1, 0] = N                                            # local N: global 1000 + N is out, global N is below the base
    a, b = GalleryIndex(G, device=0), GalleryIndex(G, device=0, idx_base=1000)
    (e0, l0, v0, s0), _ = _check(a, G, idx, bits)
    shifted = np.where((idx >= 0) & (idx < N), idx + 1000, idx)
    (e1, l1, v1, s1), _ = _check(b, G, shifted, bits, idx_base=1000)
    for x, y in ((e0, e1), (l0, l1), (s0, s1)):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    assert np.array_equal(v0, v1)
    # indices below the base are skipped: the unshifted lists hold nothing for the based index
    (_, _, v2, _), _ = _check(b, G, np.where(idx == N, 0, idx), bits, idx_base=1000)
    assert not v2.any()
    a.close()
    b.close()


@pytest.mark.parametrize("k", [4, 20])
def test_norm_edge_cases(k):
    d = 4
    G = _gallery(40, d, 31)
    G[0:3] = 0.0                                             # zero rows
    G[3:6] = np.float32(1e-9)                                # |g| = 2e-9, below the 1e-8 clip
    G[7] = G[6]                                              # byte-identical rows under two indices
    rng = np.random.default_rng(32)
    idx = np.full((6, k), -1, np.int64)
    idx[0, :2] = [3, 4]                                      # the clip alone: 1 - 4e-18 / 1e-16
    idx[1] = rng.integers(0, 12, size=k)                     # zero, tiny and ordinary rows mixed
    idx[2] = 9                                               # one row k times
    idx[3, :2] = [6, 7]
    idx[4, :3] = [0, 1, 2]                                   # zero rows only: cosines 0, diversity 1
    idx[5] = rng.integers(0, 40, size=k)
    ix = GalleryIndex(G, device=0, mode="x3")
    (emb, _, nv, sim), _ = _check(ix, G, idx)
    assert abs(emb[0] - 0.96) <= 1e-8 and nv[0] == 2         # f32(1e-9) = 1e-9 (1 +- 2^-24)
    pairs = k * (k - 1) // 2
    assert nv[2] == k and abs(emb[2]) <= R.TOL64(d, pairs)
    assert abs(emb[3]) <= R.TOL64(d, 1) and sim[3, 0, 0] == sim[3, 1, 1] == sim[3, 0, 1]
    assert emb[4] == 1.0 and not sim[4].any()
    ix.close()


@pytest.mark.parametrize("d", [100, 768])
def test_native_fp16_index(d):
    Gh = _gallery(N, d, 41 + d).astype(np.float16)
    bits = _bits(N, 42)
    ix = GalleryIndex(Gh, device=0)
    assert ix.native_f16
    rng = np.random.default_rng(43)
    for k in (5, 16, 17, 64, 256):
        idx = rng.integers(0, N, size=(7, k))
        idx[1, k // 2] = -1
        _check(ix, Gh.astype(np.float32), idx, bits)
    ix.close()


def test_labels():
    d = 5
    G = _gallery(N, d, 51)
    ix = GalleryIndex(G, device=0)
    rng = np.random.default_rng(52)
    b43 = (rng.integers(0, 2 ** 43, size=N, dtype=np.uint64))
    b64 = _bits(N, 53, empty_every=3)
    b64[4], b64[8] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1) << np.uint64(63)
    assert (b64 >> np.uint64(63)).any() and (b64 == 0).any()
    for k in (5, 40):
        idx = rng.integers(0, N, size=(9, k))
        idx[0, :3] = [4, 8, 3]                               # all 64 labels, bit 63 alone, no labels
        idx[1, 1] = -1
        for bits in (b43, b64):
            _check(ix, G, idx, bits)
        # the same through each accepted carrier of the bitsets
        want = R.list_diversity_ref(G, idx, b64)["label_div"]
        for carrier in (b64, b64.view(np.int64), torch.from_numpy(b64.view(np.int64)), _dev(b64.view(np.int64))):
            got = ix.list_diversity(_dev(idx), carrier)[1].cpu().numpy()
            assert np.array_equal(got.view(np.int64), want.view(np.int64))
        (_, lab0, _, _), _ = _check(ix, G, idx, np.zeros(N, np.uint64))
        assert not lab0.any()                                # only empty sets: 0.0
        assert ix.list_diversity(_dev(idx))[1] is None       # no bitsets: no label diversity
    ix.close()


@pytest.mark.parametrize("k", [5, 40])
def test_slot_independence_and_determinism(k):
    d = 100
    G, bits = _gallery(N, d, 61), _bits(N, 62)
    ix = GalleryIndex(G, device=0)
    rng = np.random.default_rng(63 + k)
    idx = rng.integers(0, N, size=(70, k))
    idx[::6, 1] = -1
    one = rng.integers(0, N, size=k)
    one[k // 2] = -1
    for slot in (0, 3, 69):
        idx[slot] = one
    run = lambda t: ix.list_diversity(_dev(t), bits, want_sim=True)     # noqa: E731
    a, b, alone = run(idx), run(idx), run(one[None])
    for x, y in zip(a, b):                                   # the whole call twice: identical bytes
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                           y.view(torch.int64) if y.dtype == torch.float64 else y)
    for slot in (0, 3, 69):
        for x, y in zip(a, alone):
            xs, ys = x[slot].cpu().numpy(), y[0].cpu().numpy()
            assert xs.tobytes() == ys.tobytes(), slot
    ix.close()


@pytest.mark.parametrize("k", [5, 40])
def test_guards_and_optional_outputs(k):
    """Every output with sentinel rows before and after, out_sim / out_lab / out_valid NULL in turn."""
    d, nq, pad = 100, 7, 3
    G, bits = _gallery(N, d, 71), _bits(N, 72)
    ix = GalleryIndex(G, device=0)
    L = _lib.lib()
    idx = np.random.default_rng(73).integers(0, N, size=(nq, k))
    idx[2, 0] = -1
    r = R.list_diversity_ref(G, idx, bits)
    t_idx, t_bits = _dev(idx), _dev(bits.view(np.int64))
    nbytes = int(L.mmr_index_list_diversity_work_bytes(ix._h, nq, k))
    assert (nbytes == 0) == (k <= 16)
    SENT_F, SENT_I = -12345.5, -77
    for skip in (None, "sim", "lab", "valid"):
        emb = torch.full((nq + 2 * pad,), SENT_F, dtype=torch.float64, device=DEV)
        lab = torch.full((nq + 2 * pad,), SENT_F, dtype=torch.float64, device=DEV)
        val = torch.full((nq + 2 * pad,), SENT_I, dtype=torch.int32, device=DEV)
        sim = torch.full((nq + 2 * pad, k, k), SENT_F, dtype=torch.float64, device=DEV)
        work = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device=DEV)
        p = lambda t, on=True: _lib.ptr(t[pad:]) if on else ctypes.c_void_p(0)    # noqa: E731
        _lib.check(L.mmr_index_list_diversity(
            ix._h, _lib.ptr(t_idx), nq, k, _lib.ptr(t_bits) if skip != "lab" else None, p(emb), p(lab, skip != "lab"),
            p(val, skip != "valid"), p(sim, skip != "sim"), _lib.ptr(work[256:]) if nbytes else None,
            _lib.stream_ptr(torch.device(DEV))), "mmr_index_list_diversity")
        torch.cuda.synchronize()
        for t, s, on in ((emb, SENT_F, True), (lab, SENT_F, skip != "lab"), (val, SENT_I, skip != "valid"),
                         (sim, SENT_F, skip != "sim")):
            assert bool((t[:pad] == s).all()) and bool((t[nq + pad:] == s).all()), f"sentinel overwritten ({skip})"
            assert bool((t[pad:nq + pad] != s).all()) == on, f"output written / not written ({skip})"
        assert bool((work[:256] == 0x5A).all()) and bool((work[256 + nbytes:] == 0x5A).all())
        tol = np.array([R.TOL64(d, int(x)) for x in r["pairs"]])
        assert np.all(np.abs(emb[pad:nq + pad].cpu().numpy() - r["emb_div"]) <= tol)
        if skip != "lab":
            assert np.array_equal(lab[pad:nq + pad].cpu().numpy().view(np.int64), r["label_div"].view(np.int64))
        if skip != "valid":
            assert np.array_equal(val[pad:nq + pad].cpu().numpy(), r["n_valid"])
    ix.close()


def test_no_lists():
    ix = GalleryIndex(_gallery(N, 5, 81), device=0)
    for k in (5, 40):
        emb, lab, nv, sim = ix.list_diversity(torch.empty((0, k), dtype=torch.int64, device=DEV), _bits(N, 82),
                                              want_sim=True)
        assert emb.shape == (0,) and lab.shape == (0,) and nv.shape == (0,) and sim.shape == (0, k, k)
        assert emb.dtype == torch.float64 and nv.dtype == torch.int32
    ix.close()


def test_python_errors():
    ix = GalleryIndex(_gallery(N, 5, 91), device=0)
    good = torch.zeros((3, 5), dtype=torch.int64, device=DEV)
    for bad in (good.to(torch.int32), good.cpu(), good[0], torch.zeros((3, 0), dtype=torch.int64, device=DEV),
                torch.zeros((3, 257), dtype=torch.int64, device=DEV), good.cpu().numpy()):
        with pytest.raises(ValueError):
            ix.list_diversity(bad)
    with pytest.raises(ValueError, match="label bitsets"):
        ix.list_diversity(good, np.zeros(N + 1, np.uint64))
    assert ix.list_diversity(good)[2].tolist() == [5, 5, 5]
    ix.close()


# ---------------------------------------------------------------------------------------------- engines
EN, ED, EB = 2000, 64, 33
KEYS = {"retrieval_diversity", "retrieval_label_diversity", "n_valid", "summary"}


@pytest.fixture(scope="module")
def labelled():
    G, gl = synthetic.labelled_gallery(EN, ED, synthetic.SEED + 70)
    Q, _ = synthetic.labelled_gallery(EB, ED, synthetic.SEED + 71)
    return G, synthetic.labels_to_bits(gl), Q


def _same(out, emb, lab, nv):
    assert torch.equal(out["retrieval_diversity"].view(torch.int64), emb.view(torch.int64))
    assert torch.equal(out["n_valid"], nv)
    if lab is None:
        assert out["retrieval_label_diversity"] is None and set(out["summary"]) == {"retrieval_diversity"}
    else:
        assert torch.equal(out["retrieval_label_diversity"].view(torch.int64), lab.view(torch.int64))
    for name, t in (("retrieval_diversity", emb), ("retrieval_label_diversity", lab)):
        if t is not None:
            want, got = metrics.diversity_summary(t), out["summary"][name]
            assert list(got) == list(R.COLUMNS)
            assert all(got[c] == want[c] or (np.isnan(got[c]) and np.isnan(want[c])) for c in R.COLUMNS)


def test_exact_engine_diversity(labelled):
    G, gb, Q = labelled
    eng = MI355XRetrievalEngine(embs=G, ids=[f"r{i}" for i in range(EN)])
    for K in (5, 10, 20):
        out = eng.diversity(Q, K=K, gallery_bits=gb, return_lists=True)
        assert set(out) == KEYS | {"idx", "scores"}
        idx, sc = eng.search(torch.from_numpy(Q), K)
        assert torch.equal(out["idx"], idx) and torch.equal(out["scores"], sc)
        _same(out, *eng.index.list_diversity(idx, gb))
        assert int(out["n_valid"].min()) == K
        r = R.list_diversity_ref(G, idx.cpu().numpy(), gb)
        assert np.all(np.abs(out["retrieval_diversity"].cpu().numpy() - r["emb_div"]) <= R.TOL64(ED, K * (K - 1) // 2))
    plain = eng.diversity(Q, K=5)
    assert set(plain) == KEYS
    _same(plain, *eng.index.list_diversity(eng.search(torch.from_numpy(Q), 5)[0]))
    # test -> test protocol: the queries are gallery rows, each excluded from its own list
    rows = np.arange(0, 3 * EB, 3)
    ex = eng.diversity(G[rows], K=5, gallery_bits=gb, exclude_ids=rows, return_lists=True)
    assert ex["idx"].shape == (EB, 5) and not bool((ex["idx"].cpu() == torch.from_numpy(rows)[:, None]).any())
    wide, wsc = eng.search(torch.from_numpy(G[rows]), 6)
    assert bool((wide[:, 0].cpu() == torch.from_numpy(rows)).all())          # each query finds itself first
    assert torch.equal(ex["idx"], drop_excluded(wide, torch.from_numpy(rows))) and torch.equal(ex["scores"], wsc[:, 1:])
    _same(ex, *eng.index.list_diversity(ex["idx"], gb))
    by_id = eng.diversity(G[rows], K=5, gallery_bits=gb, exclude_ids=[f"r{i}" for i in rows], return_lists=True)
    assert torch.equal(by_id["idx"], ex["idx"])
    eng.close()


def test_dls_engine_diversity(labelled):
    G, gb, Q = labelled
    eng = DLSRetrievalEngine(embs=G, ids=[str(i) for i in range(EN)], link_threshold=0.5, max_links=10)
    out = eng.diversity(Q, K=5, gallery_bits=gb, return_lists=True, seed=7)
    idx, sc = eng.retrieve_batch(torch.from_numpy(Q), 5, seed=7)
    assert set(out) == KEYS | {"idx", "scores"}
    assert torch.equal(out["idx"], idx) and torch.equal(out["scores"], sc)
    _same(out, *eng.index.list_diversity(idx, gb))
    # a graph so sparse that walks end with fewer than K rows: only every third row has links, seeds without one
    eng.link_graph = [[i + 1, i + 2] if i % 3 == 0 and i + 2 < EN else [] for i in range(EN)]
    seeds = np.stack([np.array([1, 2, 4]) + 3 * b for b in range(EB)])
    seeds[1] = [0, 3, 6]                                      # these link on: the first pop leaves 4 rows
    out = eng.diversity(Q, K=5, gallery_bits=gb, return_lists=True, seeds=seeds, seed_size=3)
    idx, _ = eng.retrieve_batch(torch.from_numpy(Q), 5, seeds=seeds, seed_size=3)
    assert torch.equal(out["idx"], idx) and bool((idx[0] < 0).any())
    # a walk whose seeds have no links pops its best row and stops: 2 rows are left of 3
    assert out["n_valid"].tolist() == (idx >= 0).sum(1).tolist() and out["n_valid"][0] == 2 and out["n_valid"][1] > 2
    _same(out, *eng.index.list_diversity(idx, gb))
    r = R.list_diversity_ref(G, idx.cpu().numpy(), gb)
    assert np.all(np.abs(out["retrieval_diversity"].cpu().numpy() - r["emb_div"]) <= R.TOL64(ED, 10))
    assert np.array_equal(out["retrieval_label_diversity"].cpu().numpy().view(np.int64), r["label_div"].view(np.int64))
    # exact=True is the exact engine's path
    a = eng.diversity(Q, K=5, gallery_bits=gb, exact=True, return_lists=True)
    b = MI355XRetrievalEngine.diversity(eng, Q, K=5, gallery_bits=gb, return_lists=True)
    assert torch.equal(a["idx"], b["idx"]) and torch.equal(a["idx"], eng.search(torch.from_numpy(Q), 5)[0])
    _same(a, b["retrieval_diversity"], b["retrieval_label_diversity"], b["n_valid"])
    eng.close()
