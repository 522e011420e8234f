"""GPU: the batched DLS walk on device (mmr_index_dls_walk, GalleryIndex.dls_walk,
DLSRetrievalEngine.retrieve_batch) against the reference's recorded walks (tests/golden/dls_rerank.npz) and the
f64 set-algorithm restatement (tests/dls_walk_ref.py, itself checked against the reference's heap walk in
test_dls_walk_cpu.py).

Bars: index lists, step counts and visited counts identical; score64 within 1e-12 absolute of the restatement (an
f64 reordering of <= 1024 terms of magnitude <= 1 stays far below that); the f32 score is the rounded score64;
recorded f32 scores within 1e-6 (the host-walk test's tolerance; the expression in f64 differs by 1.4e-7)."""
import os

import numpy as np
import pytest
import torch

import mmr_amd
from mmr_amd import _lib, synthetic
from mmr_amd.retrieval import GalleryIndex

from conftest import GOLDEN
from dls_walk_ref import walk_batch
from test_dls_walk_cpu import PARAMS, ref_seeds
from test_oracle_dls import graph_from

pytestmark = pytest.mark.gpu


def table(graph, width=None):
    width = width or max(1, max(len(x) for x in graph))
    t = np.full((len(graph), width), -1, np.int64)
    for i, x in enumerate(graph):
        t[i, :len(x)] = x
    return t


def device_walk(ix, Q, nbr, seeds, k, max_steps=100, r=None):
    out = ix.dls_walk(torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda(), torch.from_numpy(nbr).cuda(),
                      torch.from_numpy(np.ascontiguousarray(seeds, np.int64)).cuda(), k, max_steps=max_steps, r=r,
                      want_f64=True, want_stats=True)
    return tuple(t.cpu().numpy() for t in out)


def assert_matches_ref(G, nbr, Q, seeds, k, max_steps, r, got, base=0):
    idx, sc, sc64, steps, vis = got
    ri, rs, rst, rvis = walk_batch(G, nbr, Q, seeds, k, max_steps, r)
    live = ri >= 0
    assert np.array_equal(idx, np.where(live, ri + base, -1)), (idx, ri)
    assert np.array_equal(steps, rst) and np.array_equal(vis, rvis)
    assert np.all(sc64[~live] == -np.inf) and np.all(sc[~live] == -np.inf)
    err = np.abs(sc64[live] - rs[live]).max() if live.any() else 0.0
    print(f"k={k} r={r} max_steps={max_steps}: max |score64 - ref| = {err:.3e}, padded slots {int((~live).sum())}")
    assert err <= 1e-12
    assert np.array_equal(sc[live], sc64[live].astype(np.float32))
    return ri


@pytest.fixture(scope="module")
def fx():
    f = np.load(os.path.join(GOLDEN, "dls_rerank.npz"), allow_pickle=False)
    G, _ = synthetic.dls_gallery()
    Qm, _ = synthetic.labelled_gallery(synthetic.DLS_Q, synthetic.DLS_D, synthetic.SEED + 12)
    graph = graph_from(f, "t50_m10")
    ix = GalleryIndex(G)
    yield f, G, graph, table(graph), Qm, ix
    ix.close()


def golden_seeds(n, seed_size):
    return np.stack([ref_seeds(n, seed_size, synthetic.SEED + qi) for qi in range(synthetic.DLS_Q)])


def test_golden_walks(fx):
    f, G, _, nbr, Qm, ix = fx
    idx, sc, *_ = device_walk(ix, Qm, nbr, golden_seeds(len(G), 5), 5)
    assert np.array_equal(idx, f["walk_idx"])
    err = np.abs(sc.astype(np.float64) - f["walk_score"]).max()
    print(f"max |score - recorded| = {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("K,seed_size,max_steps,cm", PARAMS)
def test_parameter_grid(fx, K, seed_size, max_steps, cm):
    """Covers the max_steps cut-off (4 steps), truncation at every step (r = 1) and K larger than the set."""
    f, G, _, nbr, Qm, ix = fx
    seeds, r = golden_seeds(len(G), seed_size), max(cm * K, seed_size)
    got = device_walk(ix, Qm, nbr, seeds, K, max_steps, r)
    ri = assert_matches_ref(G, nbr, Qm, seeds, K, max_steps, r, got)
    if K == 50:
        assert (ri < 0).any()      # the -1 / -inf padding is exercised
    if max_steps == 4:
        assert got[3].max() == 4   # ... and the step cut-off


def own_graph(ix, thr, ml):
    nbr, _ = ix.link_graph(thr, ml)
    return nbr.cpu().numpy()


def shape_case(n, d, thr, ml, nq, k, seed_size, zero_dup=False, idx_base=0, max_steps=100, r=None, gseed=41):
    G, _ = synthetic.labelled_gallery(n, d, gseed)
    if zero_dup:
        G[17] = 0.0
        G[100] = G[99]
    Q, _ = synthetic.labelled_gallery(nq, d, gseed + 2)
    ix = GalleryIndex(G, idx_base=idx_base)
    nbr = own_graph(ix, thr, ml)
    seeds = np.stack([ref_seeds(n, seed_size, 7 + i) for i in range(nq)])
    if zero_dup:
        seeds[0, 0], seeds[1, :2] = 17, (99, 100)  # a zero-row seed; the duplicate pair as seeds
        seeds[0, 1:] = [x if x != 17 else 18 for x in seeds[0, 1:]]
    r = max(10 * k, seed_size) if r is None else r
    got = device_walk(ix, Q, nbr, seeds, k, max_steps, r)
    assert_matches_ref(G, nbr, Q, seeds, k, max_steps, r, got, base=idx_base)
    ix.close()
    return got


def test_shape_6000x96_own_graph():
    shape_case(6000, 96, 0.4, 12, 33, 5, 5, zero_dup=True, gseed=31)


@pytest.mark.parametrize("n,d,thr,ml", [(300, 768, 0.3, 8), (300, 8, 0.6, 8), (300, 300, 0.3, 6)])
def test_shape_small(n, d, thr, ml):
    shape_case(n, d, thr, ml, 6, 5, 5)


@pytest.mark.parametrize("d", [512, 1024])
def test_shape_wide_rows_32_links_many_seeds(d):
    """max_links = 32 (a second row batch per step), 40 seeds (two seed rounds), d = 1024 (8-row batches)."""
    got = shape_case(400, d, 0.1, 32, 6, 8, 40, r=96)
    assert got[3].max() >= 1 and got[4].max() > 40


def test_shape_three_rows():
    G, _ = synthetic.labelled_gallery(3, 32, 5)
    Q, _ = synthetic.labelled_gallery(4, 32, 6)
    ix = GalleryIndex(G)
    nbr = table([[1, 2], [0], [0, 1]])
    seeds = np.stack([ref_seeds(3, 5, i) for i in range(4)])       # min(seed_size, N) = 3 seeds
    assert seeds.shape == (4, 3)
    got = device_walk(ix, Q, nbr, seeds, 5, 100, 50)
    ri = assert_matches_ref(G, nbr, Q, seeds, 5, 100, 50, got)
    assert ((ri >= 0).sum(1) == 2).all() and (got[4] == 3).all()   # all three visited; the popped best is gone
    ix.close()


def test_shape_idx_base():
    shape_case(300, 64, 0.3, 8, 5, 5, 5, idx_base=1000)


def hand_built():
    rng = np.random.default_rng(7)
    G = rng.standard_normal((12, 16)).astype(np.float32)
    q = rng.standard_normal(16).astype(np.float32)
    G[0] = 0.0
    G[1] = q
    G[3] = G[7] = G[9] = (0.9 * q + 0.3 * rng.standard_normal(16)).astype(np.float32)
    # -1 in the middle, an entry >= n, a self-loop (row 0); a row listed twice (row 3); rows with no links
    graph = [[1, -1, 3, 50, 0], [7, 9, 3], [1, 3, 7, 9], [4, 4, 5], [], [6, 11], [8], [], [10], [], [2], []]
    return G, q, table(graph)


@pytest.mark.parametrize("seeds,k,max_steps,r", [([2, 2, 2], 3, 1, 30), ([2, 2, 2], 2, 1, 30), ([2, 2, 2], 3, 1, 3),
                                                 ([0, 0, 2], 3, 100, 30), ([5, 5, 0], 4, 100, 40),
                                                 ([0, -1, 99], 12, 100, 120), ([10, 6, 5], 5, 2, 5)])
def test_hand_built_graph_and_ties(seeds, k, max_steps, r):
    G, q, nbr = hand_built()
    ix = GalleryIndex(G)
    Q = np.stack([q, np.zeros_like(q), -q])          # an all-zero query: every score ties at 0
    S = np.tile(np.array(seeds, np.int64), (3, 1))
    got = device_walk(ix, Q, nbr, S, k, max_steps, r)
    assert_matches_ref(G, nbr, Q, S, k, max_steps, r, got)
    if seeds == [2, 2, 2] and k == 3 and max_steps == 1:
        # one step from row 2 leaves {1, 3, 7, 9}; 3, 7, 9 are identical: the tie keeps 3 and 7, printed high to low
        assert got[0][0].tolist() == [1, 7, 3]
        assert got[2][0, 1] == got[2][0, 2]             # bit-identical scores of byte-identical rows
    ix.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_slot_independence(fx):
    f, G, _, nbr, Qm, ix = fx
    seeds24 = golden_seeds(len(G), 5)
    base = device_walk(ix, Qm, nbr, seeds24, 5)
    Q = np.tile(Qm, (9, 1))[:201].copy()
    S = np.tile(seeds24, (9, 1))[:201].copy()
    slots = [0, 1, 63, 64, 200]
    Q[slots], S[slots] = Qm[7], seeds24[7]
    idx, sc, sc64, steps, vis = device_walk(ix, Q, nbr, S, 5)
    for s in slots:
        assert np.array_equal(idx[s], base[0][7]) and np.array_equal(bits(sc64[s]), bits(base[2][7]))
        assert steps[s] == base[3][7] and vis[s] == base[4][7]
    assert np.array_equal(idx[2], base[0][2])            # the other slots still hold their own walks
    for qi in (0, 7, 23):                                # a B = 1 call equals its row of the B = 24 call
        one = device_walk(ix, Qm[qi:qi + 1], nbr, seeds24[qi:qi + 1], 5)
        assert np.array_equal(one[0][0], base[0][qi]) and np.array_equal(bits(one[2][0]), bits(base[2][qi]))
        assert np.array_equal(one[1][0], base[1][qi]) and one[3][0] == base[3][qi] and one[4][0] == base[4][qi]


def test_guard_rows_untouched(fx):
    f, G, _, nbr, Qm, ix = fx
    B, k = 24, 7
    dev = "cuda"
    q = torch.from_numpy(Qm).to(dev)
    nb = torch.from_numpy(nbr).to(dev)
    sd = torch.from_numpy(golden_seeds(len(G), 5)).to(dev)
    oi = torch.full((B + 2, k), 12345, dtype=torch.int64, device=dev)
    os_ = torch.full((B + 2, k), 7.5, dtype=torch.float32, device=dev)
    o64 = torch.full((B + 2, k), 7.5, dtype=torch.float64, device=dev)
    st = torch.full((B + 2,), 77, dtype=torch.int32, device=dev)
    vi = torch.full((B + 2,), 77, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().mmr_index_dls_walk(ix._h, _lib.ptr(q), B, _lib.ptr(nb), nb.shape[1], _lib.ptr(sd), 5, k, 100,
                                             70, _lib.ptr(oi[1:]), _lib.ptr(os_[1:]), _lib.ptr(o64[1:]),
                                             _lib.ptr(st[1:]), _lib.ptr(vi[1:]), _lib.stream_ptr(q.device)), "walk")
    torch.cuda.synchronize()
    for t, g in ((oi, 12345), (os_, 7.5), (o64, 7.5), (st, 77), (vi, 77)):
        assert (t[0] == g).all() and (t[-1] == g).all()
        assert not (t[1:-1] == g).any()
    ref = device_walk(ix, Qm, nbr, golden_seeds(len(G), 5), k, 100, 70)
    assert np.array_equal(oi[1:-1].cpu().numpy(), ref[0])


def test_engine_retrieve_batch(fx):
    f, G, ref_graph, _, Qm, _ = fx
    ids = [f"r{i}" for i in range(len(G))]
    eng = mmr_amd.DLSRetrievalEngine(embs=G, ids=ids, link_threshold=0.5, max_links=10)
    own = eng.link_graph
    assert eng._nbr_cache[0] is own                      # the built table stays on the device
    assert eng._device_graph() is eng._nbr_cache[1]
    eng.link_graph = ref_graph
    sl = [synthetic.SEED + qi for qi in range(synthetic.DLS_Q)]
    idx, sc = eng.retrieve_batch(Qm, K=5, seed=sl)
    assert isinstance(idx, np.ndarray) and idx.dtype == np.int64 and sc.dtype == np.float32 and idx.shape == (24, 5)
    for qi in range(synthetic.DLS_Q):
        h_ids, h_sc = eng.retrieve(Qm[qi], K=5, seed=sl[qi])
        assert [ids[i] for i in idx[qi]] == h_ids
        np.testing.assert_allclose(sc[qi], h_sc, rtol=0, atol=1e-6)
    assert np.array_equal(idx, f["walk_idx"])
    ti, ts, tst, tvis = eng.retrieve_batch(torch.from_numpy(Qm).cuda(), K=5, seed=sl, return_stats=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (ti, ts, tst, tvis))
    assert np.array_equal(ti.cpu().numpy(), idx) and int(tst.min()) >= 0 and int(tvis.min()) >= 5
    # query_ids: the host path's (process-salted) seeds
    qids = [f"query-{qi}" for qi in range(synthetic.DLS_Q)]
    bi, _ = eng.retrieve_batch(Qm, K=5, query_ids=qids)
    for qi in (0, 5, 23):
        assert [ids[i] for i in bi[qi]] == eng.retrieve(Qm[qi], K=5, query_id=qids[qi])[0]
    # explicit seeds; then another graph takes effect
    seeds = np.stack([ref_seeds(len(G), 5, s) for s in sl])
    ei, _ = eng.retrieve_batch(Qm, K=5, seeds=seeds)
    assert np.array_equal(ei, idx)
    other = graph_from(f, "t30_m8")
    eng.link_graph = other
    oi, _ = eng.retrieve_batch(Qm, K=5, seeds=seeds)
    ri, *_ = walk_batch(G, other, Qm, seeds, 5, 100, 50)
    assert np.array_equal(oi, ri) and not np.array_equal(oi, idx)
    eng.close()


def test_errors_launch_nothing(fx):
    f, G, _, nbr, Qm, ix = fx
    q = torch.from_numpy(Qm).cuda()
    nb = torch.from_numpy(nbr).cuda()
    sd = torch.from_numpy(golden_seeds(len(G), 5)).cuda()
    with pytest.raises(_lib.MMRError, match=r"r=513 outside \[1, 512\]"):
        ix.dls_walk(q, nb, sd, 5, r=513)
    with pytest.raises(_lib.MMRError, match=r"k=51 outside \[1, r=50\]"):
        ix.dls_walk(q, nb, sd, 51, r=50)
    wide = torch.full((len(G), 33), -1, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.MMRError, match=r"max_links=33 outside \[1, 32\]"):
        ix.dls_walk(q, wide, sd, 5)
    with pytest.raises(_lib.MMRError, match=r"seed_size=5 outside \[0, r=4\]"):
        ix.dls_walk(q, nb, sd, 2, r=4)
    big = GalleryIndex(synthetic.gauss_gallery(5000, 128, 3))       # the visited-set bound is min(n, ...)
    with pytest.raises(_lib.MMRError, match=r"visited-set limit 4096"):
        big.dls_walk(q, torch.full((5000, 32), -1, dtype=torch.int64, device="cuda"), sd, 5, max_steps=1000)
    assert b"4096" in _lib.lib().mmr_last_error()
    big.close()
    half = GalleryIndex(G.astype(np.float16))
    with pytest.raises(_lib.MMRError, match=r"status 4.*fp16"):
        half.dls_walk(q, nb, sd, 5)
    half.close()
    # nothing was launched or left pending: the stream is clean and the next walk is the golden one
    torch.cuda.synchronize()
    idx, *_ = ix.dls_walk(q, nb, sd, 5)
    assert np.array_equal(idx.cpu().numpy(), f["walk_idx"])
