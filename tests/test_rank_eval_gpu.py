"""GPU: the full-ranking label evaluation (mmr_index_best_relevant / mmr_index_count_ahead, csrc/rank_eval.hip)
through GalleryIndex.best_relevant / count_ahead / rank_eval, ShardedIndex.rank_eval and the engines' evaluate(),
against the numpy f64 reference of rank_eval_ref.py.

Gaussian rows, each with 1-2 of 43 random labels, so first relevant ranks are deep.  The shapes are the smallest
that reach every edge: one row, a partial 16-row tile (63), one row past a 256-row block (257), several blocks
(1000); D = 1, 7 (below one k step), 100 (zero-padded to 128), 768, 1088; one query, a partial query tile (17),
one query past a tile (33), several tiles (257), and more queries than one internal pass (1030).

Tolerance: scores to rank_eval_ref.TOL = 1e-12 (derived there).  Ranks are compared exactly: every case asserts
that the reference's rank interval [lo, hi] is a point (no other score within TOL of the best relevant one), or,
where ties are built in (duplicates, zero rows), uses the exact (score desc, index asc) rank."""
import functools
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rank_eval_ref as R
from conftest import GOLDEN
from mmr_amd import metrics, synthetic
from mmr_amd.parallel import ShardedIndex, shard_bounds
from mmr_amd.retrieval import GalleryIndex, MI355XRetrievalEngine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(DEV)


def _index(G, half, idx_base=0):
    """(index, the rows as the index holds them, f32)."""
    if half:
        Gh = np.asarray(G, np.float16)
        return GalleryIndex(Gh, device=0, idx_base=idx_base), Gh.astype(np.float32)
    return GalleryIndex(np.asarray(G, np.float32), device=0, idx_base=idx_base, mode="x3"), np.asarray(G, np.float32)


def _run(ix, Q, qb, gb, ex=None):
    exd = None if ex is None else torch.from_numpy(ex).to(DEV)
    out = ix.rank_eval(torch.from_numpy(Q).to(DEV), _bits(qb), _bits(gb), exd)
    return tuple(t.cpu().numpy() for t in out)


def _check(got, ref, qb, gb, ex, idx_base, exact_rank=False):
    first, n_rel, bi, bs = got
    np.testing.assert_array_equal(n_rel, ref["n_rel"])
    has = ref["n_rel"] > 0
    assert np.array_equal(bi >= 0, has) and np.all(bs[~has] == 0.0)
    loc = bi[has] - idx_base
    assert np.all((loc >= 0) & (loc < len(gb)))
    assert np.all((gb[loc] & qb[has]) != 0), "best_idx is not relevant"
    if ex is not None:
        assert np.all(bi[has] != ex[has]), "best_idx is the excluded row"
    err = np.abs(bs[has] - ref["S"][np.nonzero(has)[0], loc])
    print("max |best_score - ref| =", err.max() if err.size else 0.0)
    assert np.all(err <= R.TOL)
    if exact_rank:
        np.testing.assert_array_equal(first, ref["rank"])
    else:
        np.testing.assert_array_equal(ref["lo"], ref["hi"])      # the condition of the exact comparison
        np.testing.assert_array_equal(first, ref["lo"])


def _excludes(ref, n, idx_base, seed):
    """A third of the queries exclude their best relevant row, a third a random row, the rest nothing."""
    rng = np.random.default_rng(seed)
    nq = len(ref["rank"])
    ex = np.full(nq, -1, np.int64)
    for q in range(nq):
        if q % 3 == 0 and ref["best_idx"][q] >= 0:
            ex[q] = ref["best_idx"][q]
        elif q % 3 == 1:
            ex[q] = idx_base + int(rng.integers(0, n))
    return ex


# (N, D, Q, fp16 index, idx_base, with exclusions)
SHAPES = [
    (257, 100, 33, False, 0, False),
    (257, 100, 33, True, 1000, True),
    (1, 1, 1, False, 0, False),
    (1, 7, 17, True, 1000, False),
    (63, 7, 33, False, 1000, True),
    (63, 768, 1, True, 0, False),
    (257, 1088, 17, False, 0, True),
    (1000, 768, 257, False, 0, False),
    (1000, 100, 257, True, 1000, True),
    (1000, 7, 17, False, 0, False),
    (257, 768, 257, True, 0, False),
    (1000, 1088, 33, True, 1000, False),
    (63, 7, 1030, False, 1000, True),       # more queries than one internal pass
]


@pytest.mark.parametrize("N,D,Q,half,idx_base,with_ex", SHAPES)
def test_rank_eval_shapes(N, D, Q, half, idx_base, with_ex):
    G, Qm = R.gauss(N, D, 100 + N + D), R.gauss(Q, D, 200 + Q + D)
    gb, qb = R.sparse_bits(N, 300 + N), R.sparse_bits(Q, 400 + Q)
    ix, Gx = _index(G, half, idx_base)
    ex = None
    if with_ex:
        ex = _excludes(R.rank_eval_ref(Qm, Gx, qb, gb, None, idx_base), N, idx_base, 500 + N)
    ref = R.rank_eval_ref(Qm, Gx, qb, gb, ex, idx_base)
    got = _run(ix, Qm, qb, gb, ex)
    ix.close()
    if N >= 257:
        assert ref["rank"].max() > 10                          # deep first ranks
    _check(got, ref, qb, gb, ex, idx_base)


@functools.lru_cache(maxsize=None)
def _base_case():
    """(257, 100, 33): the rows, queries, bitsets and the unexcluded reference the edge tests share (read-only)."""
    N, D, Q = 257, 100, 33
    G, Qm = R.gauss(N, D, 41), R.gauss(Q, D, 42)
    gb, qb = R.sparse_bits(N, 43), R.sparse_bits(Q, 44)
    return G, Qm, gb, qb, R.rank_eval_ref(Qm, G, qb, gb)


@pytest.mark.parametrize("half", [False, True])
def test_pad_rows_do_not_count(half):
    """N = 257 (255 pad rows, score 0): each query's only relevant row is its own negation (cosine -1), so all
    256 other real rows rank ahead of it and no pad row does."""
    N, D = 257, 16
    G = np.asarray(R.gauss(N, D, 51), np.float16).astype(np.float32)
    Qm = np.asarray(R.gauss(3, D, 52), np.float16).astype(np.float32)
    rows = [5, 100, 256]
    gb = np.full(N, np.uint64(1) << np.uint64(20), np.uint64)
    qb = np.zeros(3, np.uint64)
    for i, r in enumerate(rows):
        G[r] = -Qm[i]
        gb[r] = np.uint64(1) << np.uint64(i)
        qb[i] = np.uint64(1) << np.uint64(i)
    ix, Gx = _index(G, half)
    ref = R.rank_eval_ref(Qm, Gx, qb, gb)
    got = _run(ix, Qm, qb, gb)
    ix.close()
    assert np.all(ref["best_score"] < -0.999) and ref["lo"].tolist() == [257, 257, 257]
    _check(got, ref, qb, gb, None, 0)
    assert got[0].tolist() == [257, 257, 257] and got[2].tolist() == rows


@pytest.mark.parametrize("half", [False, True])
def test_zero_rows_and_zero_query(half):
    """Two zero gallery rows score exactly 0: ordered by index among themselves, behind every positive score and
    ahead of every negative one; a zero query scores 0 everywhere, so its ranking is the index order."""
    N, D = 63, 7
    G = R.gauss(N, D, 61)
    G[[10, 40]] = 0.0
    Qm = R.gauss(3, D, 62)
    Qm[2] = 0.0
    gb = np.full(N, np.uint64(1), np.uint64)
    gb[40] = np.uint64(2)                          # the only row relevant to query 0: a zero row
    gb[[7, 30]] |= np.uint64(4)                    # query 2 (zero): first relevant row is 7
    qb = np.array([2, 1, 4], np.uint64)
    ix, Gx = _index(G, half)
    ref = R.rank_eval_ref(Qm, Gx, qb, gb)
    got = _run(ix, Qm, qb, gb)
    ix.close()
    s0 = ref["S"][0]
    assert s0[10] == 0.0 and s0[40] == 0.0 and np.min(np.abs(np.delete(s0, [10, 40]))) > 1e-6
    assert ref["rank"][0] == 1 + (s0 > 0).sum() + 1 and (s0 < 0).sum() > 0   # row 10 ahead by index, negatives behind
    assert ref["rank"][2] == 8 and ref["n_rel"][2] == 2
    _check(got, ref, qb, gb, None, 0, exact_rank=True)
    assert got[2].tolist()[0] == 40 and got[2].tolist()[2] == 7 and got[3][2] == 0.0


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("idx_base", [0, 1000])
def test_duplicates_rank_by_index(half, idx_base):
    """70 byte-identical rows, only copy c relevant: all 70 scores must be bit-identical in both passes, so the
    first rank is exactly c + 1 — no tolerance."""
    N, D = 70, 100
    G = np.repeat(np.asarray(R.gauss(1, D, 71), np.float16).astype(np.float32), N, axis=0)
    Qm = R.gauss(3, D, 72)
    copies = [0, 37, 69]
    gb = np.full(N, np.uint64(1) << np.uint64(30), np.uint64)
    qb = np.zeros(3, np.uint64)
    for i, c in enumerate(copies):
        gb[c] |= np.uint64(1) << np.uint64(i)
        qb[i] = np.uint64(1) << np.uint64(i)
    ix, _ = _index(G, half, idx_base)
    first, n_rel, bi, bs = _run(ix, Qm, qb, gb)
    ix.close()
    assert first.tolist() == [c + 1 for c in copies]
    assert n_rel.tolist() == [1, 1, 1] and bi.tolist() == [idx_base + c for c in copies]


def test_bitset_extremes_and_search_top1():
    G, Qm, gb, qb, _ = _base_case()
    N, Q = len(G), len(Qm)
    ix, _ = _index(G, False)
    qd = torch.from_numpy(Qm).to(DEV)
    # every row relevant: the best is the search's top-1 and the second pass reproduces its score bit for bit
    ones = np.full(Q, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    first, n_rel, bi, bs = _run(ix, Qm, ones, gb)
    si, _, s64 = ix.search(qd, 1, want_f64=True)
    assert first.tolist() == [1] * Q and n_rel.tolist() == [N] * Q
    np.testing.assert_array_equal(bi, si.cpu().numpy()[:, 0])
    assert np.max(np.abs(bs - s64.cpu().numpy()[:, 0])) <= R.TOL
    # only label bit 63 shared
    gb63 = gb.copy()
    gb63[::7] |= np.uint64(1) << np.uint64(63)
    q63 = np.full(Q, np.uint64(1) << np.uint64(63), np.uint64)
    _check(_run(ix, Qm, q63, gb63), R.rank_eval_ref(Qm, G, q63, gb63), q63, gb63, None, 0)
    # no label at all
    first, n_rel, bi, bs = _run(ix, Qm, np.zeros(Q, np.uint64), gb)
    assert not first.any() and not n_rel.any() and np.all(bi == -1) and np.all(bs == 0.0)
    ix.close()


def test_no_queries_and_bad_shapes():
    G, Qm, gb, qb, _ = _base_case()
    ix, _ = _index(G, False)
    out = ix.rank_eval(torch.empty((0, G.shape[1]), device=DEV), _bits(qb[:0]), _bits(gb))   # nq == 0: no launch
    assert all(t.shape == (0,) for t in out)
    with pytest.raises(ValueError):
        ix.rank_eval(torch.from_numpy(Qm[:, :50]).to(DEV), _bits(qb), _bits(gb))
    with pytest.raises(ValueError):
        ix.best_relevant(torch.from_numpy(Qm).to(DEV), _bits(qb), _bits(gb[:100]))
    ix.close()


def test_exclusion():
    G, Qm, gb, qb, ref0 = _base_case()
    Q = len(Qm)
    ix, _ = _index(G, False, 1000)
    none = _run(ix, Qm, qb, gb)
    minus1 = _run(ix, Qm, qb, gb, np.full(Q, -1, np.int64))
    for a, b in zip(none, minus1):                              # exclude = -1 equals NULL, to the byte
        assert a.tobytes() == b.tobytes()
    # excluding the best relevant row: the second best takes over, n_rel drops by one
    ex = none[2].copy()
    assert np.all(ex >= 1000)
    ref = R.rank_eval_ref(Qm, G, qb, gb, ex, 1000)
    got = _run(ix, Qm, qb, gb, ex)
    _check(got, ref, qb, gb, ex, 1000)
    np.testing.assert_array_equal(got[1], none[1] - 1)
    assert np.all(got[2] != none[2]) and np.all(got[0] >= none[0])
    # an excluded row that ranks ahead of the best is not counted
    deep = none[0] > 1
    assert deep.sum() > 10
    top1 = 1000 + np.argmax(ref0["S"], axis=1)
    ex2 = np.where(deep, top1, -1)
    got2 = _run(ix, Qm, qb, gb, ex2)
    _check(got2, R.rank_eval_ref(Qm, G, qb, gb, ex2, 1000), qb, gb, ex2, 1000)
    np.testing.assert_array_equal(got2[0], none[0] - deep)
    np.testing.assert_array_equal(got2[2], none[2])
    ix.close()


def test_count_ahead_foreign_and_negative_reference():
    """ref_idx need not be a row of this index (the sharded case): the index only breaks exact score ties."""
    G, Qm, gb, qb, ref0 = _base_case()
    Q = len(Qm)
    ix, _ = _index(G, False, 1000)
    qd = torch.from_numpy(Qm).to(DEV)
    bi, bs, _ = ix.best_relevant(qd, _bits(qb), _bits(gb))
    own = ix.count_ahead(qd, bi, bs).cpu().numpy()
    np.testing.assert_array_equal(own + 1, ref0["lo"])
    # the same score under an index past / before every row of this index: the tied row itself counts / does not
    after = ix.count_ahead(qd, torch.full_like(bi, 10 ** 9), bs).cpu().numpy()
    before = ix.count_ahead(qd, torch.full_like(bi, 3), bs).cpu().numpy()
    np.testing.assert_array_equal(after, own + 1)
    np.testing.assert_array_equal(before, own)
    # a reference score no row has: the index plays no part
    assert np.min(np.abs(ref0["S"] - 0.01)) > R.TOL
    rs = torch.full((Q,), 0.01, dtype=torch.float64, device=DEV)
    got = ix.count_ahead(qd, torch.full_like(bi, 3), rs).cpu().numpy()
    np.testing.assert_array_equal(got, (ref0["S"] > 0.01).sum(1))
    # ref_idx < 0: nothing is counted — for some queries, and for all of them
    ri = bi.clone()
    ri[::2] = -1
    mixed = ix.count_ahead(qd, ri, bs).cpu().numpy()
    np.testing.assert_array_equal(mixed, np.where(np.arange(Q) % 2 == 0, 0, own))
    assert not ix.count_ahead(qd, torch.full_like(bi, -1), bs).cpu().numpy().any()
    ix.close()


def test_consistent_with_search_and_deterministic():
    N, D, Q = 1000, 768, 257
    G, Qm = R.gauss(N, D, 81), R.gauss(Q, D, 82)
    gb, qb = R.sparse_bits(N, 83), R.sparse_bits(Q, 84)
    ix, _ = _index(G, False)
    a = _run(ix, Qm, qb, gb)
    b = _run(ix, Qm, qb, gb)
    for x, y in zip(a, b):                                      # two runs: identical bytes
        assert x.tobytes() == y.tobytes()
    si = ix.search(torch.from_numpy(Qm).to(DEV), 10)[0].cpu().numpy()
    ix.close()
    rel = (gb[si] & qb[:, None]) != 0
    shallow = (a[0] > 0) & (a[0] <= 10)
    assert shallow.sum() > 20 and (~shallow).sum() > 20
    np.testing.assert_array_equal(rel[shallow].argmax(1) + 1, a[0][shallow])
    assert not rel[~shallow].any()                              # a deeper first rank: nothing relevant in the top 10


# ---------------------------------------------------------------- sharding
def _shard_case(world, b):
    N, D = 515, 100
    G, Q = R.gauss(N, D, 91), R.gauss(world * b, D, 92)
    gb, qb = R.sparse_bits(N, 93), R.sparse_bits(world * b, 94)
    G[300] = G[7]                                              # byte-identical rows on either side of the boundary
    gb[7] = gb[300] = np.uint64(1) << np.uint64(50)
    Q[0] = G[7]                                                # query 0: the pair is its best relevant rows
    qb[0] = np.uint64(1) << np.uint64(50)
    Q[3] = G[7] + 0.05 * R.gauss(1, D, 95)[0]                  # query 3: the pair ranks ahead of its best
    qb[5] = 0
    ex = np.full(world * b, -1, np.int64)
    ex[1], ex[4] = 20, 400
    return N, D, G, Q, gb, qb, ex


def _worker_world2(rank, world, port, b, out_q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        N, D, G, Q, gb, qb, ex = _shard_case(world, b)
        s, e = shard_bounds(N, world)[rank]
        ix = GalleryIndex(G[s:e], device=0, idx_base=s)

        def best(q, q_bits, g_bits, exclude):   # gloo exchanges host tensors: device steps, results staged to host
            return tuple(t.cpu() for t in ix.best_relevant(q.cuda(), q_bits.cuda(), g_bits.cuda(), exclude.cuda()))

        def ahead(q, ref_idx, ref_score, exclude):
            return ix.count_ahead(q.cuda(), ref_idx.cuda(), ref_score.cuda(), exclude.cuda()).cpu()

        sh = ShardedIndex(None, N, s, local_search=lambda q, k: None, local_best_relevant=best, local_count_ahead=ahead)
        out = sh.rank_eval(torch.from_numpy(Q[rank * b:(rank + 1) * b]), torch.from_numpy(qb.view(np.int64)),
                           torch.from_numpy(gb[s:e].view(np.int64)), torch.from_numpy(ex))
        out_q.put((rank,) + tuple(t.numpy() for t in out))
        ix.close()
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_sharded_rank_eval_world2_equals_single_index():
    """Two GalleryIndex halves (both on cuda:0, lists staged to host for gloo) = one index over the whole gallery,
    bit for bit; byte-identical rows straddle the shard boundary."""
    world, b = 2, 6
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_world2, args=(r, world, port, b, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    N, D, G, Q, gb, qb, ex = _shard_case(world, b)
    ix, _ = _index(G, False)
    one = _run(ix, Q, qb, gb, ex)
    ix.close()
    assert (one[0][0], one[2][0], one[1][0]) == (1, 7, 2) and one[0][3] >= 3 and one[0][5] == 0
    _check(one, R.rank_eval_ref(Q, G, qb, gb, ex), qb, gb, ex, 0, exact_rank=True)
    for rank, *out in res:
        for got, want in zip(out, one):
            assert got.tobytes() == want[rank * b:(rank + 1) * b].tobytes()


def _golden(name):
    g = json.load(open(os.path.join(GOLDEN, name)))
    if name == "ranking.json":
        G, gl = synthetic.labelled_gallery(g["n_gallery"], g["D"], g["seed_g"])
        Qm, ql = synthetic.labelled_gallery(g["n_query"], g["D"], g["seed_q"])
    else:
        s = g["seed"]
        G, Qm = R.gauss(g["n_gallery"], g["D"], s), R.gauss(g["n_query"], g["D"], s + 1)
        gl, ql = R.sparse_labels(g["n_gallery"], s + 2), R.sparse_labels(g["n_query"], s + 3)
    return g, G, Qm, synthetic.labels_to_bits(gl), synthetic.labels_to_bits(ql)


def _worker_rccl1(port, out_q):
    """ShardedRetrievalEngine.evaluate at world 1 over RCCL: the device path of the collective."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        from mmr_amd.parallel import ShardedRetrievalEngine
        g, G, Qm, gb, qb = _golden("rank_eval.json")
        eng = ShardedRetrievalEngine(embs=G, ids=[str(i) for i in range(len(G))])
        ex = np.arange(len(Qm), dtype=np.int64) * 3
        outs = []
        for e in (None, ex):
            r = eng.evaluate(Qm, qb, gb, ks=(1, 5, 10), exclude_ids=e)
            outs.append({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()})
        out_q.put(outs)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", ["ranking.json", "rank_eval.json"])
def test_engine_evaluate_reproduces_the_reference(name):
    """compute_ranking_metrics' recorded values: ranking.json (first ranks all 1) and rank_eval.json (deep ranks,
    the fixture only a full ranking satisfies), to 1e-12."""
    g, G, Qm, gb, qb = _golden(name)
    eng = MI355XRetrievalEngine(embs=G, ids=[str(i) for i in range(len(G))])
    res = eng.evaluate(Qm, qb, gb, ks=(1, 5, 10))
    ref = R.rank_eval_ref(Qm, G, qb, gb)
    np.testing.assert_array_equal(res["first_rank"].cpu().numpy(), ref["rank"])
    np.testing.assert_array_equal(res["n_rel"].cpu().numpy(), ref["n_rel"])
    for k, want in g["cases"].items():
        assert res["mrr"] == pytest.approx(want["mrr"], abs=1e-12)
        assert res[f"hit@{k}"] == pytest.approx(want["hit_at_k"], abs=1e-12)
        assert res[f"recall@{k}"] == pytest.approx(want["recall_at_k"], abs=1e-12)
    if name == "rank_eval.json":
        assert res["mrr@10"] < res["mrr"] - 0.01          # what a top-10 list alone would have reported
    eng.close()


def _evaluate_ref(G, Qm, gb, qb, ex, ks):
    """evaluate()'s dict from the numpy reference and the id-list functions."""
    from oracle import knn as oknn
    ref = R.rank_eval_ref(Qm, G, qb, gb, ex)
    K = max(ks)
    top, _ = oknn.exact_topk(Qm, G, K + 1)
    lists = [[int(j) for j in row if ex is None or j != ex[q]][:K] for q, row in enumerate(top)]
    rels = [set(np.nonzero(((gb & qb[q]) != 0) & (np.arange(len(G)) != (-1 if ex is None else ex[q])))[0].tolist())
            for q in range(len(Qm))]
    out = {"mrr": float(np.mean(np.where(ref["rank"] > 0, 1.0 / np.maximum(ref["rank"], 1), 0.0))),
           f"mrr@{K}": metrics.mean_reciprocal_rank(lists, rels)}
    for k in ks:
        out[f"hit@{k}"] = float(np.mean((ref["rank"] > 0) & (ref["rank"] <= k)))
        out[f"recall@{k}"] = float(np.mean([metrics.recall_at_k(r, s, k) for r, s in zip(lists, rels)]))
        out[f"p@{k}"] = float(np.mean([metrics.precision_at_k(r, s, k) for r, s in zip(lists, rels)]))
        out[f"map@{k}"] = metrics.mean_average_precision(lists, rels, k)
        out[f"ndcg@{k}"] = float(np.mean([metrics.ndcg_at_k(r, s, k) for r, s in zip(lists, rels)]))
    return out, ref


def test_evaluate_with_exclusions_single_and_sharded_engine():
    """evaluate() with and without exclude_ids on the deep-rank fixture: every value equals the numpy reference +
    the id-list functions, and ShardedRetrievalEngine.evaluate (world 1 over RCCL) equals the one-GPU engine."""
    g, G, Qm, gb, qb = _golden("rank_eval.json")
    ks = (1, 5, 10)
    ex = np.arange(len(Qm), dtype=np.int64) * 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker_rccl1, args=(_free_port(), q))
    p.start()
    eng = MI355XRetrievalEngine(embs=G, ids=[str(i) for i in range(len(G))])
    mine = [eng.evaluate(Qm, qb, gb, ks=ks, exclude_ids=e) for e in (None, [str(i) for i in ex])]
    eng.close()
    for res, e in zip(mine, (None, ex)):
        want, ref = _evaluate_ref(G, Qm, gb, qb, e, ks)
        np.testing.assert_array_equal(ref["lo"], ref["hi"])
        np.testing.assert_array_equal(res["first_rank"].cpu().numpy(), ref["rank"])
        np.testing.assert_array_equal(res["n_rel"].cpu().numpy(), ref["n_rel"])
        for k, v in want.items():
            assert res[k] == pytest.approx(v, abs=1e-12), k
    sharded = q.get(timeout=180)
    p.join(timeout=60)
    assert p.exitcode == 0
    for res, sh in zip(mine, sharded):
        for k, v in res.items():
            if isinstance(v, torch.Tensor):
                np.testing.assert_array_equal(sh[k], v.cpu().numpy())
            else:
                assert sh[k] == v, k
