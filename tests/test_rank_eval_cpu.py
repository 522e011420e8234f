"""CPU: the numpy reference of the full-ranking evaluation (rank_eval_ref.py) against metrics.ranking_metrics
and the reference-pinned fixtures, metrics.list_metrics against the id-list functions, and the sharded
collective (ShardedIndex.rank_eval) over gloo with the two local steps injected — before the GPU file relies
on any of them."""
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
from oracle import knn as oknn


def test_helper_matches_ranking_metrics_on_a_full_ranking():
    N, Q, D = 300, 25, 32
    G, Qm = R.gauss(N, D, 11), R.gauss(Q, D, 12)
    gb, qb = R.sparse_bits(N, 13), R.sparse_bits(Q, 14)
    qb[3] = 0                                     # a query with no relevant row
    ref = R.rank_eval_ref(Qm, G, qb, gb)
    full, _ = oknn.exact_topk(Qm, G, N)
    assert ref["rank"].max() > 10 and ref["rank"][3] == 0 and ref["n_rel"][3] == 0
    assert np.array_equal(ref["lo"], ref["rank"]) and np.array_equal(ref["hi"], ref["rank"])
    for k in (1, 5, 10):
        want = metrics.ranking_metrics(full, qb, gb, k)                    # first ranks from the full list
        got = metrics.ranking_metrics(full[:, :k], qb, gb, k, first_rank=ref["rank"])
        assert got == pytest.approx(want, abs=1e-15)
        rel_top = (gb[full[:, :k]] & qb[:, None]) != 0
        assert R.summary_ref(ref["rank"], rel_top, ref["n_rel"], k) == pytest.approx(want, abs=1e-15)
        trunc = metrics.ranking_metrics(full[:, :k], qb, gb, k)            # the truncated form undercounts MRR
        assert trunc[0] < want[0]


def test_helper_exclusion_and_ties():
    G = np.zeros((6, 4), np.float32)
    G[0] = [1, 0, 0, 0]
    G[1] = [1, 0, 0, 0]      # exact duplicate of row 0
    G[2] = [0, 1, 0, 0]
    G[4] = [-1, 0, 0, 0]     # rows 3 and 5 stay zero (score 0)
    q = np.array([[1, 0, 0, 0]], np.float32)
    gb = np.array([1, 2, 0, 4, 4, 4], np.uint64)
    ref = R.rank_eval_ref(q, G, np.array([2], np.uint64), gb)
    assert (ref["best_idx"][0], ref["rank"][0], ref["n_rel"][0]) == (1, 2, 1)      # tie with row 0: index order
    ref = R.rank_eval_ref(q, G, np.array([2], np.uint64), gb, exclude=[0])
    assert (ref["best_idx"][0], ref["rank"][0]) == (1, 1)                          # the excluded row is not counted
    ref = R.rank_eval_ref(q, G, np.array([4], np.uint64), gb, idx_base=100)
    assert (ref["best_idx"][0], ref["rank"][0], ref["n_rel"][0]) == (103, 4, 3)    # zero rows: score 0, by index
    ref = R.rank_eval_ref(q, G, np.array([4], np.uint64), gb, exclude=[103], idx_base=100)
    assert (ref["best_idx"][0], ref["rank"][0], ref["n_rel"][0]) == (105, 4, 2)
    assert R.count_ahead_ref(ref["S"], [-1], [0.0]).tolist() == [0]
    assert R.count_ahead_ref(ref["S"], [10 ** 6], [0.0]).tolist() == [5]            # a row of another shard


def _fixture_case(name):
    g = json.load(open(os.path.join(GOLDEN, name)))
    if name == "ranking.json":
        G, gl = synthetic.labelled_gallery(g["n_gallery"], g["D"], g["seed_g"])
        Qm, ql = synthetic.labelled_gallery(g["n_query"], g["D"], g["seed_q"])
    else:
        s = g["seed"]
        G, Qm = R.gauss(g["n_gallery"], g["D"], s), R.gauss(g["n_query"], g["D"], s + 1)
        gl, ql = R.sparse_labels(g["n_gallery"], s + 2), R.sparse_labels(g["n_query"], s + 3)
    return g, G, Qm, synthetic.labels_to_bits(gl), synthetic.labels_to_bits(ql)


@pytest.mark.parametrize("name", ["ranking.json", "rank_eval.json"])
def test_helper_reproduces_the_reference_fixtures(name):
    """compute_ranking_metrics' recorded (mrr, hit@k, recall@k): ranking.json (clustered labels, every first rank
    1) and rank_eval.json (sparse labels, first ranks up to tens of rows deep)."""
    g, G, Qm, gb, qb = _fixture_case(name)
    ref = R.rank_eval_ref(Qm, G, qb, gb)
    assert np.array_equal(ref["lo"], ref["hi"])
    top, _ = oknn.exact_topk(Qm, G, 10)
    rel_top = (gb[top] & qb[:, None]) != 0
    if name == "rank_eval.json":
        assert ref["rank"].max() == g["first_rank_max"] > 10 and ref["rank"].sum() == g["first_rank_sum"]
        assert ref["n_rel"].sum() == g["n_rel_sum"]
    for k, want in g["cases"].items():
        mrr, hit, rec = R.summary_ref(ref["rank"], rel_top, ref["n_rel"], int(k))
        assert mrr == pytest.approx(want["mrr"], abs=1e-12)
        assert hit == pytest.approx(want["hit_at_k"], abs=1e-12)
        assert rec == pytest.approx(want["recall_at_k"], abs=1e-12)
        got = metrics.evaluation_summary(torch.from_numpy(rel_top), torch.from_numpy(ref["rank"]),
                                         torch.from_numpy(ref["n_rel"]), (int(k),))
        assert got["mrr"] == pytest.approx(want["mrr"], abs=1e-12)
        assert got[f"hit@{k}"] == pytest.approx(want["hit_at_k"], abs=1e-12)
        assert got[f"recall@{k}"] == pytest.approx(want["recall_at_k"], abs=1e-12)


def test_list_metrics_match_the_id_list_functions():
    m = json.load(open(os.path.join(GOLDEN, "ranking.json")))["metrics"]
    lists = m["lists"]
    flags = torch.tensor([[r in set(rel) for r in ret] for ret, rel in lists])
    n_rel = torch.tensor([len(set(rel)) for _, rel in lists])
    L = flags.shape[1]
    for k in (1, 5, 10, 20):
        got = metrics.list_metrics(flags, n_rel, k)
        for i, ((ret, rel), row) in enumerate(zip(lists, m["per_list"])):
            rs = set(rel)
            assert got["p"][i].item() == pytest.approx(metrics.precision_at_k(ret, rel, k), abs=1e-15)
            assert got["p"][i].item() == pytest.approx(row[f"p@{k}"], abs=1e-15)
            assert got["r"][i].item() == pytest.approx(row[f"r@{k}"], abs=1e-15)
            assert got["ndcg"][i].item() == pytest.approx(row[f"ndcg@{k}"], abs=1e-12)
            assert got["ap"][i].item() == pytest.approx(metrics.average_precision(ret, rs, k), abs=1e-15)
            assert got["rr"][i].item() == pytest.approx(metrics.mean_reciprocal_rank([ret[:k]], [rs]), abs=1e-15)
    full = metrics.list_metrics(flags, n_rel, L)
    assert full["ap"].mean().item() == pytest.approx(m["map"], abs=1e-15)
    assert metrics.list_metrics(flags, n_rel, 10)["ap"].mean().item() == pytest.approx(m["map@10"], abs=1e-15)
    assert full["rr"].mean().item() == pytest.approx(m["mrr"], abs=1e-15)
    # no relevant item at all, and a list without a hit: every metric 0, as the id-list functions give
    got = metrics.list_metrics(torch.zeros((2, 5), dtype=torch.bool), torch.tensor([0, 3]), 5)
    ret = ["a", "b", "c", "d", "e"]
    for i, rel in enumerate([set(), {"x", "y", "z"}]):
        assert got["p"][i].item() == metrics.precision_at_k(ret, rel, 5) == 0.0
        assert got["r"][i].item() == metrics.recall_at_k(ret, rel, 5) == 0.0
        assert got["ap"][i].item() == metrics.average_precision(ret, rel, 5) == 0.0
        assert got["ndcg"][i].item() == metrics.ndcg_at_k(ret, rel, 5) == 0.0
        assert got["rr"][i].item() == metrics.mean_reciprocal_rank([ret], [rel]) == 0.0


def test_c_abi_version_and_argument_checks_without_gpu():
    """The ABI grew: mmr_version() == the binding's ABI_VERSION (2), and the new entry points reject bad
    arguments before touching the device."""
    import ctypes

    from mmr_amd import _lib
    L = _lib.lib()
    assert L.mmr_version() == _lib.ABI_VERSION == 2
    assert L.mmr_index_rank_work_bytes(None, 10) == 0
    p = ctypes.c_void_p(256)
    assert L.mmr_index_best_relevant(None, p, 1, p, p, None, p, p, p, p, None) == 1
    assert b"index is NULL" in L.mmr_last_error()
    assert L.mmr_index_count_ahead(None, p, 1, p, p, None, p, p, None) == 1
    assert b"index is NULL" in L.mmr_last_error()


# ---------------------------------------------------------------- the sharded collective over gloo
def _sharded_case(world, b, N, D=24):
    G, Q = R.gauss(N, D, 31), R.gauss(world * b, D, 32)
    G[N - 2] = G[1]                                        # an exact duplicate across the shards
    gb, qb = R.sparse_bits(N, 33, nlab=12), R.sparse_bits(world * b, 34, nlab=12)
    gb[1] = gb[N - 2] = np.uint64(1) << np.uint64(40)       # ... relevant to query 0 only
    Q[0] = G[1]
    qb[0] = np.uint64(1) << np.uint64(40)
    qb[2] = 0                                              # no relevant row
    ex = np.full(world * b, -1, np.int64)
    ex[1] = R.rank_eval_ref(Q[1:2], G, qb[1:2], gb)["best_idx"][0]     # the best relevant row itself
    ex[4] = int(np.argmax(R.scores(Q[4:5], G)[0]))                      # the top row of the ranking
    return G, Q, gb, qb, ex


def _worker(rank, world, port, b, N, out_q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        G, Q, gb, qb, ex = _sharded_case(world, b, N)
        s, e = shard_bounds(N, world)[rank]
        S = R.scores(Q, G)[:, s:e]                         # one score matrix, sliced: the shards' scores agree bit for bit

        def best(q, q_bits, g_bits, exclude):
            return tuple(torch.from_numpy(x) for x in
                         R.best_relevant_ref(S, q_bits.numpy().view(np.uint64), g_bits.numpy().view(np.uint64),
                                             exclude.numpy(), idx_base=s))

        def ahead(q, ref_idx, ref_score, exclude):
            return torch.from_numpy(R.count_ahead_ref(S, ref_idx.numpy(), ref_score.numpy(), exclude.numpy(), idx_base=s))

        sh = ShardedIndex(None, N, s, local_search=lambda q, k: None, local_best_relevant=best, local_count_ahead=ahead)
        out = sh.rank_eval(torch.from_numpy(Q[rank * b:(rank + 1) * b]), torch.from_numpy(qb.view(np.int64)),
                           torch.from_numpy(gb[s:e].view(np.int64)), torch.from_numpy(ex))
        out_q.put((rank,) + tuple(t.numpy() for t in out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,N", [(2, 301), (3, 20)])
def test_sharded_rank_eval_equals_unsharded(world, N):
    b = 5
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_worker, args=(r, world, port, b, N, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    G, Q, gb, qb, ex = _sharded_case(world, b, N)
    ref = R.rank_eval_ref(Q, G, qb, gb, exclude=ex)
    assert ref["best_idx"][0] == 1 and ref["rank"][0] == 1 and ref["n_rel"][0] == 2   # the duplicate pair
    assert ref["rank"][2] == 0 and ref["best_idx"][2] == -1
    for rank, first, n_rel, bi, bs in res:
        sl = slice(rank * b, (rank + 1) * b)
        np.testing.assert_array_equal(first, ref["rank"][sl])
        np.testing.assert_array_equal(n_rel, ref["n_rel"][sl])
        np.testing.assert_array_equal(bi, ref["best_idx"][sl])
        np.testing.assert_array_equal(bs, ref["best_score"][sl])
