"""Golden generator for the full-ranking evaluation with DEEP first-relevant ranks: runs the reference's
`compute_ranking_metrics` (src/Evaluate/retrieval_overlap.py:84-115) on Gaussian rows with sparse labels and
writes tests/golden/rank_eval.json — seeds and results only.  Run by hand next to make_golden.py (whose stub
loader it reuses), never by the test suite, bench.py or smoke().

ranking.json's clustered labels put every query's first relevant item at rank 1; here each row carries 1-2 of 43
random labels and the rows are unclustered, so the first relevant rank is tens of rows deep and an MRR taken from
a top-10 list is wrong.

The reference ranks in f32 through sklearn, the library in exact f64.  So the recorded seed is one for which the
two provably agree: the generator asserts, on the CPU, that the f32 ranking's first-relevant ranks equal the f64
helper's (tests/rank_eval_ref.py) for every query, that the helper's rank interval is a point (no score within
1e-12 of the best relevant one), and that the top-10 sets agree; a seed that fails is advanced.
"""
import importlib
import json
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import make_golden as mg  # noqa: E402  (stub loader + the reference's location)
import rank_eval_ref as R  # noqa: E402
from mmr_amd import synthetic  # noqa: E402
from oracle import knn as oknn  # noqa: E402

N, Q, D, KS = 600, 40, 64, (1, 5, 10)
SEED0 = mg.SEED + 40


def load_reference():
    mg.install_stubs()
    mg._pkg("Model", mg.REF / "Model", MultiModalRetrievalModel=None)
    mg._pkg("Retrieval", mg.REF / "Retrieval")
    sys.modules["Retrieval"].reranker = types.SimpleNamespace(Reranker=None)
    sys.modules["Retrieval.reranker"] = sys.modules["Retrieval"].reranker
    sys.modules["Helpers"].Config = importlib.import_module("Helpers.config").Config
    return mg._load_file("Evaluate_retrieval_overlap", mg.REF / "Evaluate" / "retrieval_overlap.py")


def data(seed):
    return (R.gauss(N, D, seed), R.gauss(Q, D, seed + 1), R.sparse_labels(N, seed + 2), R.sparse_labels(Q, seed + 3))


def f32_first_ranks(Qm, G, ql, gl):
    """First-relevant ranks and top-10 lists of the f32 ranking the reference sorts (sklearn + argsort)."""
    from sklearn.metrics.pairwise import cosine_similarity
    sim = cosine_similarity(Qm, G)
    rel = (ql.astype(np.int64) @ gl.astype(np.int64).T) > 0
    order = np.stack([np.argsort(sim[i])[::-1] for i in range(len(Qm))])
    hit = np.take_along_axis(rel, order, 1)
    return np.where(hit.any(1), hit.argmax(1) + 1, 0), order[:, :max(KS)]


def main():
    ro = load_reference()
    seed = SEED0
    while True:
        G, Qm, gl, ql = data(seed)
        qb, gb = synthetic.labels_to_bits(ql), synthetic.labels_to_bits(gl)
        ref = R.rank_eval_ref(Qm, G, qb, gb)
        r32, top32 = f32_first_ranks(Qm, G, ql, gl)
        top64, _ = oknn.exact_topk(Qm, G, max(KS))
        ok = (np.array_equal(r32, ref["rank"]) and np.array_equal(ref["lo"], ref["hi"])
              and np.array_equal(ref["lo"], ref["rank"]) and np.array_equal(top32, top64))
        if ok:
            break
        print("seed", seed, "f32 and f64 rankings differ: advancing")
        seed += 10
    out = {"n_gallery": N, "n_query": Q, "D": D, "seed": seed, "nlab": R.NUM_LABELS, "cases": {},
           "first_rank_min": int(ref["rank"].min()), "first_rank_max": int(ref["rank"].max()),
           "first_rank_sum": int(ref["rank"].sum()), "n_rel_sum": int(ref["n_rel"].sum())}
    rel_top = ((gb[top64] & qb[:, None]) != 0)
    for k in KS:
        mrr, hit, rec = ro.compute_ranking_metrics(Qm, G, ql, gl, k=k)
        want = R.summary_ref(ref["rank"], rel_top, ref["n_rel"], k)
        assert max(abs(a - b) for a, b in zip((mrr, hit, rec), want)) <= 1e-12, (k, (mrr, hit, rec), want)
        out["cases"][str(k)] = {"mrr": float(mrr), "hit_at_k": float(hit), "recall_at_k": float(rec)}
    (HERE / "rank_eval.json").write_text(json.dumps(out, indent=1) + "\n")
    print("wrote rank_eval.json", out)


if __name__ == "__main__":
    main()
