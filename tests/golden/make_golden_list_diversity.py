"""Golden generator for the retrieval-diversity metrics: runs the reference's own compute_embedding_diversity,
compute_label_diversity_from_labels and summary_all_metrics (src/Evaluate/retrieval_diversity_compute.py:142-194,
loaded by file path) on about 40 small lists and writes tests/golden/list_diversity.npz — inputs and results only.
Run by hand next to make_golden.py (whose loader and reference location it reuses), never by the test suite,
bench.py or smoke().

Layout: per dimension D a small gallery G_<D> (n, D) f32 with label bitsets bits_<D> (n,) uint64; the lists are row
numbers into the gallery of their dimension (list_dim, list_off, list_idx); ref_emb / ref_lab are the reference's
values per list; summary_<column> the 8 columns of summary_all_metrics (list_div_ref.COLUMNS) for the per-list
columns and for columns with missing values (col_<column> holds those inputs); max_dev the observed max
|reference - f64 restatement| of the embedding diversity, for the record (the tests use the derived bound).

Cases: K in {0, 1, 2, 3, 5, 10} at D in {5, 16, 64}; three K = 5 lists at D = 768; clustered and near-orthogonal
rows; a zero row; rows of 1e-9 (norm below the 1e-8 clip); a row listed twice; two byte-identical rows; label lists
with empty sets, only empty sets, a 43-label and a 64-label row.
"""
import sys
from pathlib import Path

import numpy as np
import pandas as pd

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import make_golden as mg  # noqa: E402  (loader + the reference's location)
import list_div_ref as R  # noqa: E402

SEED = mg.SEED + 60
ALL43, ALL64 = np.uint64((1 << 43) - 1), np.uint64(0xFFFFFFFFFFFFFFFF)


def gallery(d, rng):
    if d == 4:
        G = rng.standard_normal((8, 4)).astype(np.float32)
        G[0:2] = np.float32(1e-9)          # |g| = 2e-9 < the clip
        G[2] = 0.0
        return G
    if d == 768:
        G = rng.standard_normal((12, d)).astype(np.float32)
        G[5:10] = G[4] + 0.1 * rng.standard_normal((5, d)).astype(np.float32)
        return G
    G = rng.standard_normal((24, d)).astype(np.float32)
    G[10:15] = G[9] + 0.05 * rng.standard_normal((5, d)).astype(np.float32)                 # clustered
    G[15:20] = 3.0 * np.eye(5, d, dtype=np.float32) + 0.01 * rng.standard_normal((5, d)).astype(np.float32)
    G[20] = 0.0
    G[21] = G[3]                                                                            # byte-identical rows
    return G


def labels(n, rng):
    b = np.zeros(n, np.uint64)
    for i in range(n):
        for j in rng.choice(43, size=int(rng.integers(1, 4)), replace=False):
            b[i] |= np.uint64(1) << np.uint64(j)
    b[:min(3, n)] = 0                      # records without labels
    if n > 5:
        b[4], b[5] = ALL43, ALL64
    return b


def main():
    ref = mg._load_file("Evaluate_retrieval_diversity_compute", mg.REF / "Evaluate" / "retrieval_diversity_compute.py")
    rng = np.random.default_rng(SEED)
    dims = (4, 5, 16, 64, 768)
    G = {d: gallery(d, rng) for d in dims}
    B = {d: labels(len(G[d]), rng) for d in dims}
    lists = []
    pool = np.array(list(range(10)) + [22, 23])
    for d in (5, 16, 64):
        for k in (0, 1, 2, 3, 5, 10):
            lists.append((d, rng.choice(pool, size=k, replace=False)))
        lists += [(d, np.arange(10, 15)), (d, np.arange(15, 20))]
    lists += [(4, [0, 1]), (4, [0, 1, 3]), (4, [2, 3, 4]), (4, [2, 2]), (4, [3, 4, 5, 6, 7])]
    lists += [(16, [3, 3, 5]), (16, [3, 21, 7]), (16, [20, 1, 2])]
    lists += [(768, rng.choice(12, size=5, replace=False)) for _ in range(2)] + [(768, np.arange(5, 10))]
    lists += [(64, [0, 1, 2]), (64, [0, 4, 6]), (64, [5, 4, 7, 8])]
    lists = [(d, np.asarray(ix, np.int64)) for d, ix in lists]

    ref_emb, ref_lab, dev = [], [], 0.0
    for d, ix in lists:
        emb = G[d][ix] if len(ix) else np.array([])          # as run_retrieval_experiment builds it
        ref_emb.append(ref.compute_embedding_diversity(emb))
        ref_lab.append(ref.compute_label_diversity_from_labels([R.bits_to_names(b) for b in B[d][ix]]))
        if len(ix):
            mine = R.list_diversity_ref(G[d], ix[None], B[d])
            p = int(mine["pairs"][0])
            assert abs(mine["emb_div"][0] - ref_emb[-1]) <= R.TOL32(d, p), (d, ix, mine["emb_div"][0], ref_emb[-1])
            assert mine["label_div"][0] == ref_lab[-1], (d, ix)
            dev = max(dev, abs(mine["emb_div"][0] - ref_emb[-1]))
    ref_emb, ref_lab = np.array(ref_emb, np.float64), np.array(ref_lab, np.float64)

    cols = {"retrieval_diversity": ref_emb, "retrieval_label_diversity": ref_lab}
    with_nan = ref_emb.copy()
    with_nan[::4] = np.nan
    single = np.full(len(lists), np.nan)
    single[7] = ref_emb[7]
    cols.update(with_nan=with_nan, single=single, all_nan=np.full(len(lists), np.nan))
    df = pd.DataFrame({"qid": [f"q{i}" for i in range(len(lists))], **cols})
    summ = ref.summary_all_metrics(df)
    out = {f"G_{d}": G[d] for d in dims}
    out.update({f"bits_{d}": B[d] for d in dims})
    out.update(list_dim=np.array([d for d, _ in lists], np.int64),
               list_off=np.cumsum([0] + [len(ix) for _, ix in lists]).astype(np.int64),
               list_idx=np.concatenate([ix for _, ix in lists]).astype(np.int64),
               ref_emb=ref_emb, ref_lab=ref_lab, max_dev=np.float64(dev))
    for name, v in cols.items():
        out[f"col_{name}"] = np.asarray(v, np.float64)
        out[f"summary_{name}"] = np.array([float(summ.loc[name, c]) for c in R.COLUMNS], np.float64)
    np.savez_compressed(HERE / "list_diversity.npz", **out)
    print("wrote list_diversity.npz:", len(lists), "lists, max_dev", dev)
    print(summ)


if __name__ == "__main__":
    main()
