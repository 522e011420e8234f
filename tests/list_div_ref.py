"""f64 numpy restatement of mmr_index_list_diversity's semantics (include/mmr.h): retrieval diversity of lists of
GLOBAL indices over a gallery — compute_embedding_diversity / compute_label_diversity_from_labels of
src/Evaluate/retrieval_diversity_compute.py:171-194 with the validity rule, the 1e-8 norm clip and the label
bitsets spelled out.  Shared by test_list_diversity_cpu.py (against the reference's recorded values) and
test_list_diversity_gpu.py (the device against it).

Tolerances, derived and not measured.  A cosine is a d-term dot product with sum |a_k b_k| <= |a| |b|, divided by
two norms (each a d-term sum and a square root) — at most (d + 4) roundings of relative size u, on a value of
magnitude <= 1; the diversity adds a mean of P = m (m - 1) / 2 such terms, <= P more roundings:
  TOL64(d, P) = 2 (d + 4 + P) 2^-53   device f64 against this f64 restatement (one bound for each side); P = 0 for
                                       a single cosine of `sim`
  TOL32(d, P) =   (d + 4 + P) 2^-24   the reference, which works in f32, against this restatement
"""
import numpy as np

CLIP = 1e-8
COLUMNS = ("mean", "std", "median", "min", "max", "count_nonnull", "total_rows", "pct_missing")


def TOL64(d, pairs=0):
    return 2.0 * (d + 4 + pairs) * 2.0 ** -53


def TOL32(d, pairs=0):
    return (d + 4 + pairs) * 2.0 ** -24


def popcount(a):
    a = np.asarray(a, np.uint64)
    return np.array([bin(int(x)).count("1") for x in a.reshape(-1)], np.int64).reshape(a.shape)


def bits_to_names(b):
    """One uint64 bitset -> the reference's list of label names."""
    return [f"L{j}" for j in range(64) if (int(b) >> j) & 1]


def list_diversity_ref(G, idx, bits=None, idx_base=0):
    """G (n, d) rows (f32 or f16: upcast exactly); idx (B, k) int64 global indices; bits (n,) uint64 or None.
    -> dict(emb_div f64 (B,), label_div f64 (B,) or None, n_valid int32 (B,), sim f64 (B, k, k), pairs int64 (B,))."""
    G = np.asarray(G).astype(np.float64)
    n = G.shape[0]
    idx = np.asarray(idx, np.int64)
    B, k = idx.shape
    norm = np.maximum(np.sqrt((G * G).sum(1)), CLIP) if n else np.zeros(0)
    emb = np.zeros(B)
    lab = None if bits is None else np.zeros(B)
    nv = np.zeros(B, np.int32)
    sim = np.zeros((B, k, k))
    pairs = np.zeros(B, np.int64)
    for q in range(B):
        pos = np.array([p for p in range(k) if idx_base <= idx[q, p] < idx_base + n], np.int64)
        rows = idx[q, pos] - idx_base
        m = len(pos)
        nv[q] = m
        if m:
            R = G[rows]
            sim[q][np.ix_(pos, pos)] = (R @ R.T) / np.outer(norm[rows], norm[rows])
        if m >= 2:
            iu = np.triu_indices(m, k=1)
            pairs[q] = len(iu[0])
            emb[q] = 1.0 - float(sim[q][np.ix_(pos, pos)][iu].sum()) / float(pairs[q])
        if bits is not None and m:
            b = np.asarray(bits, np.uint64)[rows]
            u = bin(int(np.bitwise_or.reduce(b))).count("1")
            sizes = popcount(b)
            s, c = int(sizes.sum()), int((sizes > 0).sum())
            lab[q] = 0.0 if c == 0 else float(u) / (float(s) / float(c))
    return {"emb_div": emb, "label_div": lab, "n_valid": nv, "sim": sim, "pairs": pairs}


def summary_ref(values):
    """One metric's row of summary_all_metrics in plain numpy (NaN = missing, sample std)."""
    v = np.asarray(values, np.float64).reshape(-1)
    ok = v[~np.isnan(v)]
    cnt, total, nan = len(ok), len(v), float("nan")
    return {"mean": float(ok.mean()) if cnt else nan, "std": float(ok.std(ddof=1)) if cnt > 1 else nan,
            "median": float(np.median(ok)) if cnt else nan, "min": float(ok.min()) if cnt else nan,
            "max": float(ok.max()) if cnt else nan, "count_nonnull": cnt, "total_rows": total,
            "pct_missing": 100.0 * (1.0 - cnt / total) if total else nan}


def fixture_lists(gold):
    """The fixture's lists as [(dim, idx (k,) int64 rows of G_<dim>)], in recorded order."""
    off, flat, dims = gold["list_off"], gold["list_idx"], gold["list_dim"]
    return [(int(dims[i]), flat[off[i]:off[i + 1]].astype(np.int64)) for i in range(len(dims))]
