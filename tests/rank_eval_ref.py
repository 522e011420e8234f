"""Numpy f64 reference of the full-ranking label evaluation (mmr_index_best_relevant /
mmr_index_count_ahead; compute_ranking_metrics, src/Evaluate/retrieval_overlap.py:84-115), built on
oracle.knn.exact_scores, plus the generators the CPU and GPU tests share.

Order: score desc, then global index (idx_base + row) asc.  Row g is relevant to query q iff
(g_bits[g] & q_bits[q]) != 0; the row whose global index is exclude[q] does not exist for q.

TOL = 1e-12 is derived, not measured: an f64 dot product of D <= 1088 terms of unit scale errs by at most
D * 2^-53 ~ 1.2e-13 in either implementation, whatever its summation order, and the cosine's two
roundings add a few ulp — so two exact-arithmetic implementations agree on every score to well within 1e-12.
"""
import numpy as np

from oracle import knn as oknn

TOL = 1e-12
NUM_LABELS = 43


def scores(Q, G):
    """(Q, N) f64 cosine of the raw rows, 0 where a norm is 0."""
    return oknn.exact_scores(np.asarray(Q, np.float32), np.asarray(G, np.float32))


def _masks(S, q_bits, g_bits, exclude, idx_base):
    nq, n = S.shape
    gidx = np.arange(n, dtype=np.int64) + idx_base
    ex = np.full(nq, -1, np.int64) if exclude is None else np.asarray(exclude, np.int64)
    exists = gidx[None, :] != ex[:, None]
    rel = None
    if q_bits is not None:
        rel = ((np.asarray(g_bits, np.uint64)[None, :] & np.asarray(q_bits, np.uint64)[:, None]) != 0) & exists
    return gidx, exists, rel


def best_relevant_ref(S, q_bits, g_bits, exclude=None, idx_base=0):
    """From a score matrix S (Q, n) of rows [idx_base, idx_base + n): (idx (Q,) global, -1 = none; score, 0.0 when
    none; n_rel) — the exact (score desc, index asc) first relevant row."""
    gidx, _, rel = _masks(S, q_bits, g_bits, exclude, idx_base)
    nq = S.shape[0]
    idx, sc = np.full(nq, -1, np.int64), np.zeros(nq)
    for q in range(nq):
        c = np.nonzero(rel[q])[0]
        if len(c):
            b = c[np.lexsort((c, -S[q, c]))[0]]
            idx[q], sc[q] = gidx[b], S[q, b]
    return idx, sc, rel.sum(1).astype(np.int64)


def count_ahead_ref(S, ref_idx, ref_score, exclude=None, idx_base=0):
    """Rows of S's index ranked strictly ahead of (ref_score, ref_idx), the excluded row left out; 0 for ref_idx < 0."""
    gidx, exists, _ = _masks(S, None, None, exclude, idx_base)
    ri, rs = np.asarray(ref_idx, np.int64)[:, None], np.asarray(ref_score, np.float64)[:, None]
    ahead = exists & ((S > rs) | ((S == rs) & (gidx[None, :] < ri))) & (ri >= 0)
    return ahead.sum(1).astype(np.int64)


def rank_eval_ref(Q, G, q_bits, g_bits, exclude=None, idx_base=0, tol=TOL):
    """dict: S (Q, N) scores; n_rel; best_idx (global, -1) / best_score of the exact order; rank = the exact
    first-relevant rank (0 = none); [lo, hi] = the ranks an implementation whose scores err by < tol may return:
    lo = 1 + #{s > s_b + tol}, hi = 1 + #{j != b : s >= s_b - tol}, the excluded row out of both."""
    S = scores(Q, G)
    bi, bs, nrel = best_relevant_ref(S, q_bits, g_bits, exclude, idx_base)
    gidx, exists, _ = _masks(S, q_bits, g_bits, exclude, idx_base)
    has = bi >= 0
    rank = np.where(has, count_ahead_ref(S, bi, bs, exclude, idx_base) + 1, 0)
    lo = np.where(has, 1 + (exists & (S > bs[:, None] + tol)).sum(1), 0)
    hi = np.where(has, 1 + (exists & (gidx[None, :] != bi[:, None]) & (S >= bs[:, None] - tol)).sum(1), 0)
    return dict(S=S, n_rel=nrel, best_idx=bi, best_score=bs, rank=rank.astype(np.int64), lo=lo.astype(np.int64),
                hi=hi.astype(np.int64))


def summary_ref(first_rank, rel_top, n_rel, k):
    """(mrr, hit@k, recall@k) of compute_ranking_metrics from first ranks, the top list's flags and n_rel."""
    fr = np.asarray(first_rank)
    rr = np.where(fr > 0, 1.0 / np.maximum(fr, 1), 0.0)
    hit = ((fr > 0) & (fr <= k)).sum() / len(fr)
    rec = np.where(n_rel > 0, rel_top[:, :k].sum(1) / np.maximum(n_rel, 1), 0.0)
    return float(rr.mean()), float(hit), float(rec.mean())


def sparse_bits(n, seed, nlab=NUM_LABELS):
    """1-2 of `nlab` random labels per row as uint64 bitsets: first relevant ranks are deep."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, nlab, size=n).astype(np.uint64)
    b = rng.integers(0, nlab, size=n).astype(np.uint64)
    two = rng.random(n) < 0.5
    return (np.uint64(1) << a) | np.where(two, np.uint64(1) << b, np.uint64(0))


def gauss(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)


def sparse_labels(n, seed, nlab=NUM_LABELS):
    """sparse_bits as the reference's (n, 43) multi-hot matrix."""
    b = sparse_bits(n, seed, nlab)
    return ((b[:, None] >> np.arange(nlab, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
