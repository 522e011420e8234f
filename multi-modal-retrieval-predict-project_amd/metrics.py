"""Retrieval metrics on id lists — same definitions as src/Helpers/retrieval_metrics.py.

precision_at_k  retrieval_metrics.py:4-11
recall_at_k     retrieval_metrics.py:74-79 (the module redefines it; the later, set-based one wins)
average_precision / mean_average_precision  :24-54
mean_reciprocal_rank  :56-72
ndcg_at_k  :81-89 (binary gains, ideal = the same gains sorted, i.e. normalised within the top-k)
Plus `ranking_metrics`, the exact brute-force evaluation of
src/Evaluate/retrieval_overlap.py:84-115 (first-relevant rank -> MRR, hit@k, recall@k over the whole
gallery), computed from top-k indices and label bitsets instead of a Python loop over N.  Its
`first_rank` argument makes it exact; the device supplies it: GalleryIndex.rank_eval /
ShardedIndex.rank_eval rank the WHOLE gallery per query (mmr_index_best_relevant +
mmr_index_count_ahead) and return the first-relevant rank and the relevant count, so
MI355XRetrievalEngine.evaluate's mrr / hit@k / recall@k are compute_ranking_metrics' values at any
gallery size, with or without the test -> test protocol's self-exclusion (contructGT.py:73).
`list_metrics` is the id-list metrics above on device tensors: relevance flags of a ranked list +
the per-query relevant count (recall's and AP's denominator) -> P@k, R@k, AP@k, RR, nDCG@k per query;
`evaluation_summary` turns those and the first ranks into the evaluation's dict.
"""
import math

import numpy as np
import torch


def precision_at_k(retrieved_ids, relevant_ids, k=5):
    rel = set(relevant_ids)
    return sum(1 for r in retrieved_ids[:k] if r in rel) / k


def recall_at_k(retrieved, relevant, k=5):
    if len(relevant) == 0:
        return 0.0
    return len(set(retrieved[:k]) & set(relevant)) / len(set(relevant))


def average_precision(retrieved, relevant, k=None):
    if k is None:
        k = len(retrieved)
    hits, score = 0, 0.0
    for i, r in enumerate(retrieved[:k], start=1):
        if r in relevant:
            hits += 1
            score += hits / i
    return score / len(relevant) if relevant else 0.0


def mean_average_precision(all_retrieved, all_relevant, k=None):
    return float(np.mean([average_precision(r, s, k) for r, s in zip(all_retrieved, all_relevant)]))


def mean_reciprocal_rank(all_retrieved, all_relevant):
    rr = []
    for retrieved, relevant in zip(all_retrieved, all_relevant):
        v = 0.0
        for i, r in enumerate(retrieved, start=1):
            if r in relevant:
                v = 1.0 / i
                break
        rr.append(v)
    return float(np.mean(rr))


def ndcg_at_k(retrieved, relevant, k=5):
    gains = [1 if r in relevant else 0 for r in retrieved[:k]]
    dcg = sum(g / math.log2(i + 2) for i, g in enumerate(gains))
    idcg = sum(g / math.log2(i + 2) for i, g in enumerate(sorted(gains, reverse=True)))
    return dcg / idcg if idcg > 0 else 0.0


def _popcount_nonzero(a):
    return a != 0


def ranking_metrics(topk_idx, query_bits, gallery_bits, k, first_rank=None):
    """retrieval_overlap.py:84-115 from top-k indices.

    topk_idx (Q, >=k) int gallery indices in rank order; query_bits (Q,) / gallery_bits (N,) uint64
    label bitsets (relevance = any shared label).  `first_rank` (Q,) optional: 1-based rank of the
    first relevant gallery item in the full ranking (0 = none); when None it is taken from topk_idx
    (exact when the first relevant item is inside the returned list, else MRR counts 0 for it).
    Returns (mrr, hit@k, recall@k) like compute_ranking_metrics.
    """
    topk_idx = np.asarray(topk_idx)
    qb = np.asarray(query_bits, np.uint64)
    gb = np.asarray(gallery_bits, np.uint64)
    rel_top = _popcount_nonzero(gb[topk_idx] & qb[:, None])             # (Q, K')
    total_rel = _popcount_nonzero(gb[None, :] & qb[:, None]).sum(axis=1)  # (Q,)
    if first_rank is None:
        any_rel = rel_top.any(axis=1)
        first_rank = np.where(any_rel, rel_top.argmax(axis=1) + 1, 0)
    first_rank = np.asarray(first_rank)
    rr = np.where(first_rank > 0, 1.0 / np.maximum(first_rank, 1), 0.0)
    hits = ((first_rank > 0) & (first_rank <= k)).sum()
    rel_k = rel_top[:, :k].sum(axis=1)
    recalls = np.where(total_rel > 0, rel_k / np.maximum(total_rel, 1), 0.0)
    return float(np.mean(rr)), hits / len(qb), float(np.mean(recalls))


def list_metrics(rel_flags, n_rel, k):
    """The id-list metrics per query from relevance flags: rel_flags (Q, K) bool in rank order (True where
    the retrieved item is relevant; distinct items), n_rel (Q,) the number of relevant items in the whole
    gallery, on any device.  The first k entries count.  -> dict of (Q,) f64 tensors:
      p     precision_at_k: hits / k
      r     recall_at_k: hits / n_rel (0 when n_rel == 0)
      ap    average_precision(k): sum over hits of (hits so far / position) / n_rel (0 when n_rel == 0)
      rr    reciprocal rank of the first hit within the first k (0 when none)
      ndcg  ndcg_at_k: binary gains, ideal = the same gains sorted"""
    f = rel_flags[:, :k].to(torch.float64)
    kk = f.shape[1]
    n = n_rel.to(f.device, torch.float64)
    pos = torch.arange(1, kk + 1, dtype=torch.float64, device=f.device)
    hits = f.sum(1)
    has_rel = n > 0
    den = torch.where(has_rel, n, torch.ones_like(n))
    zero = torch.zeros_like(hits)
    ap = (f * f.cumsum(1) / pos).sum(1)
    first = torch.where(f > 0, pos.expand_as(f), torch.full_like(f, float("inf"))).min(1).values if kk else \
        torch.full_like(hits, float("inf"))
    disc = 1.0 / torch.log2(pos + 1.0)
    dcg = (f * disc).sum(1)
    idcg = ((pos.expand_as(f) <= hits[:, None]).to(torch.float64) * disc).sum(1)
    return {"p": hits / k, "r": torch.where(has_rel, hits / den, zero), "ap": torch.where(has_rel, ap / den, zero),
            "rr": 1.0 / first, "ndcg": torch.where(idcg > 0, dcg / torch.where(idcg > 0, idcg, torch.ones_like(idcg)), zero)}


def evaluation_summary(rel_flags, first_rank, n_rel, ks):
    """The evaluation's result dict from a ranked list's relevance flags (Q, K), K >= max(ks) where the gallery
    allows, and the full-ranking first_rank / n_rel (Q,): `mrr` (full ranking), `hit@k`, `recall@k` (the three
    values of compute_ranking_metrics), `p@k`, `map@k`, `ndcg@k` per k, `mrr@K` (first hit within the list, K =
    max(ks)) as floats, plus the per-query `first_rank` / `n_rel` tensors.  One host sync."""
    fr = first_rank.to(torch.float64)
    found = first_rank > 0
    names, vals = ["mrr"], [torch.where(found, 1.0 / torch.where(found, fr, torch.ones_like(fr)), torch.zeros_like(fr))]
    for k in ks:
        m = list_metrics(rel_flags, n_rel, k)
        names += [f"hit@{k}", f"recall@{k}", f"p@{k}", f"map@{k}", f"ndcg@{k}"]
        vals += [(found & (first_rank <= k)).to(torch.float64), m["r"], m["p"], m["ap"], m["ndcg"]]
    K = max(ks)
    names.append(f"mrr@{K}")
    vals.append(list_metrics(rel_flags, n_rel, K)["rr"])
    means = torch.stack([v.mean() if v.numel() else v.sum() for v in vals]).tolist()
    out = dict(zip(names, means))
    out["first_rank"], out["n_rel"] = first_rank, n_rel
    return out
