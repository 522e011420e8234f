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
`classification_metrics` / `find_best_thresholds` are the classifier's evaluation
(src/Evaluate/eval_on_test.py: per-class AUROC, AP, best-F1 thresholds, precision / recall / F1, macro
and micro aggregates) from the exact sums ops.cls_eval computes on the device.
`compute_embedding_diversity` / `compute_label_diversity_from_labels` are the host mirrors of
src/Evaluate/retrieval_diversity_compute.py:171-194 in f64 (the device computes them for whole batches of
lists: GalleryIndex.list_diversity, the engines' diversity()); `diversity_summary` is one metric's row of
its summary_all_metrics (:142-166).
`compare_maps` is src/Helpers/helper.py:173-209 (Pearson, Spearman, top-k IoU of two heat maps) for device
tensors, single maps or stacks of pairs, through ops.map_alignment (csrc/map_align.hip).
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


# ---------------------------------------------------------------- classifier evaluation (eval_on_test.py)
def label_bits(y_true, num_classes, device):
    """Labels of N samples -> ((N,) int64 tensor on `device` carrying the uint64 bitsets, a 0-d bool tensor: some
    dense entry was not 0 / 1).  y_true: (N, C) array / tensor of {0, 1}, or (N,) bitsets (numpy uint64 / int64
    or a torch int64 tensor, as retrieval.bits_tensor takes them)."""
    C = int(num_classes)
    if not 1 <= C <= 64:
        raise ValueError(f"{C} classes outside 1..64 (label sets are uint64 bitsets)")
    t = y_true if isinstance(y_true, torch.Tensor) else None
    if t is None:
        a = np.asarray(y_true)
        if a.ndim == 1:
            a = np.ascontiguousarray(a)
            a = a.view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64)
        elif a.dtype == np.uint64 or a.dtype == object:
            a = a.astype(np.int64)
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a if a.flags.writeable else a.copy())
    t = t.to(device)
    if t.dim() == 1:
        return t.to(torch.int64), torch.zeros((), dtype=torch.bool, device=t.device)
    if t.dim() != 2 or t.shape[1] != C:
        raise ValueError(f"labels must be (N, {C}) of 0 / 1 or (N,) bitsets, got {tuple(t.shape)}")
    one = t != 0
    bad = (one & (t != 1)).any()
    shifts = torch.arange(C, dtype=torch.int64, device=t.device)
    # disjoint bits: the sum is the bitwise or (bit 63 wraps into the sign bit, which is the uint64's top bit)
    return torch.bitwise_left_shift(one.to(torch.int64), shifts[None, :]).sum(dim=1), bad


def _scores_tensor(y_score, device=None):
    if isinstance(y_score, torch.Tensor):
        t = y_score if y_score.is_cuda or device is None else y_score.to(device)
        t = t if t.is_cuda else t.to("cuda")
    else:
        a = np.ascontiguousarray(np.asarray(y_score, dtype=np.float32))
        t = torch.from_numpy(a if a.flags.writeable else a.copy()).to(device or "cuda")
    if t.dim() != 2:
        raise ValueError(f"scores must be (N, C), got {tuple(t.shape)}")
    return t.to(torch.float32)


def _safe_div(num, den):
    """num / den in f64, 0 where den == 0 (sklearn's zero_division=0)."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den != 0)


def _nanmean(v):
    v = np.asarray(v, np.float64)
    ok = ~np.isnan(v)
    return float(v[ok].mean()) if ok.any() else float("nan")


def classification_metrics(y_true, y_score, thresholds=None, label_names=None):
    """eval_on_test's metrics dict (src/Evaluate/eval_on_test.py:130-207; Trainner/train.py:621-681), computed on
    the device by ops.cls_eval (csrc/cls_eval.hip) and derived in f64 from its integer outputs with one host sync.

    y_score (N, C): probabilities or logits, numpy or torch (taken as float32, as the reference's sigmoid
    outputs are; moved to the GPU when not there); y_true: (N, C) of {0, 1}, or (N,) uint64 label bitsets.
    thresholds: None — the per-class best-F1 thresholds of _find_best_thresholds (precision_recall_curve's
    thresholds, f1 = 2 p r / (p + r + 1e-8), argmax, i.e. the lowest score among equal f1) — or a scalar / (C,)
    vector of fixed ones (use_fixed_threshold).  Predictions are `score > threshold`.
    -> num_samples, num_classes, macro_auc, macro_ap (nanmean over classes; a class without positives or without
    negatives is NaN: safe_roc_auc / safe_avg_precision), macro_f1 / macro_prec / macro_rec (mean over classes,
    zero_division=0), micro_prec / micro_rec / micro_f1 (summed counts), micro_ap (AP of the N C flattened pairs),
    per_class: labels, auroc, ap, prec, rec, f1, thresholds (lists of float), n_pos (list of int).
    A NaN / infinite score raises ValueError, as sklearn does."""
    from . import ops
    s = _scores_tensor(y_score)
    N, C = (int(v) for v in s.shape)
    if label_names is not None and len(label_names) != C:
        raise ValueError(f"label_names has {len(label_names)} entries for {C} classes")
    if len(y_true) != N:
        raise ValueError(f"labels of {len(y_true)} samples for {N} score rows")
    fixed = None
    if thresholds is not None:
        t = thresholds.detach().cpu().numpy() if isinstance(thresholds, torch.Tensor) else np.asarray(thresholds)
        t = t.astype(np.float32)
        if t.ndim == 0:
            t = np.full((C,), t, np.float32)
        if t.shape != (C,):
            raise ValueError(f"thresholds must be a scalar or have shape ({C},), got {t.shape}")
        if not np.isfinite(t).all():
            raise ValueError("thresholds must be finite")
        fixed = torch.from_numpy(t)
    bits, bad = label_bits(y_true, C, s.device)
    r = ops.cls_eval(s, bits, C, fixed)
    words = torch.cat([r["counts"].flatten(), r["confusion"].flatten(), r["nonfinite"], r["ap_sum"].view(torch.int64),
                       r["best_f1"].view(torch.int64), r["best_thr"].view(torch.int32).to(torch.int64),
                       bad.to(torch.int64).reshape(1)]).cpu().numpy()  # the one host sync
    R = C + 1
    o = np.cumsum([0, 4 * R, 3 * R, 1, R, R, R, 1])
    counts, conf = words[o[0]:o[1]].reshape(R, 4), words[o[1]:o[2]].reshape(R, 3)
    if words[o[2]] != 0:
        raise ValueError(f"classification_metrics: {int(words[o[2]])} scores are NaN or infinite")
    if words[o[6]] != 0:
        raise ValueError("classification_metrics: labels must be 0 or 1")
    ap_sum = words[o[3]:o[4]].copy().view(np.float64)
    best_thr = words[o[5]:o[6]].astype(np.int32).view(np.float32)
    n_pos, n_neg, A = counts[:, 0], counts[:, 1], counts[:, 2]
    both = (n_pos > 0) & (n_neg > 0)
    nan = np.full(R, np.nan)
    auroc = np.divide(A.astype(np.float64), (2 * n_pos * n_neg).astype(np.float64), out=nan.copy(), where=both)
    ap = np.divide(ap_sum, n_pos.astype(np.float64), out=nan.copy(), where=both)
    thr = fixed.numpy() if fixed is not None else best_thr[:C]
    tp, fp, fn = conf[:C, 0], conf[:C, 1], conf[:C, 2]
    prec, rec, f1 = _safe_div(tp, tp + fp), _safe_div(tp, tp + fn), _safe_div(2 * tp, 2 * tp + fp + fn)
    TP, FP, FN = (int(v) for v in conf[C])
    # micro AP: only "no positives at all" is undefined (sklearn: 0 with a warning; kept as 0)
    micro_ap = float(ap_sum[C] / n_pos[C]) if n_pos[C] > 0 else 0.0
    return {
        "num_samples": N, "num_classes": C,
        "macro_auc": _nanmean(auroc[:C]), "macro_ap": _nanmean(ap[:C]), "macro_f1": float(f1.mean()),
        "micro_ap": micro_ap, "micro_f1": float(_safe_div(2 * TP, 2 * TP + FP + FN)),
        "macro_prec": float(prec.mean()), "macro_rec": float(rec.mean()),
        "micro_prec": float(_safe_div(TP, TP + FP)), "micro_rec": float(_safe_div(TP, TP + FN)),
        "per_class": {"labels": list(label_names) if label_names is not None else list(range(C)),
                      "auroc": [float(x) for x in auroc[:C]], "ap": [float(x) for x in ap[:C]],
                      "prec": [float(x) for x in prec], "rec": [float(x) for x in rec], "f1": [float(x) for x in f1],
                      "thresholds": [float(x) for x in thr], "n_pos": [int(x) for x in n_pos[:C]]},
    }


def find_best_thresholds(y_true, y_score):
    """_find_best_thresholds (eval_on_test.py:29-38; retrieval_overlap.py:40-49) on the device: per class the
    lowest score with the maximal f1 = 2 p r / (p + r + 1e-8) over precision_recall_curve's thresholds -> (C,)
    float32 (a class without positives gets its minimum score, as there)."""
    from . import ops
    s = _scores_tensor(y_score)
    C = int(s.shape[1])
    bits, bad = label_bits(y_true, C, s.device)
    r = ops.cls_eval(s, bits, C)
    flags = torch.cat([r["nonfinite"], bad.to(torch.int64).reshape(1)])
    thr, flags = r["best_thr"][:C].cpu().numpy(), flags.cpu().numpy()
    if flags[0] != 0:
        raise ValueError(f"find_best_thresholds: {int(flags[0])} scores are NaN or infinite")
    if flags[1] != 0:
        raise ValueError("find_best_thresholds: labels must be 0 or 1")
    return thr


def compute_embedding_diversity(embeddings):
    """1 - mean pairwise cosine of the rows (retrieval_diversity_compute.py:171-182), in f64: norms clipped at
    1e-8, the mean over the i < j pairs; None or fewer than 2 rows -> 0.0."""
    if embeddings is None or len(embeddings) < 2:
        return 0.0
    e = np.asarray(embeddings, np.float64)
    normed = e / np.linalg.norm(e, axis=1, keepdims=True).clip(min=1e-8)
    sim = normed @ normed.T
    return float(1.0 - float(np.mean(sim[np.triu_indices(sim.shape[0], k=1)])))


def compute_label_diversity_from_labels(labels_list):
    """Distinct labels of the list / mean label count of its labelled items (retrieval_diversity_compute.py:184-194);
    an empty list or only empty label sets -> 0.0."""
    if not labels_list:
        return 0.0
    all_labels = set(l for lab in labels_list for l in lab)
    sizes_nonzero = [len(lab) for lab in labels_list if len(lab) > 0]
    if not sizes_nonzero:
        return 0.0
    return float(len(all_labels) / float(np.mean(sizes_nonzero)))


def diversity_summary(values):
    """summary_all_metrics' columns (retrieval_diversity_compute.py:142-166) for one metric's per-query values
    (a device tensor costs one host sync; numpy and lists as they are): mean, std (the SAMPLE std, ddof = 1, as
    pandas; NaN with fewer than 2 values), median, min, max over the non-NaN values (NaN when there are none),
    count_nonnull, total_rows, pct_missing.  NaN and None count as missing."""
    if isinstance(values, torch.Tensor):
        v = values.detach().to("cpu", torch.float64).numpy().reshape(-1)
    elif isinstance(values, np.ndarray) and values.dtype.kind in "fiu":
        v = values.astype(np.float64).reshape(-1)
    else:
        v = np.array([np.nan if x is None else x for x in np.asarray(values, dtype=object).reshape(-1)], np.float64)
    total = int(v.shape[0])
    ok = v[~np.isnan(v)]
    cnt = int(ok.shape[0])
    nan = float("nan")
    return {"mean": float(ok.mean()) if cnt > 0 else nan,
            "std": float(ok.std(ddof=1)) if cnt > 1 else nan,
            "median": float(np.median(ok)) if cnt > 0 else nan,
            "min": float(ok.min()) if cnt > 0 else nan,
            "max": float(ok.max()) if cnt > 0 else nan,
            "count_nonnull": cnt, "total_rows": total,
            "pct_missing": 100.0 * (1.0 - cnt / total) if total > 0 else nan}


def iou_key(topk_frac):
    """compare_maps' IoU key (helper.py:208)"""
    return f"iou_top{int(topk_frac * 100)}pct"


def compare_maps(map_a, map_b, topk_frac=0.05):
    """src/Helpers/helper.py:173-209 on the device: map_a, map_b (H, W) — or stacks (P, H, W) compared pair by
    pair — float32 device tensors of equal shape -> {'pearson', 'spearman', f'iou_top{int(topk_frac*100)}pct'}:
    floats for one pair, (P,) float64 numpy arrays for a stack.  Pearson and Spearman are 0.0 when either map is
    constant (:188-190); iou = inter / (union + 1e-8) over the top max(1, int(HW * topk_frac)) pixels, ties
    at the threshold included (np.partition's value, `>=`).  One ops.map_alignment call and one host sync; a
    NaN / infinite pixel raises ValueError."""
    from . import ops
    a, b = torch.as_tensor(map_a), torch.as_tensor(map_b)
    if a.shape != b.shape:
        raise ValueError(f"compare_maps: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    single = a.dim() <= 2
    if single:
        a, b = a.reshape(1, -1), b.reshape(1, -1)
    P = int(a.shape[0])
    maps = torch.cat([a.reshape(P, -1), b.to(a.device).reshape(P, -1)]).to(torch.float32)
    idx = torch.arange(P, dtype=torch.int64, device=maps.device)
    r = ops.map_alignment(maps, idx, idx + P, fracs=(topk_frac,))
    host = {k: r[k].cpu().numpy() for k in ("nonfinite", "inter_union", "pearson", "spearman")}  # the one sync
    if int(host["nonfinite"][0]):
        raise ValueError(f"compare_maps: {int(host['nonfinite'][0])} NaN / infinite pixels")
    iu = host["inter_union"].astype(np.float64)
    out = {"pearson": host["pearson"], "spearman": host["spearman"],
           iou_key(topk_frac): iu[:, 0, 0] / (iu[:, 0, 1] + 1e-8)}
    return {k: float(v[0]) for k, v in out.items()} if single else out
