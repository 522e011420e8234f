"""numpy restatement of the classifier evaluation (csrc/cls_eval.hip, metrics.classification_metrics) — the
semantics of src/Evaluate/eval_on_test.py in integer arithmetic and f64 true division, tests-only.

Per class (and for the N*C flattened pairs, "micro"): scores are ordered by the integer image of their float32
bit pattern (-0 == +0; denormals distinct), equal scores form a tie group, and at each group end
  tp, fp = positives / negatives scoring >= the group's value,  dtp, dfp = the group's own
  A      = sum dfp * (2 * (tp - dtp) + dtp)                 AUROC = A / (2 P Nn)       (NaN when P or Nn is 0)
  ap_sum = sum dtp * (tp / (tp + fp))                       AP    = ap_sum / P         (NaN when P or Nn is 0)
  f1     = (2 * p * r) / ((p + r) + 1e-8), p = tp / (tp + fp), r = tp / P (1.0 when P == 0)
  best threshold = the LOWEST score among those with the maximal f1 (float32).
Predictions are score > threshold; precision / recall / F1 use zero_division = 0.

Error bounds used by the tests: AP sums <= N terms, each <= 1 after the division by P and each rounded by <=
2^-53 relative, in any order, so two correct f64 evaluations differ by <= N * 2^-52 (AP_TOL(n)); AUROC is one
division of two integers that f64 holds exactly at the tested sizes (A <= 2 P Nn < 2^53): bit-equal."""
import numpy as np


def AP_TOL(n):
    return n * 2.0 ** -52


def order_image(s):
    """float32 array -> int64 image, ascending with the score; -0 and +0 share one image."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.int64)
    u = np.where((u & 0x7FFFFFFF) == 0, 0, u)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def image_score(img):
    """The float32 score of an image (the canonical +0 for zero)."""
    img = np.asarray(img, np.int64)
    u = np.where(img & 0x80000000, img ^ 0x80000000, 0xFFFFFFFF - img)
    return u.astype(np.uint32).view(np.float32)


def curve(scores, labels):
    """One segment: scores (n,) float32, labels (n,) 0 / 1 -> dict of its exact sums and the best threshold."""
    img = order_image(scores)
    lab = np.asarray(labels).astype(np.int64)
    order = np.argsort(-img, kind="stable")
    img, lab = img[order], lab[order]
    ends = np.flatnonzero(np.r_[img[1:] != img[:-1], True])
    tp = np.cumsum(lab)[ends]
    fp = (ends + 1) - tp
    dtp, dfp = np.diff(tp, prepend=0), np.diff(fp, prepend=0)
    P, Nn = int(tp[-1]), int(fp[-1])
    A = int((dfp * (2 * (tp - dtp) + dtp)).sum())  # int64: exact below 2^63
    p = tp.astype(np.float64) / (tp + fp).astype(np.float64)
    ap_sum = float(np.cumsum(dtp.astype(np.float64) * p)[-1])  # summed in order
    r = tp.astype(np.float64) / np.float64(P) if P else np.ones(len(tp))
    f1 = (2.0 * p * r) / ((p + r) + 1e-8)
    best = len(f1) - 1 - int(np.argmax(f1[::-1]))  # ends run from the highest score down: the last maximum
    return {"n_pos": P, "n_neg": Nn, "A": A, "n_distinct": len(ends), "ap_sum": ap_sum,
            "best_thr": image_score(img[ends[best]]).reshape(()), "best_f1": float(f1[best])}


def cls_eval_ref(S, Y, thresholds=None):
    """S (N, C) float32, Y (N, C) 0 / 1 -> the device call's outputs as numpy arrays with C + 1 rows (row C: the
    flattened pairs): counts (C + 1, 4) int64, ap_sum, best_thr float32, best_f1, confusion (C + 1, 3) int64."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    Y = np.asarray(Y).astype(np.int64)
    N, C = S.shape
    rows = [curve(S[:, c], Y[:, c]) for c in range(C)] + [curve(S.reshape(-1), Y.reshape(-1))]
    best_thr = np.array([r["best_thr"] for r in rows], np.float32)
    thr = best_thr[:C] if thresholds is None else np.broadcast_to(np.asarray(thresholds, np.float32), (C,))
    pred = S > thr[None, :]
    pos = Y == 1
    conf = np.stack([(pred & pos).sum(0), (pred & ~pos).sum(0), (~pred & pos).sum(0)], 1).astype(np.int64)
    return {"counts": np.array([[r["n_pos"], r["n_neg"], r["A"], r["n_distinct"]] for r in rows], np.int64),
            "ap_sum": np.array([r["ap_sum"] for r in rows]), "best_thr": best_thr,
            "best_f1": np.array([r["best_f1"] for r in rows]),
            "confusion": np.concatenate([conf, conf.sum(0, keepdims=True)]), "thresholds": thr.copy()}


def _div0(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape), where=b != 0)


def _nanmean(v):
    ok = ~np.isnan(v)
    return float(v[ok].mean()) if ok.any() else float("nan")


def metrics_ref(S, Y, thresholds=None):
    """The metrics dict of metrics.classification_metrics from cls_eval_ref's sums."""
    r = cls_eval_ref(S, Y, thresholds)
    C = S.shape[1]
    P, Nn, A = (r["counts"][:, k].astype(np.float64) for k in range(3))
    both = (P > 0) & (Nn > 0)
    nan = np.full(C + 1, np.nan)
    auroc = np.divide(A, 2.0 * P * Nn, out=nan.copy(), where=both)
    ap = np.divide(r["ap_sum"], P, out=nan.copy(), where=both)
    tp, fp, fn = (r["confusion"][:C, k] for k in range(3))
    TP, FP, FN = (int(v) for v in r["confusion"][C])
    prec, rec, f1 = _div0(tp, tp + fp), _div0(tp, tp + fn), _div0(2 * tp, 2 * tp + fp + fn)
    return {"num_samples": S.shape[0], "num_classes": C,
            "macro_auc": _nanmean(auroc[:C]), "macro_ap": _nanmean(ap[:C]), "macro_f1": float(f1.mean()),
            "micro_ap": float(r["ap_sum"][C] / P[C]) if P[C] > 0 else 0.0,
            "micro_f1": float(_div0(2 * TP, 2 * TP + FP + FN)),
            "macro_prec": float(prec.mean()), "macro_rec": float(rec.mean()),
            "micro_prec": float(_div0(TP, TP + FP)), "micro_rec": float(_div0(TP, TP + FN)),
            "per_class": {"labels": list(range(C)), "auroc": auroc[:C].tolist(), "ap": ap[:C].tolist(),
                          "prec": prec.tolist(), "rec": rec.tolist(), "f1": f1.tolist(),
                          "thresholds": [float(x) for x in r["thresholds"]],
                          "n_pos": [int(x) for x in r["counts"][:C, 0]]}}


# ---------------------------------------------------------------- test data (seeded, shared by the CPU and GPU files)
FAMILIES = ("distinct", "ties8", "tied", "logits", "zeros")


def scores(family, n, c, seed):
    """(n, c) float32 scores of one family: distinct sigmoid probabilities; 8 levels; all equal; negative-heavy
    logits; the +-0 / denormal / tiny-normal set."""
    g = np.random.default_rng(seed)
    if family == "distinct":
        return (1.0 / (1.0 + np.exp(-g.normal(size=(n, c)) * 2.0))).astype(np.float32)
    if family == "ties8":
        return (g.integers(0, 8, size=(n, c)) / 8.0).astype(np.float32)
    if family == "tied":
        return np.full((n, c), 0.25, np.float32)
    if family == "logits":
        return (g.normal(size=(n, c)) * 3.0 - 2.0).astype(np.float32)
    if family == "zeros":
        pool = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00000002, 0x007FFFFF, 0x807FFFFF,
                         0x00800000, 0x80800000, 0x3F800000, 0xBF800000], np.uint32).view(np.float32)
        return pool[g.integers(0, len(pool), size=(n, c))]
    raise ValueError(family)


def labels(n, c, seed, prevalence=0.3):
    """(n, c) uint8 labels; with c >= 4 class 1 has no positives and class 2 no negatives."""
    g = np.random.default_rng(seed + 7919)
    y = (g.random((n, c)) < prevalence).astype(np.uint8)
    if c >= 4:
        y[:, 1] = 0
        y[:, 2] = 1
    return y


def pack_bits(Y):
    """(N, C <= 64) 0 / 1 -> (N,) uint64 bitsets."""
    Y = np.asarray(Y).astype(np.uint64)
    return (Y << np.arange(Y.shape[1], dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
