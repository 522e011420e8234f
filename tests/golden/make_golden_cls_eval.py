"""Golden generator for the classifier evaluation: what scikit-learn returns for one synthetic case, written to
tests/golden/cls_eval.npz — data only.  Run by hand where scikit-learn is installed (recorded with 1.7.2), never by
the test suite, bench.py or smoke(); the tests read the fixture and do not import sklearn.

The case: N = 257 samples, C = 43 classes, sigmoid probabilities (float32), labels with prevalence 0.3, and four
special classes — 5: scores on 8 levels (ties), 6: all scores equal, 7: no positives, 8: all positives.
Recorded, with the calls of src/Evaluate/eval_on_test.py:
  auroc (C,)        roc_auc_score per class, NaN where a class has no positives or no negatives (safe_roc_auc)
  ap (C,), micro_ap average_precision_score per class (NaN under the same rule: safe_avg_precision) / average='micro'
  pr_thresholds     precision_recall_curve's thresholds of every class, concatenated (float32, as the scores are),
  pr_offsets        class c's are pr_thresholds[pr_offsets[c]:pr_offsets[c + 1]]
  best_ts (C,)      thresholds[argmax(2 p r / (p + r + 1e-8))] per class (_find_best_thresholds)
  preds at `scores > best_ts`: prec / rec / f1 (C,) (average=None, zero_division=0) and their macro / micro forms,
  tp / fp / fn (C,) from multilabel_confusion_matrix.
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import cls_eval_ref as R  # noqa: E402

N, C, SEED = 257, 43, 4301
TIES, TIED, NOPOS, ALLPOS = 5, 6, 7, 8


def case():
    S = R.scores("distinct", N, C, SEED)
    S[:, TIES] = R.scores("ties8", N, 1, SEED + 1)[:, 0]
    S[:, TIED] = 0.25
    Y = (np.random.default_rng(SEED + 2).random((N, C)) < 0.3).astype(np.uint8)
    Y[:, NOPOS] = 0
    Y[:, ALLPOS] = 1
    return S, Y


def main():
    import sklearn
    from sklearn.metrics import (average_precision_score, f1_score, multilabel_confusion_matrix,
                                 precision_recall_curve, precision_score, recall_score, roc_auc_score)
    import warnings
    warnings.simplefilter("ignore")
    S, Y = case()
    one_sided = (Y.sum(0) == 0) | (Y.sum(0) == N)
    auroc = np.array([np.nan if one_sided[c] else roc_auc_score(Y[:, c], S[:, c]) for c in range(C)])
    ap = np.array([np.nan if one_sided[c] else average_precision_score(Y[:, c], S[:, c]) for c in range(C)])
    thr, off, best = [], [0], []
    for c in range(C):
        p, r, t = precision_recall_curve(Y[:, c], S[:, c])
        f1 = 2 * p * r / (p + r + 1e-8)
        best.append(float(t[f1.argmax()]))
        assert np.array_equal(t.astype(np.float32), t)
        thr.append(t.astype(np.float32))
        off.append(off[-1] + len(t))
    best = np.array(best)
    pred = (S > best[None, :]).astype(int)
    kw = dict(zero_division=0)
    mcm = multilabel_confusion_matrix(Y, pred)
    out = dict(
        scores=S, labels=Y, auroc=auroc, ap=ap, micro_ap=np.float64(average_precision_score(Y, S, average="micro")),
        pr_thresholds=np.concatenate(thr), pr_offsets=np.array(off, np.int64), best_ts=best,
        prec=precision_score(Y, pred, average=None, **kw), rec=recall_score(Y, pred, average=None, **kw),
        f1=f1_score(Y, pred, average=None, **kw),
        macro=np.array([precision_score(Y, pred, average="macro", **kw), recall_score(Y, pred, average="macro", **kw),
                        f1_score(Y, pred, average="macro", **kw)]),
        micro=np.array([precision_score(Y, pred, average="micro", **kw), recall_score(Y, pred, average="micro", **kw),
                        f1_score(Y, pred, average="micro", **kw)]),
        tp=mcm[:, 1, 1].astype(np.int64), fp=mcm[:, 0, 1].astype(np.int64), fn=mcm[:, 1, 0].astype(np.int64),
        special=np.array([TIES, TIED, NOPOS, ALLPOS], np.int64), sklearn_version=np.array(sklearn.__version__))
    path = HERE / "cls_eval.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, path.stat().st_size, "bytes; sklearn", sklearn.__version__)


if __name__ == "__main__":
    main()
