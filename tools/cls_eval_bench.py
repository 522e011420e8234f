"""Timing of the classifier evaluation (ops.cls_eval = mmr_cls_eval, csrc/cls_eval.hip; metrics.
classification_metrics = that call + packing the labels + one host sync) at 100k x 43 and 4k x 43 against two
baselines computing the same quantities (per class and micro: A, the AP sum, the best-F1 threshold, tp / fp / fn):
  torch      a restatement on the same GPU: torch.sort + gather + cumsum + cummax along the contiguous
             dimension of the transposed (C, N) scores (and of the flattened pairs), timed here
  sklearn    eval_on_test's calls on the CPU (roc_auc_score, average_precision_score per class and micro,
             precision_recall_curve per class, precision / recall / f1_score), where scikit-learn is installed
One process, warmed, device events around `iters` calls, the forms interleaved per round, median over the rounds
(sklearn: host clock, once).  The torch restatement's sums are checked against the device's before timing.
Diagnostic only.
usage: python tools/cls_eval_bench.py [rounds] [--out FILE]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmr_amd import metrics, ops  # noqa: E402


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def torch_curve(s, y):
    """Rows of s (k, n) f32 / y (k, n) int64 (one segment per row, sorted along the contiguous dimension) -> A (k,),
    ap_sum (k,), best threshold (k,), n_pos (k,)."""
    n = s.shape[1]
    srt, idx = torch.sort(s, dim=1, descending=True)
    lab = torch.gather(y, 1, idx)
    tp = lab.cumsum(1)
    rank = torch.arange(1, n + 1, device=s.device, dtype=torch.int64)[None, :]
    fp = rank - tp
    end = torch.ones_like(lab, dtype=torch.bool)
    end[:, :-1] = srt[:, 1:] != srt[:, :-1]
    zero = torch.zeros_like(tp[:, :1])
    # tp / fp at the previous group end: both are non-decreasing, so a running max of the end values
    tp_prev = torch.cat([zero, torch.cummax(torch.where(end, tp, zero), 1).values[:, :-1]], 1)
    fp_prev = torch.cat([zero, torch.cummax(torch.where(end, fp, zero), 1).values[:, :-1]], 1)
    dtp, dfp = tp - tp_prev, fp - fp_prev
    A = torch.where(end, dfp * (2 * tp_prev + dtp), zero).sum(1)
    p = tp.double() / rank.double()
    ap = torch.where(end, dtp.double() * p, torch.zeros_like(p[:, :1])).sum(1)
    P = tp[:, -1]
    r = torch.where(P[:, None] > 0, tp.double() / P[:, None].clamp(min=1).double(), torch.ones_like(p))
    f1 = torch.where(end, 2 * p * r / (p + r + 1e-8), torch.full_like(p, -1.0))
    best = n - 1 - torch.argmax(f1.flip(1), dim=1)  # the lowest score among equal f1
    return A, ap, torch.gather(srt, 1, best[:, None])[:, 0], P


def torch_eval(s, y):
    A, ap, thr, P = torch_curve(s.t().contiguous(), y.t().contiguous())
    mA, map_, _, mP = torch_curve(s.reshape(1, -1), y.reshape(1, -1))
    pred = s > thr[None, :]
    pos = y != 0
    conf = torch.stack([(pred & pos).sum(0), (pred & ~pos).sum(0), (~pred & pos).sum(0)], 1)
    return A, ap, thr, P, mA, map_, conf


def sklearn_eval(S, Y):
    import warnings

    from sklearn.metrics import (average_precision_score, f1_score, precision_recall_curve, precision_score,
                                 recall_score, roc_auc_score)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        C = S.shape[1]
        best = []
        for c in range(C):
            p, r, t = precision_recall_curve(Y[:, c], S[:, c])
            best.append(t[(2 * p * r / (p + r + 1e-8)).argmax()])
        pred = (S > np.array(best)[None, :]).astype(int)
        ok = [c for c in range(C) if 0 < Y[:, c].sum() < len(Y)]
        out = [[roc_auc_score(Y[:, c], S[:, c]) for c in ok], [average_precision_score(Y[:, c], S[:, c]) for c in ok],
               average_precision_score(Y, S, average="micro")]
        for avg in (None, "macro", "micro"):
            out += [f(Y, pred, average=avg, zero_division=0) for f in (precision_score, recall_score, f1_score)]
    return out


def main(rounds, out_path):
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    for n, c in ((100_000, 43), (4_000, 43)):
        g = np.random.default_rng(n)
        S = (1.0 / (1.0 + np.exp(-g.normal(size=(n, c)) * 2.0))).astype(np.float32)
        Y = (g.random((n, c)) < 0.1).astype(np.int64)
        s, y = torch.from_numpy(S).cuda(), torch.from_numpy(Y).cuda()
        bits, _ = metrics.label_bits(y, c, s.device)
        dev = ops.cls_eval(s, bits, c)
        ref = torch_eval(s, y)
        assert torch.equal(dev["counts"][:c, 2], ref[0]) and torch.equal(dev["counts"][c, 2], ref[4][0])
        assert torch.equal(dev["best_thr"][:c], ref[2]) and torch.equal(dev["confusion"][:c], ref[6])
        assert ((dev["ap_sum"][:c] - ref[1]).abs() <= n * 2.0 ** -52 * ref[3]).all()
        iters = 5 if n >= 50_000 else 20
        forms = {"ops.cls_eval (device only)": lambda: ops.cls_eval(s, bits, c),
                 "classification_metrics (labels packed, host sync)": lambda: metrics.classification_metrics(y, s),
                 "torch restatement (sort + cumsum, same GPU)": lambda: torch_eval(s, y)}
        res = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                res[k].append(timeit(fn, iters))
        say(f"N={n} C={c}  workspace {ops._L().mmr_cls_eval_work_bytes(n, c)} B  ({rounds} rounds x {iters} calls)")
        for k, v in res.items():
            say(f"  {k:52s} median {statistics.median(v):9.3f} ms   rounds " + " ".join(f"{t:9.3f}" for t in v))
        try:
            import sklearn
            t0 = time.perf_counter()
            sklearn_eval(S, Y)
            say(f"  {'scikit-learn ' + sklearn.__version__ + ' on the CPU (host clock, one call)':52s} "
                f"{(time.perf_counter() - t0) * 1e3:16.3f} ms")
        except ImportError:
            say("  scikit-learn: not installed here, not measured")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    main(int(args[0]) if args else 5, out)
