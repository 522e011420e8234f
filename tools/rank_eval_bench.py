"""Timing of the full-ranking label evaluation (GalleryIndex.rank_eval = mmr_index_best_relevant +
mmr_index_count_ahead, csrc/rank_eval.hip) and of MI355XRetrievalEngine.evaluate (one top-10 search + rank_eval +
the list metrics) at Q = 256 and Q = 2048 over a 100k x 768 Gaussian gallery with 1-3 of 43 labels per row, for the
f32 index and the native fp16 index.  One process, device events, medians over several rounds; the achieved f64
FLOP/s of rank_eval counts its two passes of 2 Q N D each, against the vendor's 78.6 TF f64-matrix figure (not
measured on this hardware by this project).  Diagnostic only.
usage: python tools/rank_eval_bench.py [rounds] [N]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmr_amd import MI355XRetrievalEngine, synthetic  # noqa: E402

PEAK_F64_MATRIX = 78.6e12


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


def bits(n, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, synthetic.NUM_LABELS, size=(n, 3)).astype(np.uint64)
    keep = np.arange(3)[None, :] < rng.integers(1, 4, size=n)[:, None]
    return np.bitwise_or.reduce(np.where(keep, np.uint64(1) << lab, np.uint64(0)), axis=1)


def main(rounds, N, D=768):
    G = synthetic.gauss_gallery(N, D, synthetic.SEED)
    gb = torch.from_numpy(bits(N, 7).view(np.int64)).cuda()
    ids = [str(i) for i in range(N)]
    for dtype in ("fp32", "fp16"):
        eng = MI355XRetrievalEngine(embs=G.astype(np.float16) if dtype == "fp16" else G, ids=ids, dtype=dtype)
        for Q in (256, 2048):
            q = torch.from_numpy(synthetic.gauss_gallery(Q, D, synthetic.SEED + 1)).cuda()
            qb = torch.from_numpy(bits(Q, 8).view(np.int64)).cuda()
            iters = 8 if Q <= 256 else 3
            forms = {"rank_eval": lambda: eng.index.rank_eval(q, qb, gb),
                     "evaluate": lambda: eng.evaluate(q, qb, gb, ks=(1, 5, 10)),
                     "search K=10": lambda: eng.index.search(q, 10)}
            res = {k: [] for k in forms}
            for _ in range(rounds):
                for k, fn in forms.items():
                    res[k].append(timeit(fn, iters))
            fr = eng.index.rank_eval(q, qb, gb)[0]
            work = eng.index._rank_args(q, None)[1].numel()
            print(f"{dtype} index N={N} D={D} Q={Q}  workspace {work} B  first_rank mean {fr.double().mean().item():.1f} "
                  f"max {int(fr.max().item())}")
            for k, v in res.items():
                med = statistics.median(v)
                extra = ""
                if k == "rank_eval":
                    fl = 2 * 2.0 * Q * N * D / (med * 1e-3)
                    extra = f"   {fl / 1e12:6.2f} TF f64 = {100 * fl / PEAK_F64_MATRIX:5.1f} % of 78.6 TF"
                print(f"  {k:12s} median {med:9.3f} ms   rounds " + " ".join(f"{t:9.3f}" for t in v) + extra, flush=True)
        eng.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    main(int(args[0]) if args else 3, int(args[1]) if len(args) > 1 else 100_000)
