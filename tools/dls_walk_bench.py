"""Times the batched DLS walk on the device (DLSRetrievalEngine.retrieve_batch / mmr_index_dls_walk) against the
host walk (DLSRetrievalEngine.retrieve, one query per call) and the exact search, on one synthetic gallery.

Gallery: synthetic.labelled_gallery(N, D) (default 100k x 768), link graph link_graph(0.5, 10) built on the device.
Per batch size B in {1, 16, 256}, with K = 5 and the reference's defaults (seed_size 5, max_steps 100,
candidate_multiplier 10):
  walk     device time of one mmr_index_dls_walk call on device tensors, from device events around `--reps` back to
           back calls, `--repeats` times after a warm-up: median and the min .. max spread; per query = / B
  batch    host wall time of retrieve_batch(numpy Q, explicit seeds) -> numpy, synchronised (upload, launch, download)
  host     host wall time per query of the retrieve() loop over min(B, --host-queries) of the same queries and seeds
  search   device time of MI355XRetrievalEngine.search at the same B and K (the exact scan), measured like `walk`
  steps / visited: means over the batch of the walk's counted steps and visited rows
Seeds are drawn before any timed region.  The walks of both paths are compared (identical id lists) before timing.

    python tools/dls_walk_bench.py --out profiles/dls_walk.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd  # noqa: E402
from mmr_amd import synthetic  # noqa: E402


def device_us(fn, reps, repeats, warmup):
    """Median, min, max device microseconds per call of fn over `repeats` windows of `reps` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def wall_us(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-queries", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dls_walk_bench needs a GPU: no timing is taken on the CPU")

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    G, _ = synthetic.labelled_gallery(a.n, a.d, synthetic.SEED)
    Qall, _ = synthetic.labelled_gallery(max(a.batches), a.d, synthetic.SEED + 2)
    eng = mmr_amd.DLSRetrievalEngine(embs=G, ids=[str(i) for i in range(a.n)], link_threshold=0.5, max_links=10)
    links = [len(x) for x in eng.link_graph]
    say(f"# DLS walk: device batch walk vs host walk vs exact search; {torch.cuda.get_device_name(0)}")
    say(f"# gallery labelled_gallery({a.n}, {a.d}), link_graph(0.5, 10): mean {np.mean(links):.2f} links per row, "
        f"{sum(1 for x in links if x == 0)} rows without links; set-up {time.perf_counter() - t0:.1f} s")
    say(f"# K={a.k} seed_size=5 max_steps=100 candidate_multiplier=10; device times: median [min .. max] of "
        f"{a.repeats} windows of {a.reps} calls after {a.warmup} warm-up calls")
    nbr = eng._device_graph()
    for B in a.batches:
        Q = Qall[:B]
        seeds = eng.draw_seeds(B, 5, seed=[synthetic.SEED + i for i in range(B)])   # outside every timed region
        qd = torch.from_numpy(Q).cuda()
        sd = torch.from_numpy(seeds).cuda()
        idx, sc, st, vis = eng.index.dls_walk(qd, nbr, sd, a.k, r=max(10 * a.k, 5), want_stats=True)
        idx = idx.cpu().numpy()
        nh = min(B, a.host_queries)
        t0 = time.perf_counter()
        host = [eng.retrieve(Q[i], K=a.k, seed=synthetic.SEED + i)[0] for i in range(nh)]
        host_us = (time.perf_counter() - t0) * 1e6 / nh
        same = sum([str(j) for j in idx[i] if j >= 0] == host[i] for i in range(nh))
        w = device_us(lambda: eng.index.dls_walk(qd, nbr, sd, a.k, r=max(10 * a.k, 5)), a.reps, a.repeats, a.warmup)
        s = device_us(lambda: eng.index.search(qd, a.k), a.reps, a.repeats, a.warmup)
        e = wall_us(lambda: eng.retrieve_batch(Q, K=a.k, seeds=seeds), a.repeats, a.warmup)
        say(f"B={B:4d}  walk {w[0]:9.1f} us [{w[1]:.1f} .. {w[2]:.1f}] = {w[0] / B:8.2f} us/query | "
            f"batch (numpy in/out, wall) {e[0]:9.1f} us [{e[1]:.1f} .. {e[2]:.1f}] | "
            f"host retrieve() {host_us:9.1f} us/query over {nh} ({same}/{nh} id lists identical) | "
            f"exact search {s[0]:9.1f} us [{s[1]:.1f} .. {s[2]:.1f}] = {s[0] / B:8.2f} us/query | "
            f"mean steps {st.float().mean().item():.1f} (max {int(st.max())}), mean visited "
            f"{vis.float().mean().item():.1f} (max {int(vis.max())})")
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
