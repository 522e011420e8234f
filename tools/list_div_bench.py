"""Times the retrieval-diversity pass on the device (GalleryIndex.list_diversity / mmr_index_list_diversity) against
a torch restatement on the same GPU and against the host loop it replaces, on one synthetic gallery.

Gallery: synthetic.labelled_gallery(N, D) (default 100k x 768) in an MMR_F32 index; the lists are the exact top-K of
B = 256 queries (MI355XRetrievalEngine.search), K in {5, 10, 16, 17, 50, 256}: 16 | 17 are the two sides of the
switch from the one-wave kernel to the tiled one.  Per K:
  device   device time of one list_diversity call (embedding + label diversity + n_valid) on device tensors, from
           device events around `--reps` back to back calls, `--repeats` times after a warm-up: median [min .. max];
           `+sim` the same with the (B, K, K) cosine matrix written too
  torch    the same quantity restated in torch on the same GPU and measured the same way: index_select of the B K
           rows, f64 bmm of the normalised rows, mean of the upper triangle (embedding diversity only)
  host     host wall time of what callers did before: the (B, K) indices to the host, fancy-indexing the host
           gallery, metrics.compute_embedding_diversity per list (embedding diversity only)
  bytes    B K D 4, the gallery bytes one call gathers
The three paths are compared (max |difference| of the embedding diversity) before any timing.

    python tools/list_div_bench.py --out profiles/list_diversity.txt
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
from mmr_amd import metrics, synthetic  # noqa: E402


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


def torch_diversity(Gd, idx):
    """1 - mean pairwise cosine of the listed rows, f64, every entry valid."""
    B, K = idx.shape
    rows = Gd.index_select(0, idx.reshape(-1)).view(B, K, -1).double()
    rows = rows / rows.norm(dim=2, keepdim=True).clamp_min(1e-8)
    sim = torch.bmm(rows, rows.transpose(1, 2))
    iu = torch.triu_indices(K, K, offset=1, device=idx.device)
    return 1.0 - sim[:, iu[0], iu[1]].mean(dim=1)


def host_diversity(G, idx_dev):
    idx = idx_dev.cpu().numpy()
    return np.array([metrics.compute_embedding_diversity(G[row]) for row in idx])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--ks", type=int, nargs="+", default=[5, 10, 16, 17, 50, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("list_div_bench needs a GPU: no timing is taken on the CPU")

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    G, gl = synthetic.labelled_gallery(a.n, a.d, synthetic.SEED)
    Q, _ = synthetic.labelled_gallery(a.batch, a.d, synthetic.SEED + 2)
    eng = mmr_amd.MI355XRetrievalEngine(embs=G, ids=[str(i) for i in range(a.n)])
    gb = torch.from_numpy(synthetic.labels_to_bits(gl).view(np.int64)).cuda()
    Gd, qd = torch.from_numpy(G).cuda(), torch.from_numpy(Q).cuda()
    say(f"# retrieval diversity of retrieved lists: device pass vs torch restatement vs host loop; "
        f"{torch.cuda.get_device_name(0)}")
    say(f"# gallery labelled_gallery({a.n}, {a.d}), B = {a.batch} exact top-K lists; set-up "
        f"{time.perf_counter() - t0:.1f} s")
    say(f"# device times: median [min .. max] of {a.repeats} windows of {a.reps} calls after {a.warmup} warm-up calls; "
        f"host: median wall time of {a.host_repeats} runs")
    for K in a.ks:
        idx = eng.index.search(qd, K)[0]
        emb, lab, nv = eng.index.list_diversity(idx, gb)
        ref_t = torch_diversity(Gd, idx)
        ref_h = host_diversity(G, idx)
        dt = float((emb - ref_t).abs().max())
        dh = float(np.abs(emb.cpu().numpy() - ref_h).max())
        dev = device_us(lambda: eng.index.list_diversity(idx, gb), a.reps, a.repeats, a.warmup)
        dvs = device_us(lambda: eng.index.list_diversity(idx, gb, want_sim=True), a.reps, a.repeats, a.warmup)
        tor = device_us(lambda: torch_diversity(Gd, idx), a.reps, a.repeats, a.warmup)
        hs = []
        for _ in range(a.host_repeats):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            host_diversity(G, idx)
            hs.append((time.perf_counter() - t1) * 1e6)
        host = statistics.median(hs)
        say(f"K={K:4d}  device {dev[0]:8.1f} us [{dev[1]:.1f} .. {dev[2]:.1f}] | +sim {dvs[0]:8.1f} us [{dvs[1]:.1f} .. "
            f"{dvs[2]:.1f}] | torch {tor[0]:8.1f} us [{tor[1]:.1f} .. {tor[2]:.1f}] = {tor[0] / dev[0]:5.1f} x | "
            f"host loop {host:10.1f} us = {host / dev[0]:7.1f} x | gathered {a.batch * K * a.d * 4 / 1e6:6.1f} MB = "
            f"{a.batch * K * a.d * 4 / dev[0] / 1e3:6.1f} GB/s | max |device - torch| {dt:.2e}, |device - host| "
            f"{dh:.2e} | mean diversity {float(emb.mean()):.4f}, label diversity {float(lab.mean()):.3f}, "
            f"n_valid {int(nv.min())}..{int(nv.max())}")
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
