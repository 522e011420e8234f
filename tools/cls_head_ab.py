"""A/B timing of the fused classifier head (ops.classifier_head, csrc/cls_head.hip) against the chain of existing
ops that computes the same logits: two ops.linear_x3 calls with W2 zero-padded to 64 rows (the hidden written and
re-read as a (B, 4D) f32 tensor).  Shapes: B = 256, D = 768 (cfg2) and B = 2048, D = 1024 (cfg5), C = 43.  One
process, device events, the two alternated over several rounds; medians in us, the workspace bytes, and the
largest logit difference between the two (both bf16x3).  With --model: predict() against forward() on the cfg2
bench model with a seeded classifier state (the cost of the added path).  Diagnostic only.
usage: python tools/cls_head_ab.py [rounds] [--model]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mmr_amd import _lib, ops  # noqa: E402


def timeit(fn, iters=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def head_ab(rounds):
    for B, D, C in ((256, 768, 43), (2048, 1024, 43)):
        H = 4 * D
        g = torch.Generator().manual_seed(D + C)
        x = torch.randn(B, D, generator=g).to("cuda")
        w1 = (torch.randn(H, D, generator=g) * D ** -0.5).to("cuda")
        b1 = (0.1 * torch.randn(H, generator=g)).to("cuda")
        w2 = (torch.randn(C, H, generator=g) * H ** -0.5).to("cuda")
        b2 = (0.1 * torch.randn(C, generator=g)).to("cuda")
        cw = ops.ClassifierW(w1, b1, w2, b2)
        w2p, b2p = torch.zeros(64, H, device="cuda"), torch.zeros(64, device="cuda")
        w2p[:C], b2p[:C] = w2, b2
        x1, x2 = ops.X3W(w1), ops.X3W(w2p)
        hid, out = torch.empty(B, H, device="cuda"), torch.empty(B, 64, device="cuda")
        forms = {"fused logits": lambda: ops.classifier_head(x, cw),
                 "fused all 5": lambda: ops.classifier_head(x, cw, k=5, want=ops.CLASSIFIER_OUTPUTS),
                 "chain 2x linear_x3": lambda: ops.linear_x3(ops.linear_x3(x, x1, b1, act=1, out=hid), x2, b2p, out=out)}
        res = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                res[k].append(timeit(fn))
        diff = (ops.classifier_head(x, cw)["logits"] - forms["chain 2x linear_x3"]()[:, :C]).abs().max().item()
        work = _lib.lib().mmr_classifier_work_bytes(B, D, H, C)
        print(f"B={B} D={D} H={H} C={C}  workspace {work} B (chain hidden {B * H * 4} B)  max|fused - chain| {diff:.3e}")
        for k, v in res.items():
            print(f"  {k:20s} median {statistics.median(v):7.1f} us   rounds " + " ".join(f"{t:7.1f}" for t in v), flush=True)


def model_ab(rounds):
    from mmr_amd import synthetic
    from mmr_amd.model import build_bench_model, init_classifier_state
    B = 256
    m = build_bench_model(device="cuda")
    m.classifier = ops.ClassifierW(*(init_classifier_state(768, 43, 5)[k].to("cuda") for k in (
        "classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias")))
    img = torch.from_numpy(synthetic.image_from_u8(synthetic.image_u8(B, 4))).to("cuda")
    ids, mask = (torch.from_numpy(t).to("cuda") for t in synthetic.reports(B, 128, 5))
    forms = {"forward (with logits)": lambda: m(img, ids, mask),
             "_forward (no classifier)": lambda: m._forward(img, ids, mask),
             "predict (K = 5, host copies)": lambda: m.predict(img, ids, mask)}
    res = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            res[k].append(timeit(fn, iters=5))
    print(f"cfg2 bench model, B={B}, joint_dim 768, C=43")
    for k, v in res.items():
        print(f"  {k:30s} median {statistics.median(v) / 1e3:8.2f} ms   rounds " + " ".join(f"{t / 1e3:8.2f}" for t in v),
              flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 5
    head_ab(rounds)
    if "--model" in sys.argv:
        model_ab(max(2, rounds // 2))
