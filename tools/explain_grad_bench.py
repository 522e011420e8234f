"""Timing and error ratios of the gradient explanations (explain_grad.GradientExplainer over csrc/explain_grad.hip) at
the bench geometry — Np = 49, Lt = 128, Ci = Ct = D = 768, 8 heads, 22 classes, K = 5 targets, 50 IG steps, 224 x 224 —
at B = 1 and B = 16, random weights and features (no towers: the pass starts from their features), against
  torch f32   the same arithmetic by torch autograd on the same GPU: oracle.towers.cross_modal_fusion + classifier,
              one forward over the B (Grad-CAM) / B x 50 (IG) patch sets (the text side recomputed per set, as the
              reference does) and one backward per target
  CPU         that restatement on the host CPU (B = 1 only; the reference's own path is 5 x 51 separate batch-1 passes)
Error ratios at B = 1: deviation of the device result and of the torch f32 result from the torch f64 result (same GPU),
raw vectors relative to their max-abs, maps absolute — the tests' bound is device <= 8 x f32.
Per-kernel times at the shapes of one IG chunk of B = 1 (N = 50 patch sets).
One process, warmed, device events, median over the rounds.  No threshold is asserted: diagnostic only.
usage: python tools/explain_grad_bench.py [rounds] [--out FILE]"""
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mmr_amd import ops  # noqa: E402
from mmr_amd.explain_grad import GradientExplainer, gauss_legendre  # noqa: E402
from mmr_amd.model import init_classifier_state, init_fusion_state  # noqa: E402
from oracle import towers as otw  # noqa: E402

NP, LT, CI, D, HEADS, C, K, STEPS, SIZE = 49, 128, 768, 768, 8, 22, 5, 50, (224, 224)
P_ = "fusion_layers.0."


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def upsample_norm(raw, mode):
    """(B, T, Np) -> (B, T, H, W) as the two map orders"""
    B, T, n = raw.shape
    g = math.isqrt(n)

    def mm(x):
        mn, mx = x.amin(-1, keepdim=True), x.amax(-1, keepdim=True)
        return (x - mn) / (mx - mn + 1e-8)
    if mode == "ig":
        v = mm(raw).clamp(0, 1).view(B * T, 1, g, g)
        return F.interpolate(v, size=SIZE, mode="bilinear", align_corners=False).view(B, T, *SIZE)
    up = F.interpolate(torch.relu(raw).view(B * T, 1, g, g), size=SIZE, mode="bilinear", align_corners=False)
    return mm(up.view(B, T, -1)).view(B, T, *SIZE)


def torch_explain(sd, G, P, T, targets, dtype):
    """autograd restatement on the tensors' device -> (gradcam_raw, gradcam_maps, ig_raw, ig_maps)"""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    G, P, T = G.to(dtype), P.to(dtype), T.to(dtype)
    B = P.shape[0]

    def logits(g, p, t):
        seq = otw.cross_modal_fusion(g, p, t, sd, P_, HEADS, False)
        return F.linear(F.gelu(F.linear(seq, sd["classifier.0.weight"], sd["classifier.0.bias"])),
                        sd["classifier.3.weight"], sd["classifier.3.bias"])
    Pg = P.clone().requires_grad_(True)
    lg = logits(G, Pg, T)
    cams = []
    for j in range(targets.shape[1]):
        s = lg[torch.arange(B), targets[:, j]].sum()
        cams.append((torch.autograd.grad(s, Pg, retain_graph=True)[0] * P).sum(-1))
    cam = torch.stack(cams, 1)
    al, wt = gauss_legendre(STEPS)
    al, wt = torch.tensor(al, dtype=dtype, device=P.device), torch.tensor(wt, dtype=dtype, device=P.device)
    Ps = (P[:, None] * al[None, :, None, None]).reshape(B * STEPS, NP, CI).requires_grad_(True)
    lg = logits(Ps.mean(1), Ps, T.repeat_interleave(STEPS, 0))
    igs = []
    for j in range(targets.shape[1]):
        tok = targets[:, j].repeat_interleave(STEPS)
        s = lg[torch.arange(B * STEPS), tok, tok].sum()
        gr = torch.autograd.grad(s, Ps, retain_graph=True)[0].view(B, STEPS, NP, CI)
        igs.append(((gr * wt[None, :, None, None]).sum(1) * P).abs().sum(-1))
    ig = torch.stack(igs, 1)
    return cam, upsample_norm(cam, "gradcam"), ig, upsample_norm(ig, "ig")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 3
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda:0")
    hs = init_fusion_state(CI, CI, D, HEADS, 1, seed=5)
    hs.update(init_classifier_state(D, C, seed=6))
    last = {k[len(P_):]: v for k, v in hs.items() if k.startswith(P_)}
    ex = GradientExplainer(last, tuple(hs[f"classifier.{k}"] for k in ("0.weight", "0.bias", "3.weight", "3.bias")),
                           HEADS, dev)
    sd_dev = {k: v.to(dev) for k, v in hs.items() if k.startswith(P_) or k.startswith("classifier.")}
    sd_cpu = {k: v for k, v in hs.items() if k.startswith(P_) or k.startswith("classifier.")}
    lines = [f"explain_gradients Np={NP} Lt={LT} Ci=Ct=D={D} heads={HEADS} C={C} K={K} ig_steps={STEPS} "
             f"{SIZE[0]}x{SIZE[1]}  workspace bound {ex.workspace_bytes >> 20} MiB  ({rounds} rounds)"]
    g = torch.Generator().manual_seed(9)
    for B in (1, 16):
        G, P, T = torch.randn(B, CI, generator=g), torch.randn(B, NP, CI, generator=g), torch.randn(B, LT, CI, generator=g)
        targets = torch.stack([torch.randperm(C, generator=g)[:K] for _ in range(B)])
        Gd, Pd, Td, tg = G.to(dev), P.to(dev), T.to(dev), targets.to(dev)

        def device():
            TQ, tproj = ex.text_side(Td)
            a = ex.gradcam(Gd, Pd, TQ, tproj, tg, SIZE)
            b = ex.integrated_gradients(Pd, TQ, tproj, tg, STEPS, SIZE)
            return a[1], a[2], b[0], b[1]

        def torch32():
            return torch_explain(sd_dev, Gd, Pd, Td, tg, torch.float32)
        if B == 1:
            got, r32 = device(), torch32()
            r64 = torch_explain(sd_dev, Gd, Pd, Td, tg, torch.float64)
            for name, i, rel in (("gradcam_raw", 0, True), ("gradcam_maps", 1, False), ("ig_raw", 2, True),
                                 ("ig_maps", 3, False)):
                den = r64[i].abs().max().item() if rel else 1.0
                d = (got[i].double() - r64[i]).abs().max().item() / den
                d32 = (r32[i].double() - r64[i]).abs().max().item() / den
                lines.append(f"  error vs torch f64, B=1, {name:13s} device {d:.3e}   torch f32 {d32:.3e}   ratio "
                             f"{d / max(d32, 1e-300):.2f}  (bound 8)")
        td = [timed(device, 1) for _ in range(rounds)]
        tt = [timed(torch32, 1) for _ in range(rounds)]
        lines.append(f"  B={B:2d}  device pass (text side + Grad-CAM + IG, {K} targets)   median {statistics.median(td):9.2f} ms"
                     f"   rounds " + " ".join(f"{x:9.2f}" for x in td))
        lines.append(f"  B={B:2d}  torch f32 autograd, same GPU                         median {statistics.median(tt):9.2f} ms"
                     f"   rounds " + " ".join(f"{x:9.2f}" for x in tt))
        if B == 1:
            t0 = time.perf_counter()
            torch_explain(sd_cpu, G, P, T, targets, torch.float32)
            lines.append(f"  B={B:2d}  torch f32 autograd, host CPU ({torch.get_num_threads()} threads)"
                         f"                 {(time.perf_counter() - t0) * 1e3:9.2f} ms   (once)")
    # per-kernel times at one IG chunk of one sample: N = 50 patch sets
    N, dh, sc = STEPS, D // HEADS, 1.0 / math.sqrt(D // HEADS)
    x = torch.randn(N * NP, 3 * CI, device=dev)
    t3 = torch.randn(N * LT, 3 * D, device=dev)
    go_p, go_t = torch.randn(N * NP, CI, device=dev), torch.randn(N * LT, D, device=dev)
    gam = torch.ones(CI, device=dev)
    wT = torch.randn(CI, 3 * CI, device=dev)
    grads = torch.randn(K * N, NP, CI, device=dev)
    wq = torch.rand(STEPS, device=dev)
    hh = torch.randn(N, 4 * D, device=dev)
    kern = [
        ("attention_fwd  self (50 x 49 x 49, 8 x 96)", lambda: ops.attention_fwd(x[:, :CI], x[:, CI:2 * CI], x[:, 2 * CI:], N, NP, NP, HEADS, dh, sc)),
        ("attention_bwd  self dq dk dv", lambda: ops.attention_bwd(x[:, :CI], x[:, CI:2 * CI], x[:, 2 * CI:], go_p, N, NP, NP, HEADS, dh, sc)),
        ("attention_bwd  txt2img dk dv (lq 128, lk 49)", lambda: ops.attention_bwd(t3[:, :D], x[:, :D], x[:, D:2 * D], go_t, N, LT, NP, HEADS, dh, sc, want=("dk", "dv"))),
        ("attention_bwd  img2txt dq (lq 49, lk 128)", lambda: ops.attention_bwd(x[:, :D], t3[:, D:2 * D], t3[:, 2 * D:], go_p, N, NP, LT, HEADS, dh, sc, want=("dq",))),
        ("ln_bwd_rows    2450 x 768", lambda: ops.ln_bwd_rows(go_p, gam, go_p, 1e-5)),
        ("gelu_bwd       50 x 3072", lambda: ops.gelu_bwd(hh, hh)),
        ("linear_f32     dgrad 2450 x 2304 -> 768", lambda: ops.linear_f32(x, wT)),
        ("attribution_maps IG 5 maps x 50 steps, 224 x 224", lambda: ops.attribution_maps(grads, go_p.view(N, NP, CI)[:1], "ig", steps=STEPS, step_w=wq, image_size=SIZE)),
    ]
    lines.append("  per kernel, one IG chunk of one sample (N = 50 patch sets):")
    for name, fn in kern:
        ts = [timed(fn, 10) for _ in range(rounds)]
        lines.append(f"    {name:52s} median {statistics.median(ts) * 1e3:9.1f} us")
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
