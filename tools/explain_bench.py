"""Timing of the attention explanations (ops.explain_attention = mmr_explain_attention, csrc/explain.hip) at
B = 256, Lt = 128, Np = 49, 224 x 224 and of the map alignment (ops.map_alignment = mmr_map_alignment,
csrc/map_align.hip) at N = 512 maps of 224 x 224, P = 256 pairs, each against
  torch      a restatement on the same GPU: mean / the window search by cumsum / F.interpolate for the explanations;
             argsort-of-argsort ranks (ordinal: ties are NOT averaged, so it does less work than the kernel),
             kthvalue thresholds and centred products for the alignment
  host loop  what the device path replaces: every map pulled to the host and the reference-style per-sample code
             (torch on the CPU for the explanations; numpy + scipy pearsonr / spearmanr + np.partition for the
             alignment, where scipy is installed), timed on a subset and scaled to the batch
and of MultiModalRetrievalModel.evaluate_explanations end to end on the mini model (random weights, 64 queries).
One process, warmed, device events around `iters` calls, the forms interleaved per round, median over the rounds
(host loops: host clock, once).  Diagnostic only.
usage: python tools/explain_bench.py [rounds] [--out FILE]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mmr_amd import ops, synthetic  # noqa: E402


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


def minmax(x):
    mn, mx = x.amin(-1, keepdim=True), x.amax(-1, keepdim=True)
    return (x - mn) / ((mx - mn) + 1e-8)


def heat(v, size):
    g = int(round(v.shape[-1] ** 0.5))
    return F.interpolate(minmax(v).view(-1, 1, g, g), size=size, mode="bilinear", align_corners=False)[:, 0]


def torch_explain(t2i, i2t, comb, size):
    """the Lc > Np, Lc < T path of the kernel, batched (works on either device)"""
    npatch, lc = t2i.shape[2], comb.shape[1]
    p_txt, t_img = t2i.mean(1), i2t.mean(1)
    cs = comb.double().sum(1)
    cum = torch.cat([torch.zeros_like(cs[:, :1]), cs.cumsum(1)], 1)
    wins = cum[:, npatch:] - cum[:, :lc - npatch + 1]
    best, off = wins.max(1)
    idx = off[:, None] + torch.arange(npatch, device=comb.device)[None, :]
    p_comb = (torch.gather(cs, 1, idx) / lc).float() * (best / (cs.sum(1) + 1e-12) >= 0.06)[:, None]
    rm = comb.mean(2)
    t_comb = minmax(rm).clamp(0, 1)
    n = min(t_img.shape[1], t_comb.shape[1])
    final_patch = minmax(0.6 * p_txt + 0.4 * p_comb)
    final_token = minmax(0.6 * t_img[:, :n] + 0.4 * t_comb[:, :n])
    return heat(p_txt, size), heat(p_comb, size), heat(final_patch, size), final_token


def torch_align(maps, pa, pb, ks):
    n, hw = maps.shape
    rank = torch.argsort(torch.argsort(maps, 1), 1).double()  # ordinal ranks (no tie averaging)
    thr = torch.stack([torch.kthvalue(maps, hw - k + 1, 1).values for k in ks], 1)
    a, b = maps[pa].double(), maps[pb].double()
    a, b = a - a.mean(1, keepdim=True), b - b.mean(1, keepdim=True)
    pearson = (a * b).sum(1) / ((a * a).sum(1).sqrt() * (b * b).sum(1).sqrt())
    ra, rb = rank[pa] - (hw - 1) / 2, rank[pb] - (hw - 1) / 2
    spearman = (ra * rb).sum(1) / ((ra * ra).sum(1).sqrt() * (rb * rb).sum(1).sqrt())
    ta, tb = maps[pa][:, None, :] >= thr[pa][:, :, None], maps[pb][:, None, :] >= thr[pb][:, :, None]
    return pearson, spearman, (ta & tb).sum(2), (ta | tb).sum(2)


def host_align(maps, pa, pb, fracs):
    from scipy.stats import pearsonr, spearmanr
    out = []
    for i, j in zip(pa, pb):
        a, b = maps[i], maps[j]
        row = [float(pearsonr(a, b)[0]), float(spearmanr(a, b).correlation)]
        for f in fracs:
            k = max(1, int(len(a) * f))
            at, bt = a >= np.partition(a, -k)[-k], b >= np.partition(b, -k)[-k]
            row.append(float((at & bt).sum()) / (float((at | bt).sum()) + 1e-8))
        out.append(row)
    return out


def mini_model():
    from mmr_amd.model import (Backbones, MultiModalRetrievalModel, init_classifier_state, init_fusion_state,
                               init_head_state)
    from mmr_amd.towers import BERT_BASE, SWIN_T, init_bert_state, init_swin_state
    scfg = dict(SWIN_T, embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8])
    bcfg = dict(BERT_BASE, vocab_size=1000, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                intermediate_size=512)
    hs = init_head_state(256, 128, 64, 3)
    hs.update(init_fusion_state(256, 128, 64, 4, 2, 4))
    hs.update(init_classifier_state(64, 43))
    bb = Backbones(swin_state=init_swin_state(scfg, 1), bert_state=init_bert_state(bcfg, 2), swin_cfg=scfg,
                   bert_cfg=bcfg, device="cuda:0", tower_dtype="x3")
    return MultiModalRetrievalModel(joint_dim=64, num_heads=4, model_type="multimodal", backbones=bb, head_state=hs,
                                    device="cuda:0", use_shared_ffn=False)


def main(rounds, out_path):
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def table(title, forms, iters):
        res = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                res[k].append(timeit(fn, iters))
        say(f"{title}  ({rounds} rounds x {iters} calls)")
        for k, v in res.items():
            say(f"  {k:58s} median {statistics.median(v):9.3f} ms   rounds " + " ".join(f"{t:9.3f}" for t in v))

    # ---- explanations
    B, Lt, Np, Lc, size = 256, 128, 49, 51, (224, 224)
    g = torch.Generator().manual_seed(1)
    t2i = torch.softmax(torch.randn(B, Lt, Np, generator=g) * 3, -1).cuda()
    i2t = torch.softmax(torch.randn(B, Np, Lt, generator=g) * 3, -1).cuda()
    comb = torch.softmax(torch.randn(B, Lc, Lc, generator=g) * 3, -1).cuda()
    dev = ops.explain_attention(t2i, i2t, comb, text_len=Lt, image_size=size)
    ref = torch_explain(t2i, i2t, comb, size)
    err = max(float((dev[k] - r).abs().max()) for k, r in zip(("map_txt2img", "map_comb", "map_final"), ref))
    assert err <= 1e-4, err
    table(f"explain_attention B={B} Lt={Lt} Np={Np} Lc={Lc} {size[0]}x{size[1]}  (torch restatement max|diff| {err:.2e})",
          {"ops.explain_attention (vectors + 3 heat maps)": lambda: ops.explain_attention(t2i, i2t, comb, text_len=Lt,
                                                                                         image_size=size),
           "ops.explain_attention (vectors only)": lambda: ops.explain_attention(t2i, i2t, comb, text_len=Lt),
           "torch restatement (mean / cumsum / interpolate, same GPU)": lambda: torch_explain(t2i, i2t, comb, size)},
          20)
    sub = 32
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = [x[:sub].cpu() for x in (t2i, i2t, comb)]
    for b in range(sub):
        torch_explain(h[0][b:b + 1], h[1][b:b + 1], h[2][b:b + 1], size)
    dt = (time.perf_counter() - t0) * 1e3
    say(f"  {'host loop (maps to the host, torch on the CPU per sample)':58s} {dt / sub * B:16.3f} ms   "
        f"({sub} samples in {dt:.1f} ms, scaled to {B})")

    # ---- alignment
    N, P, fracs = 512, 256, (0.05, 0.20)
    maps = dev["map_final"].repeat(2, 1, 1).reshape(N, -1).contiguous()
    maps = maps + torch.rand(maps.shape, generator=torch.Generator().manual_seed(2)).cuda() * 1e-3  # distinct maps
    pa = torch.arange(P, device="cuda")
    pb = (pa * 7 + 13) % N
    ks = [ops.topk_count(maps.shape[1], f) for f in fracs]
    r = ops.map_alignment(maps, pa, pb, fracs)
    tr = torch_align(maps, pa, pb, ks)
    assert float((r["pearson"] - tr[0]).abs().max()) <= 1e-9 and torch.equal(r["inter_union"][:, :, 0], tr[2])
    table(f"map_alignment N={N} HW={maps.shape[1]} P={P} fracs={fracs}  workspace "
          f"{ops._L().mmr_map_alignment_work_bytes(N, maps.shape[1])} B",
          {"ops.map_alignment": lambda: ops.map_alignment(maps, pa, pb, fracs),
           "torch restatement (argsort x 2, kthvalue, same GPU)": lambda: torch_align(maps, pa, pb, ks)}, 3)
    try:
        import scipy
        sub = 16
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hm = maps.cpu().numpy()
        t1 = time.perf_counter()
        host_align(hm, pa[:sub].tolist(), pb[:sub].tolist(), fracs)
        dt = (time.perf_counter() - t1) * 1e3
        say(f"  {'host loop (numpy + scipy ' + scipy.__version__ + ' per pair)':58s} {dt / sub * P:16.3f} ms   "
            f"({sub} pairs in {dt:.1f} ms, scaled to {P}; + {(t1 - t0) * 1e3:.1f} ms to pull the maps)")
    except ImportError:
        say("  scipy: not installed here, the host loop is not measured")
    del maps, r, tr, dev, ref

    # ---- the evaluation end to end
    from mmr_amd.retrieval import MI355XRetrievalEngine
    m = mini_model()
    nb, bs = 4, 16
    batches = []
    for i in range(nb):
        img = torch.from_numpy(synthetic.image_from_u8(synthetic.image_u8(bs, 10 + i))).cuda()
        ids, mask = (torch.from_numpy(x).cuda() for x in synthetic.reports(bs, 128, 20 + i, vocab=1000))
        batches.append((img, ids, mask))
    embs = torch.cat([m(*b)["joint_emb"] for b in batches])
    eng = MI355XRetrievalEngine(embs=embs.cpu().numpy(), ids=[str(i) for i in range(nb * bs)])
    m.set_retriever(eng)
    out = m.evaluate_explanations(batches, K=10, exclude_self=True)
    table(f"evaluate_explanations, mini model, {nb} x {bs} queries, 224x224, exclude_self  -> {out}",
          {"evaluate_explanations (forward + explain + top-K + alignment)":
           lambda: m.evaluate_explanations(batches, K=10, exclude_self=True),
           "the forwards alone (return_attention=False)": lambda: [m(*b)["joint_emb"] for b in batches]}, 3)
    eng.close()
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
