"""GPU: the gradient explanations — the backward kernels of csrc/explain_grad.hip (ops.attention_bwd, ln_bwd_rows,
gelu_bwd, attribution_maps), the gradient pass over them (explain_grad.GradientExplainer) and the model layer
(explain_gradients, predict(explain="full")).

Bound (explain_grad_ref.BOUND_FACTOR): a device result may deviate from the f64 torch restatement by at most 8 x the
deviation of the f32 torch restatement (run on the CPU here) from it — normalised by the tensor's max-abs for
gradients and raw vectors, absolute for maps in [0, 1].

The raw attribution vectors depend on mmr_attribution_maps summing its f32 products in f64: test_model_ig[x3-50-
tokens1-text], sample 0, token 25 — a vector dominated by its own patch, where the f32 restatement lands 9.157e-10 of
max-abs from f64 — measured 8.975e-08 (ratio 98) with f32 sums and 9.157e-10 (ratio 1.00) with f64 sums."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import explain_grad_ref as gr
from attn_maps_ref import towers_mini
from mmr_amd import _lib, ops, synthetic
from mmr_amd.explain_grad import gauss_legendre
from mmr_amd.model import Backbones, MultiModalRetrievalModel
from mmr_amd.retrieval import MI355XRetrievalEngine
from mmr_amd.towers import BERT_BASE, SWIN_T

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = 2.0 ** -24
GUARD = -7.5


def bound(dev32):
    return gr.BOUND_FACTOR * dev32


# ------------------------------------------------------------------------------------------------ attention_bwd
def attn_ref(q, k, v, go, b, lq, lk, heads, dh, scale, dtype):
    """torch autograd on (b*l, heads*dh) rows -> (out, dq, dk, dv)"""
    q, k, v, go = (t.to(dtype).clone() for t in (q, k, v, go))
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)

    def hd(t, L):
        return t.view(b, L, heads, dh).transpose(1, 2)
    s = hd(q, lq) @ hd(k, lk).transpose(-1, -2) * scale
    o = (s.softmax(-1) @ hd(v, lk)).transpose(1, 2).reshape(b * lq, heads * dh)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), go)
    return o.detach(), dq, dk, dv


def attn_inputs(b, lq, lk, heads, dh, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * lq + lk + dh)
    E = heads * dh
    return (torch.randn(b * lq, E, generator=g), torch.randn(b * lk, E, generator=g), torch.randn(b * lk, E, generator=g),
            torch.randn(b * lq, E, generator=g))


ATTN_SHAPES = [(2, 49, 49, 4, 64), (2, 128, 49, 4, 16), (3, 49, 128, 4, 16), (2, 5, 3, 1, 8), (1, 128, 128, 8, 96),
               (2, 1, 49, 4, 32)]


@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_bwd_f64(shape):
    b, lq, lk, heads, dh = shape
    E = heads * dh
    scale = dh ** -0.5
    q, k, v, go = attn_inputs(*shape)
    ref = attn_ref(q, k, v, go, b, lq, lk, heads, dh, scale, torch.float64)
    r32 = attn_ref(q, k, v, go, b, lq, lk, heads, dh, scale, torch.float32)
    # q | k | v as column slices of one packed tensor (lq == lk) or strided rows; outputs inside guard padding
    pad = 8
    if lq == lk:
        packed = torch.cat([q, k, v], 1).to(DEV)
        dq_, dk_, dv_ = packed[:, :E], packed[:, E:2 * E], packed[:, 2 * E:]
    else:
        dq_, dk_, dv_ = (torch.cat([t, torch.full((t.shape[0], pad), GUARD)], 1).to(DEV)[:, :E] for t in (q, k, v))
    god = go.to(DEV)
    outs = {n: torch.full((rows, E + pad), GUARD, device=DEV) for n, rows in
            (("dq", b * lq), ("dk", b * lk), ("dv", b * lk))}
    o = ops.attention_fwd(dq_, dk_, dv_, b, lq, lk, heads, dh, scale)
    got = ops.attention_bwd(dq_, dk_, dv_, god, b, lq, lk, heads, dh, scale, out={n: t[:, :E] for n, t in outs.items()})
    torch.cuda.synchronize()
    for name, g_, rf, r3 in zip(("out", "dq", "dk", "dv"), (o,) + got, ref, r32):
        d, d32 = gr.rel_dev(g_.cpu(), rf), gr.rel_dev(r3, rf)
        print(f"{name} {shape}: device {d:.3e} f32 torch {d32:.3e} ratio {d / max(d32, EPS32):.2f}")
        assert d <= bound(d32), (name, d, d32)
    for n, t in outs.items():
        assert bool((t[:, E:] == GUARD).all()), f"{n}: guard columns written"
    # each NULL-output combination: the computed ones keep their bits
    for want in (("dq",), ("dk",), ("dv",), ("dq", "dk"), ("dq", "dv"), ("dk", "dv")):
        part = ops.attention_bwd(dq_, dk_, dv_, god, b, lq, lk, heads, dh, scale, want=want)
        for n, full, p in zip(("dq", "dk", "dv"), got, part):
            assert (p is None) == (n not in want)
            if p is not None:
                assert torch.equal(p, full), (want, n)


def test_attention_bwd_exact_cases():
    heads, dh = 2, 16
    E = heads * dh
    g = torch.Generator().manual_seed(5)
    # lk = 1: P = 1 exactly, so dV = sum_q dO (bit for bit at lq = 1) and dS = 0: dQ = dK = 0
    for lq in (1, 5):
        q, k, v, go = (torch.randn(r, E, generator=g).to(DEV) for r in (3 * lq, 3, 3, 3 * lq))
        dq, dk, dv = ops.attention_bwd(q, k, v, go, 3, lq, 1, heads, dh, 0.25)
        assert not dq.any() and not dk.any()
        if lq == 1:
            assert torch.equal(dv, go)
        else:
            assert gr.rel_dev(dv.cpu(), go.view(3, lq, E).double().sum(1).cpu()) <= 8 * EPS32
    # dO = 0: all zeros
    q, k, v = (torch.randn(r, E, generator=g).to(DEV) for r in (2 * 20, 2 * 33, 2 * 33))
    for t in ops.attention_bwd(q, k, v, torch.zeros(40, E, device=DEV), 2, 20, 33, heads, dh, 0.25):
        assert not t.any()


def test_attention_bwd_launch_independent():
    b, lq, lk, heads, dh = 7, 49, 37, 4, 32
    q, k, v, go = (t.to(DEV) for t in attn_inputs(b, lq, lk, heads, dh, seed=3))
    full = ops.attention_bwd(q, k, v, go, b, lq, lk, heads, dh, 0.2)
    fwd = ops.attention_fwd(q, k, v, b, lq, lk, heads, dh, 0.2)
    s = slice(2 * lq, 4 * lq), slice(2 * lk, 4 * lk)
    two = ops.attention_bwd(q[s[0]], k[s[1]], v[s[1]], go[s[0]], 2, lq, lk, heads, dh, 0.2)
    assert torch.equal(two[0], full[0][s[0]]) and torch.equal(two[1], full[1][s[1]]) and torch.equal(two[2], full[2][s[1]])
    assert torch.equal(ops.attention_fwd(q[s[0]], k[s[1]], v[s[1]], 2, lq, lk, heads, dh, 0.2), fwd[s[0]])


def test_refusals():
    L = _lib.lib()
    x = torch.zeros(130 * 128, device=DEV)
    p, st = _lib.ptr(x), _lib.stream_ptr(x.device)
    mis = _lib.ctypes.c_void_p(x.data_ptr() + 4)

    def bwd(lq=4, lk=4, heads=1, dh=16, q=p, go=p, ld=128):
        return L.mmr_attention_bwd_f32(q, ld, p, ld, p, ld, go, ld, p, ld, p, ld, p, ld, 1, lq, lk, heads, dh, 1.0, st)
    for kw, status, word in ((dict(lq=129), 4, b"lq = 129"), (dict(lk=129), 4, b"lk = 129"), (dict(dh=12), 4, b"12"),
                             (dict(dh=104), 4, b"104"), (dict(q=mis), 1, b"alignment"), (dict(ld=126), 1, b"multiple of 4"),
                             (dict(q=None), 1, b"NULL"), (dict(go=None), 1, b"NULL")):
        assert bwd(**kw) == status, kw
        assert word in L.mmr_last_error(), (kw, L.mmr_last_error())
    assert L.mmr_attention_fwd_f32(p, 128, p, 128, p, 128, p, 128, 1, 129, 4, 1, 16, 1.0, st) == 4
    assert L.mmr_ln_bwd_rows(p, 2048, p, p, 2048, p, 2048, 1, 1025, 1e-5, st) == 1 and b"1025" in L.mmr_last_error()
    assert L.mmr_ln_bwd_rows(None, 8, p, p, 8, p, 8, 1, 8, 1e-5, st) == 1 and b"NULL" in L.mmr_last_error()
    assert L.mmr_gelu_bwd_rows(p, 8, None, 8, p, 8, None, 0, 1, 8, st) == 1 and b"dy" in L.mmr_last_error()
    assert L.mmr_attribution_maps(p, p, None, 1, 1, 1, 1, 48, 16, 0, 8, 8, p, p, st) == 1
    assert b"perfect square" in L.mmr_last_error()
    torch.cuda.synchronize()
    assert not x.any()  # nothing was launched


# ------------------------------------------------------------------------------------------------ LN / GELU backward
@pytest.mark.parametrize("rows,c", [(7, 64), (3, 256), (2, 768), (1, 8)])
def test_ln_bwd_rows(rows, c):
    g = torch.Generator().manual_seed(rows * 1000 + c)
    z = torch.randn(rows, c, generator=g) * 2 + 0.5
    z[0] = 1.25  # a constant row: variance 0
    gam, bet = 1 + 0.1 * torch.randn(c, generator=g), torch.randn(c, generator=g)
    dy = torch.randn(rows, c, generator=g)
    eps = 1e-5

    def ref(dtype):
        zz = z.to(dtype).clone().requires_grad_(True)
        y = F.layer_norm(zz, (c,), gam.to(dtype), bet.to(dtype), eps)
        return torch.autograd.grad(y, zz, dy.to(dtype))[0]
    r64, r32 = ref(torch.float64), ref(torch.float32)
    # strided rows in and out, guard columns
    zs = torch.cat([z, torch.full((rows, 4), GUARD)], 1).to(DEV)[:, :c]
    dys = torch.cat([dy, torch.full((rows, 12), GUARD)], 1).to(DEV)[:, :c]
    out = torch.full((rows, c + 4), GUARD, device=DEV)
    got = ops.ln_bwd_rows(zs, gam.to(DEV), dys, eps, out=out[:, :c])
    d, d32 = gr.rel_dev(got.cpu(), r64), gr.rel_dev(r32, r64)
    print(f"ln_bwd ({rows}, {c}): device {d:.3e} f32 torch {d32:.3e}")
    assert d <= bound(d32)
    assert bool((out[:, c:] == GUARD).all())
    assert not ops.ln_bwd_rows(zs, gam.to(DEV), torch.zeros(rows, c, device=DEV), eps).any()


def test_gelu_bwd():
    grid = torch.linspace(-9.0, 9.0, 1441)
    h = torch.cat([torch.tensor([0.0, -0.0, 50.0, -50.0, 1e4, -1e4, 1e-30, -1e-30]), grid]).view(1, -1)
    dy = torch.full_like(h, 1.5)

    def ref(dtype):
        x = h.to(dtype).clone().requires_grad_(True)
        y = F.gelu(x)
        return torch.autograd.grad(y, x, dy.to(dtype))[0], y.detach()
    (r64, y64), (r32, y32) = ref(torch.float64), ref(torch.float32)
    got = ops.gelu_bwd(h.to(DEV), dy.to(DEV)).cpu()
    y = ops.gelu_rows(h.to(DEV)).cpu()
    assert got[0, 0] == 0.75 and got[0, 1] == 0.75 and got[0, 2] == 1.5 and got[0, 3] == 0 and got[0, 4] == 1.5
    assert got[0, 5] == 0 and torch.isfinite(got).all()
    d, d32 = gr.rel_dev(got, r64), gr.rel_dev(r32, r64)
    print(f"gelu_bwd: device {d:.3e} f32 torch {d32:.3e}")
    assert d <= bound(d32)
    fin = slice(0, None)
    assert gr.rel_dev(y[fin], y64[fin]) <= bound(gr.rel_dev(y32[fin], y64[fin]))


# ------------------------------------------------------------------------------------------------ attribution maps
@pytest.mark.parametrize("mode,steps,size", [("gradcam", 1, (28, 28)), ("ig", 5, (28, 28)), ("ig", 1, (5, 3)),
                                             ("gradcam", 1, (224, 224))])
def test_attribution_maps(mode, steps, size):
    X, T, Np, Ci = 2, 3, 49, 72
    g = torch.Generator().manual_seed(11 + steps)
    grad = torch.randn(T * X * steps, Np, Ci, generator=g)
    x = torch.randn(X, Np, Ci, generator=g)
    w = torch.rand(steps, generator=g) if steps > 1 else None
    raw, maps = ops.attribution_maps(grad.to(DEV), x.to(DEV), mode, steps=steps, step_w=None if w is None else w.to(DEV),
                                     image_size=size, target_major=True)
    raw2, maps2 = ops.attribution_maps(grad.view(T, X, steps, Np, Ci).transpose(0, 1).reshape(-1, Np, Ci).to(DEV),
                                       x.to(DEV), mode, steps=steps, step_w=None if w is None else w.to(DEV),
                                       image_size=size)
    assert torch.equal(raw.view(T, X, Np).transpose(0, 1), raw2.view(X, T, Np))
    assert torch.equal(maps.view(T, X, *size).transpose(0, 1), maps2.view(X, T, *size))
    gd = grad.double().view(T, X, steps, Np, Ci)
    tot = gd.sum(2) if w is None else (gd * w.double()[None, None, :, None, None]).sum(2)
    t = tot * x.double()[None]
    rr = (t.abs() if mode == "ig" else t).sum(-1)                      # (T, X, Np)
    scale = t.abs().sum(-1).max()
    assert float((raw.cpu().double().view(T, X, Np) - rr).abs().max() / scale) <= (Ci + steps + 2) * EPS32
    for ti in range(T):
        for xi in range(X):
            v = rr[ti, xi]
            if mode == "gradcam":
                m = gr.minmax(gr.upsample(torch.relu(v), size))
                c = gr.cond(gr.upsample(torch.relu(v), size))
            else:
                m = gr.upsample(gr.minmax(v).clamp(0, 1), size)
                c = gr.cond(v)
            err = gr.abs_dev(maps.view(T, X, *size)[ti, xi].cpu(), m)
            # the raw vector's error relative to its range, doubled by the normalisation, + the f32 map arithmetic
            tol = (2 * c * float(scale / v.abs().max()) * (Ci + steps + 2) + 16) * EPS32
            assert err <= tol, (ti, xi, err, tol)


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module", params=["x3", "bf16"])
def mini(request):
    f, w = towers_mini()
    cfg = json.loads(bytes(f["cfg"]).decode())
    scfg = dict(SWIN_T, embed_dim=cfg["swin"]["embed_dim"], depths=cfg["swin"]["depths"],
                num_heads=cfg["swin"]["num_heads"])
    bb = Backbones(swin_state=w["swin"], bert_state=w["bert"], swin_cfg=scfg, bert_cfg=dict(BERT_BASE, **cfg["bert"]),
                   device=DEV, tower_dtype=request.param)
    image = torch.from_numpy(synthetic.image_from_u8(f["img_u8"])).to(DEV)
    ids = torch.from_numpy(f["input_ids"]).to(DEV)
    mask = torch.from_numpy(f["attention_mask"]).to(DEV)
    kw = dict(joint_dim=cfg["joint_dim"], num_heads=cfg["num_heads"], backbones=bb, head_state=w["head"], device=DEV,
              use_shared_ffn=False)
    return MultiModalRetrievalModel(model_type="multimodal", **kw), kw, (image, ids, mask), w["head"]


TOKENS = [0, 1, 25, 49, 50]
SIZE = (28, 28)


def features(m, args):
    g, p, _ = m.backbones.encode_image(args[0], want_patches=True)
    t = m.backbones.encode_text(args[1], args[2]).float().cpu() if args[1] is not None else None
    return g.float().cpu(), p.float().cpu(), t


@pytest.mark.parametrize("text", [True, False], ids=["text", "default_token"])
def test_model_gradcam_tokens(mini, text):
    """Grad-CAM through the (token, class-weight) interface at the three token kinds: raw gradients, raw vectors, maps
    and token_logits against the f64 restatement on the model's own f32 features"""
    m, kw, args, hsd = mini
    args = args if text else (args[0], None, None)
    r = m.explain_gradients(*args, targets=TOKENS, methods=("gradcam",), image_size=SIZE)
    ex = m._grad_explainer
    G, P, T = features(m, args)
    T32 = T.to(DEV) if T is not None else ex.W["default_txt"].expand(2, -1, -1).contiguous()
    TQ, tproj = ex.text_side(T32)
    tg = torch.tensor([TOKENS, TOKENS], device=DEV)
    grads, raw, maps, logits = ex.gradcam(G.to(DEV), P.to(DEV), TQ, tproj, tg, SIZE)
    torch.cuda.synchronize()
    assert torch.equal(raw, r["gradcam_raw"]) and torch.equal(maps, r["gradcam_maps"])
    assert torch.equal(logits, r["token_logits"]) and r["ig_maps"] is None and r["targets"].tolist() == [TOKENS] * 2
    assert maps.shape == (2, 5, 28, 28) and logits.shape == (2, 51, 43)
    for b in range(2):
        for i, t in enumerate(TOKENS):
            tb = None if T is None else T[b]
            r64 = gr.gradcam(G[b], P[b], tb, hsd, kw["num_heads"], t, SIZE, torch.float64)
            r32 = gr.gradcam(G[b], P[b], tb, hsd, kw["num_heads"], t, SIZE, torch.float32)
            for name, got, dev in (("grad", grads[b, i], gr.rel_dev), ("raw", raw[b, i], gr.rel_dev),
                                   ("map", maps[b, i], gr.abs_dev)):
                d, d32 = dev(got.cpu(), r64[name]), dev(r32[name], r64[name])
                print(f"gradcam text={text} b={b} t={t} {name}: device {d:.3e} f32 {d32:.3e} ratio {d / max(d32, 1e-300):.2f}")
                assert d <= gr.BOUND_FACTOR * d32, (b, t, name, d, d32)
            if i == 0:
                d, d32 = gr.rel_dev(logits[b].cpu(), r64["logits"]), gr.rel_dev(r32["logits"], r64["logits"])
                print(f"token_logits b={b}: device {d:.3e} f32 {d32:.3e}")
                assert d <= gr.BOUND_FACTOR * d32


@pytest.mark.parametrize("text", [True, False], ids=["text", "default_token"])
@pytest.mark.parametrize("steps,tokens", [(8, [0, 1, 25]), (50, [0, 25])])
def test_model_ig(mini, text, steps, tokens):
    m, kw, args, hsd = mini
    args = args if text else (args[0], None, None)
    r = m.explain_gradients(*args, targets=tokens, methods=("ig",), ig_steps=steps, image_size=SIZE)
    torch.cuda.synchronize()
    assert r["gradcam_maps"] is None and r["ig_maps"].shape == (2, len(tokens), 28, 28)
    G, P, T = features(m, args)
    for b in range(2):
        for i, t in enumerate(tokens):
            tb = None if T is None else T[b]
            r64 = gr.integrated_gradients(P[b], tb, hsd, kw["num_heads"], t, SIZE, steps, torch.float64)
            r32 = gr.integrated_gradients(P[b], tb, hsd, kw["num_heads"], t, SIZE, steps, torch.float32)
            for name, got, dev in (("raw", r["ig_raw"][b, i], gr.rel_dev), ("map", r["ig_maps"][b, i], gr.abs_dev)):
                d, d32 = dev(got.cpu(), r64[name]), dev(r32[name], r64[name])
                print(f"ig text={text} steps={steps} b={b} t={t} {name}: device {d:.3e} f32 {d32:.3e} "
                      f"ratio {d / max(d32, 1e-300):.2f}")
                assert d <= gr.BOUND_FACTOR * d32, (b, t, name, d, d32)
    if steps == 8:  # the quadrature-weighted raw gradients of sample 0, token 25, through the gradient pass itself
        ex = m._grad_explainer
        T32 = T.to(DEV) if T is not None else ex.W["default_txt"].expand(2, -1, -1).contiguous()
        TQ, tproj = ex.text_side(T32[:1].contiguous())
        al, wt = gauss_legendre(steps)
        Ps = (P[0].to(DEV)[None] * torch.tensor(al, dtype=torch.float32, device=DEV)[:, None, None]).contiguous()
        S = ex.forward_sets(Ps, ops.x3_mean_rows(Ps), TQ, tproj, steps)
        tok = torch.full((steps,), 25, device=DEV)
        gs = ex.backward_sets(S, tok, ex.class_weights(steps, tok), with_global=True)
        total = (gs.double().cpu() * torch.tensor(wt)[:, None, None]).sum(0)
        tb = None if T is None else T[0]
        r64 = gr.integrated_gradients(P[0], tb, hsd, kw["num_heads"], 25, SIZE, steps, torch.float64)
        r32 = gr.integrated_gradients(P[0], tb, hsd, kw["num_heads"], 25, SIZE, steps, torch.float32)
        d, d32 = gr.rel_dev(total, r64["grad"]), gr.rel_dev(r32["grad"], r64["grad"])
        print(f"ig grad text={text}: device {d:.3e} f32 {d32:.3e}")
        assert d <= gr.BOUND_FACTOR * d32


def test_model_default_targets_and_batch(mini):
    """targets=None: each sample's own top-K classes; (224, 224) once; sample b alone = sample b in the batch; the
    forward's joint_emb bits are unchanged by the call; refusals"""
    m, kw, args, hsd = mini
    before = m(*args)["joint_emb"].clone()
    r = m.explain_gradients(*args, K=3, ig_steps=8, image_size=(224, 224))
    top = ops.classifier_head(before, m.classifier, k=3, want=("topk_idx",))["topk_idx"]
    assert torch.equal(r["targets"], top.to(torch.int64)) and r["targets"].shape == (2, 3)
    assert r["gradcam_maps"].shape == (2, 3, 224, 224) and r["ig_maps"].shape == (2, 3, 224, 224)
    assert torch.equal(m(*args)["joint_emb"], before)
    G, P, T = features(m, args)
    t = int(r["targets"][1, 0])
    for fn, key, a in ((gr.gradcam, "gradcam_maps", (G[1], P[1], T[1])), (gr.integrated_gradients, "ig_maps", (P[1], T[1]))):
        extra = (8,) if key == "ig_maps" else ()
        r64 = fn(*a, hsd, kw["num_heads"], t, (224, 224), *extra, torch.float64)
        r32 = fn(*a, hsd, kw["num_heads"], t, (224, 224), *extra, torch.float32)
        d, d32 = gr.abs_dev(r[key][1, 0].cpu(), r64["map"]), gr.abs_dev(r32["map"], r64["map"])
        print(f"{key} 224: device {d:.3e} f32 {d32:.3e}")
        assert d <= gr.BOUND_FACTOR * d32
    one = m.explain_gradients(*args, targets=r["targets"], ig_steps=8, image_size=(224, 224), samples=[1])
    for k in ("gradcam_maps", "gradcam_raw", "ig_maps", "ig_raw", "token_logits", "targets"):
        assert torch.equal(one[k][0], r[k][1]), k
    for bad, word in (([51], "outside"), ([-1], "outside"), ([43], "classes")):
        with pytest.raises(ValueError, match=word):
            m.explain_gradients(*args, targets=bad)
    m.explain_gradients(*args, targets=[50], methods=("gradcam",), image_size=SIZE)  # a token, not a class
    mt = MultiModalRetrievalModel(model_type="text", **kw)
    with pytest.raises(ValueError, match="multimodal"):
        mt.explain_gradients(*args)


def test_predict_explain_full(mini):
    m, kw, args, _ = mini
    G = synthetic.gauss_gallery(300, kw["joint_dim"], 17)
    eng = MI355XRetrievalEngine(embs=G, ids=[f"r{i}" for i in range(len(G))])
    m.set_retriever(eng)
    try:
        att = m.predict(*args, K=4, explain="attention")
        p = m.predict(*args, K=4, explain="full")
        assert list(p) == ["probs", "preds", "topk_idx", "topk_vals", "retrieval_ids", "retrieval_dists",
                           "attention_map", "ig_maps", "gradcam_maps"]
        assert att["ig_maps"] is None and att["gradcam_maps"] is None
        for k in att:
            if k in ("ig_maps", "gradcam_maps"):
                continue
            if k == "attention_map":
                assert list(p[k]) == list(att[k]) and all(np.array_equal(p[k][n], att[k][n]) for n in att[k])
            else:
                assert np.array_equal(p[k], att[k]) if isinstance(att[k], np.ndarray) else p[k] == att[k], k
        top0 = p["topk_idx"][0]
        e = m.explain_gradients(*args, targets=top0)
        for key in ("ig_maps", "gradcam_maps"):
            assert list(p[key]) == top0
            for i, t in enumerate(top0):
                mp = p[key][t]
                assert isinstance(mp, np.ndarray) and mp.dtype == np.float32 and mp.shape == (224, 224)
                assert np.array_equal(mp, e[key][0, i].cpu().numpy()), (key, t)
    finally:
        m.set_retriever(None)
        eng.close()


# ------------------------------------------------------------------------------------------------ reference golden
def test_reference_golden(mini):
    """the reference's own compute_gradcam_map_for_target / compute_ig_map_for_target outputs (recorded in f32 by
    tests/golden/make_golden_explain_grad.py on the fixture's features) against the gradient pass on those features"""
    path = os.path.join(GOLDEN, "explain_grad_mini.npz")
    g = np.load(path, allow_pickle=False)
    m, kw, args, hsd = mini
    m.explain_gradients(*args, targets=[0], methods=("gradcam",), image_size=SIZE)  # builds the explainer
    ex = m._grad_explainer
    f, _ = towers_mini()
    G, P, T = (torch.from_numpy(np.asarray(f[k], np.float32)) for k in ("img_global", "img_patches", "txt_feats"))
    size = tuple(int(s) for s in g["image_size"])
    tokens = [int(t) for t in g["gradcam_tokens"]]
    TQ, tproj = ex.text_side(T[:1].to(DEV).contiguous())
    _, _, maps, _ = ex.gradcam(G[:1].to(DEV), P[:1].to(DEV), TQ, tproj, torch.tensor([tokens], device=DEV), size)
    for i, t in enumerate(tokens):
        r64 = gr.gradcam(G[0], P[0], T[0], hsd, kw["num_heads"], t, size, torch.float64)
        d, d32 = gr.abs_dev(maps[0, i].cpu(), r64["map"]), gr.abs_dev(g["gradcam_maps"][i], r64["map"])
        print(f"golden gradcam t={t}: device {d:.3e} recorded f32 {d32:.3e}")
        assert d <= gr.BOUND_FACTOR * d32
    tokens, steps = [int(t) for t in g["ig_tokens"]], int(g["ig_steps"])
    _, maps = ex.integrated_gradients(P[:1].to(DEV), TQ, tproj, torch.tensor([tokens], device=DEV), steps, size)
    for i, t in enumerate(tokens):
        r64 = gr.integrated_gradients(P[0], T[0], hsd, kw["num_heads"], t, size, steps, torch.float64)
        d, d32 = gr.abs_dev(maps[0, i].cpu(), r64["map"]), gr.abs_dev(g["ig_maps"][i], r64["map"])
        print(f"golden ig t={t}: device {d:.3e} recorded f32 {d32:.3e}")
        assert d <= gr.BOUND_FACTOR * d32
