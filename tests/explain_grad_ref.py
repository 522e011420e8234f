"""Restatement of the reference's gradient explanations (src/Model/explain.py:170-427, multimodal form) in plain torch
autograd, in f64 (the yardstick) or f32 (the reference's own arithmetic, whose deviation from f64 sets the bound):
the last CrossModalFusion layer through oracle.towers.cross_modal_fusion, the classifier on EVERY token, so that a
target t selects a token.

  Grad-CAM (:237-300)  s = sum_c logits[t, c], img_global constant; cam_j = relu(sum_e dS/dP_je P_je); G x G, bilinear
                       (align_corners=False) to image_size, THEN (m - min) / (max - min + 1e-8), nan_to_num
  IG (:373-427)        s(P) = logits[t, t], img_global = mean_j P_j; baseline 0; Captum's default Gauss-Legendre rule:
                       alpha_s = (1 + x_s) / 2, w_s = omega_s / 2 for numpy.polynomial.legendre.leggauss(n);
                       A = (sum_s w_s dS/dP(alpha_s P)) o P; a_j = sum_e |A_je|; (a - min) / (max - min + 1e-8), clamp,
                       THEN bilinear

The bound (BOUND_FACTOR): a device result may deviate from the f64 restatement by at most 8 x the deviation of the
f32 restatement from it, both normalised the same way — by the tensor's max-abs for gradients and raw vectors,
absolutely for maps in [0, 1].  Both are f32 chains of the same length whose summation orders differ; a dropped term
shows at >= 1e-3 relative, three orders above.

`mutant`: deliberately wrong variants the bound has to reject (test_explain_grad_cpu.py)."""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import towers as otw

BOUND_FACTOR = 8.0
MUTANTS = ("softmax_jacobian", "ig_global", "order", "score", "rectangle")


def layer_state(hsd, layer, dtype):
    """(fusion + classifier weights in dtype, the layer's prefix)"""
    nl = 1 + max(int(k.split(".")[1]) for k in hsd if k.startswith("fusion_layers."))
    layer = layer + nl if layer < 0 else layer
    p = f"fusion_layers.{layer}."
    sd = {k: v.to(dtype) for k, v in hsd.items() if k.startswith(p) or k.startswith("classifier.")}
    return sd, p


def _mha_no_jacobian(q_in, k_in, v_in, sd, p, heads):
    """oracle.towers.mha whose softmax backward keeps only the diagonal term dS = P o dP (the rowsum term dropped);
    the forward value is the softmax's"""
    E = sd[p + "in_proj_weight"].shape[1]
    W, b = sd[p + "in_proj_weight"], sd[p + "in_proj_bias"]
    q = F.linear(q_in, W[:E], b[:E])
    k = F.linear(k_in, W[E:2 * E], b[E:2 * E])
    v = F.linear(v_in, W[2 * E:], b[2 * E:])
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    dh = E // heads

    def hd(t, L):
        return t.view(B, L, heads, dh).transpose(1, 2)
    s = hd(q, Lq) @ hd(k, Lk).transpose(-1, -2) / math.sqrt(dh)
    pr = s.softmax(-1).detach()
    pr = pr * (s - s.detach() + 1.0)
    return F.linear((pr @ hd(v, Lk)).transpose(1, 2).reshape(B, Lq, E), sd[p + "out_proj.weight"],
                    sd[p + "out_proj.bias"])


@contextlib.contextmanager
def _patched_mha(on):
    if not on:
        yield
        return
    keep = otw.mha
    otw.mha = _mha_no_jacobian
    try:
        yield
    finally:
        otw.mha = keep


def token_logits(img_global, P, txt, sd, p, heads):
    """classifier(CrossModalFusion(img_global, P, txt)): (B, Np + 2, C)"""
    seq = otw.cross_modal_fusion(img_global, P, txt, sd, p, heads, False)
    h = F.gelu(F.linear(seq, sd["classifier.0.weight"], sd["classifier.0.bias"]))
    return F.linear(h, sd["classifier.3.weight"], sd["classifier.3.bias"])


def score_grad(img_global, P, txt, sd, p, heads, token, cw, mutant=None):
    """d(sum_c cw[c] logits[:, token, c]) / dP for a batch of patch sets; img_global None: mean_j P_j (with gradient).
    -> (grad like P, logits detached)"""
    P = P.clone().requires_grad_(True)
    g = img_global
    if g is None:
        g = P.mean(1)
        if mutant == "ig_global":
            g = g.detach()
    with _patched_mha(mutant == "softmax_jacobian"):
        logits = token_logits(g, P, txt, sd, p, heads)
    s = (logits[:, token] * cw).sum()
    return torch.autograd.grad(s, P)[0], logits.detach()


def upsample(v, size):
    g = math.isqrt(v.numel())
    return F.interpolate(v.view(1, 1, g, g), size=tuple(size), mode="bilinear", align_corners=False)[0, 0]


def minmax(v):
    return (v - v.min()) / (v.max() - v.min() + 1e-8)


def gradcam(img_global, P, txt, hsd, heads, token, size, dtype=torch.float64, layer=-1, mutant=None):
    """one sample: img_global (Ci,), P (Np, Ci), txt (Lt, Ct) or None -> {"grad" (Np, Ci), "raw" (Np,) before the relu,
    "map" (H, W), "logits" (Np + 2, C)}"""
    sd, p = layer_state(hsd, layer, dtype)
    C = sd["classifier.3.weight"].shape[0]
    cw = torch.ones(C, dtype=dtype)
    if mutant == "score":  # the IG score in Grad-CAM's place
        cw = torch.zeros(C, dtype=dtype)
        cw[token] = 1.0
    t = None if txt is None else txt.to(dtype)[None]
    grad, logits = score_grad(img_global.to(dtype)[None], P.to(dtype)[None], t, sd, p, heads, token, cw, mutant)
    raw = (grad[0] * P.to(dtype)).sum(-1)
    cam = torch.relu(raw)
    m = upsample(minmax(cam), size) if mutant == "order" else minmax(upsample(cam, size))
    m = torch.nan_to_num(m, nan=0.0, posinf=1.0, neginf=0.0)
    return {"grad": grad[0], "raw": raw, "map": m, "logits": logits[0]}


def ig_rule(n, mutant=None):
    if mutant == "rectangle":  # left rectangles in Gauss-Legendre's place
        return np.arange(n) / n, np.full(n, 1.0 / n)
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (1.0 + x), 0.5 * w


def integrated_gradients(P, txt, hsd, heads, token, size, steps=50, dtype=torch.float64, layer=-1, mutant=None):
    """one sample -> {"grad" (Np, Ci) = sum_s w_s dS/dP(alpha_s P), "raw" (Np,) = sum_e |grad o P|, "map" (H, W)}"""
    sd, p = layer_state(hsd, layer, dtype)
    C = sd["classifier.3.weight"].shape[0]
    cw = torch.zeros(C, dtype=dtype)
    cw[token] = 1.0
    if mutant == "score":  # Grad-CAM's class sum in IG's place
        cw = torch.ones(C, dtype=dtype)
    al, wt = ig_rule(steps, mutant)
    al, wt = torch.tensor(al, dtype=dtype), torch.tensor(wt, dtype=dtype)
    Pd = P.to(dtype)
    sets = al[:, None, None] * Pd[None]
    t = None if txt is None else txt.to(dtype)[None].expand(steps, -1, -1)
    grads, _ = score_grad(None, sets, t, sd, p, heads, token, cw, mutant)
    total = (grads * wt[:, None, None]).sum(0)
    raw = (total * Pd).abs().sum(-1)
    if mutant == "order":
        m = minmax(upsample(raw, size)).clamp(0.0, 1.0)
    else:
        a = torch.nan_to_num(minmax(raw).clamp(0.0, 1.0), nan=0.0, posinf=1.0, neginf=0.0)
        m = upsample(a, size)
    return {"grad": total, "raw": raw, "map": m}


def rel_dev(got, ref):
    """max |got - ref| / max |ref| (gradients, raw vectors); an all-zero ref (a target that P does not reach: x2 with
    the one-token default text) gives max |got|, so that only exact zeros pass"""
    ref = torch.as_tensor(ref).double()
    top = float(ref.abs().max())
    return float((torch.as_tensor(got).double() - ref).abs().max()) / (top if top > 0.0 else 1.0)


def abs_dev(got, ref):
    """max |got - ref| (maps in [0, 1])"""
    return float((torch.as_tensor(got).double() - torch.as_tensor(ref).double()).abs().max())


def cond(v):
    """max / (max - min) of a vector that gets min-max normalised: the factor by which its relative error grows"""
    v = torch.as_tensor(v).double()
    return float(v.abs().max() / (v.max() - v.min()))
