"""Grad-CAM and Integrated-Gradients maps over the image patch features (the gradient family of the reference's
ExplanationEngine, src/Model/explain.py:170-427) without autograd: the reference differentiates ONE CrossModalFusion
layer (the last, model.py:629-635) plus the classifier with respect to the patch features only — a fixed graph of
linears, LayerNorms, three softmax attentions and a GELU — so the backward is written out by hand over ops.

What is computed (restated, not "fixed"): seq = CrossModalFusion_last(img_global, P, T) (Np + 2, D) = [x1; patches_fused;
x2], logits = classifier(seq) (Np + 2, C) — the classifier runs on every token, so a target t selects a TOKEN:
  Grad-CAM  s = sum_c logits[t, c]; img_global is the backbone's vector, a constant; cam_j = relu(sum_e dS/dP_je P_je);
            G x G -> bilinear -> min-max over the pixels -> nan_to_num
  IG        s(P) = logits[t, t]; img_global = mean_j P_j carries gradient; baseline 0; Captum's default rule is
            Gauss-Legendre: alpha_s = (1 + x_s) / 2, w_s = omega_s / 2 for (x, omega) = leggauss(n_steps);
            A = (sum_s w_s dS/dP(alpha_s P)) o P; a_j = sum_e |A_je|; min-max over the patches, clamp -> bilinear
Out of scope: the unimodal maps (ExplanationEngine.image_proj / text_proj are freshly initialised random nn.Linears,
explain.py:31-32: nothing to match), gradients through the other fusion layers, the combiner or the towers, token
attributions, overlays, row-sharded execution.

The pass owns f32 copies of the last layer's weights and their transposes, built on first use, whatever tower_dtype
is: the maps are those of the f32 layer on the towers' features.  Forward with saved intermediates over a batch of
patch sets (Grad-CAM: the B samples; IG: the B x S scaled sets alpha_s P with g = mean), the text side (enhancer,
q_t2i / k_i2t / v_i2t, txt_proj of the CLS row — constant in P) once per sample.  Backward per target slot from the
seed dseq[t] = W1^T (gelu'(h_t) o W2^T c) — c = 1 for Grad-CAM, e_t for IG: the interface is (token, class-weight
vector) — through the three routes (t = 0: ln_img -> txt2img out_proj / attention dK, dV -> folded k|v projection, in
IG also img_global_proj -> global enhancer -> / Np onto every patch; 1 <= t <= Np: img_patch_proj and img2txt
attention dQ of row t - 1; t = Np + 1: ln_txt -> img2txt attention dQ of all rows), then the patch enhancer's backward
(LN with alpha, out_proj, self-attention dq | dk | dv, in_proj).  Rows that a target does not reach carry zeros, so
one code path serves every token kind.

Kernels: linear data gradients are ops.linear_f32 on transposed weights (exact f32; linear_x3's bf16x3 products are
~2^-17 each, above the error bound the tests hold this path to); attention forward / backward, LayerNorm backward,
GELU and the map kernels are csrc/explain_grad.hip; means over tokens are ops.x3_mean_rows (a fixed order per set, so
a sample's result does not depend on the batch).  torch is used for elementwise glue only (adds, scalings, gathers).

Workspace: a chunk of patch sets keeps ~(14 Ci + 12 D) Np + 6 D Lt floats per set alive (saved activations, the
expanded text operands, gradient rows) plus, for IG, T x S x Np x Ci gradient floats per sample; samples are
processed in chunks sized so that this stays under `workspace_bytes` (default 1 GiB) — never less than one sample
(S sets) at a time, which is the bound's floor: at Np = 49, Lt = 128, Ci = D = 768, S = 50, T = 5 one sample takes
~0.35 GiB."""
import math

import numpy as np
import torch

from . import ops
from .fusion import _fold


def gauss_legendre(n):
    """Captum's default IntegratedGradients rule ("gausslegendre", approximation_methods.py): alphas (1 + x) / 2 and
    step sizes omega / 2 for numpy.polynomial.legendre.leggauss(n), as float64 arrays."""
    x, w = np.polynomial.legendre.leggauss(int(n))
    return 0.5 * (1.0 + x), 0.5 * w


def _pad_rows(w, mult):
    n = w.shape[0]
    if n % mult == 0:
        return w.contiguous()
    out = torch.zeros((n + mult - n % mult,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
    out[:n] = w
    return out


class GradientExplainer:
    """The gradient pass of one fusion layer + classifier.  sd: that layer's weights under the reference's keys
    (without the "fusion_layers.i." prefix); classifier: (w1 (H, D), b1, w2 (C, H), b2) f32."""

    def __init__(self, sd, classifier, heads, device, eps=1e-5, workspace_bytes=1 << 30):
        dev = torch.device(device)
        self.device, self.heads, self.eps = dev, int(heads), float(eps)
        self.workspace_bytes = int(workspace_bytes)

        def f(t):
            return t.detach().to(dev, torch.float32).contiguous()

        def ft(t):  # the transpose, for the data gradient dX = dY W as a linear on W^T
            return t.detach().to(dev, torch.float32).t().contiguous()
        W = {}
        for name, p in (("t", "txt_self_attn."), ("p", "img_patch_self_attn.")):
            W[name + "_pos"] = f(sd[p + "pos_embed"][0])
            W[name + "_in"], W[name + "_in_b"] = f(sd[p + "self_attn.in_proj_weight"]), f(sd[p + "self_attn.in_proj_bias"])
            W[name + "_o"], W[name + "_o_b"] = f(sd[p + "self_attn.out_proj.weight"]), f(sd[p + "self_attn.out_proj.bias"])
            W[name + "_alpha"] = f(sd[p + "alpha"].reshape(1))
            W[name + "_g"], W[name + "_b"] = f(sd[p + "norm1.weight"]), f(sd[p + "norm1.bias"])
        W["p_in_T"], W["p_o_T"] = ft(sd["img_patch_self_attn.self_attn.in_proj_weight"]), \
            ft(sd["img_patch_self_attn.self_attn.out_proj.weight"])
        self.Ci, self.Ct = int(W["p_in"].shape[1]), int(W["t_in"].shape[1])
        D = int(sd["img_patch_proj.weight"].shape[0])
        self.D = D
        # global enhancer: softmax over one key is 1, so LN(alpha x + out_proj(v_proj(x))) with x = G + pos0 is
        # LN((Wov + alpha I) G + b) (folded in f64, as FusionStack does)
        pg = "img_global_self_attn."
        Ci = self.Ci
        wov, bov = _fold(sd[pg + "self_attn.out_proj.weight"], sd[pg + "self_attn.out_proj.bias"],
                         sd[pg + "self_attn.in_proj_weight"][2 * Ci:], sd[pg + "self_attn.in_proj_bias"][2 * Ci:])
        pos0, ag = sd[pg + "pos_embed"][0, 0].double(), sd[pg + "alpha"].double().reshape(())
        wg = wov + ag * torch.eye(Ci, dtype=torch.float64)
        W["g_w"], W["g_w_T"], W["g_bias"] = f(wg), ft(wg), f(wov @ pos0 + bov + ag * pos0)
        W["g_g"], W["g_b"] = f(sd[pg + "norm1.weight"]), f(sd[pg + "norm1.bias"])
        # cross attentions: the pre-projections folded into nn.MultiheadAttention's in_proj (f64)
        wi1, bi1 = sd["attn_txt2img.in_proj_weight"], sd["attn_txt2img.in_proj_bias"]
        wi2, bi2 = sd["attn_img2txt.in_proj_weight"], sd["attn_img2txt.in_proj_bias"]
        sl = [slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D)]

        def fold(wi, bi, s, name):
            return _fold(wi[s], bi[s], sd[name + ".weight"], sd[name + ".bias"])
        qt, kt, vt = fold(wi1, bi1, sl[0], "query_txt"), fold(wi2, bi2, sl[1], "key_txt"), fold(wi2, bi2, sl[2], "value_txt")
        ki, vi, qi = fold(wi1, bi1, sl[1], "key_img"), fold(wi1, bi1, sl[2], "value_img"), fold(wi2, bi2, sl[0], "query_img")
        W["tq"], W["tq_b"] = f(torch.cat([qt[0], kt[0], vt[0]])), f(torch.cat([qt[1], kt[1], vt[1]]))
        pq = torch.cat([ki[0], vi[0], qi[0]])
        W["pq"], W["pq_T"], W["pq_b"] = f(pq), ft(pq), f(torch.cat([ki[1], vi[1], qi[1]]))
        for name, key in (("pp", "img_patch_proj"), ("o1", "attn_txt2img.out_proj"), ("o2", "attn_img2txt.out_proj"),
                          ("gp", "img_global_proj"), ("tp", "txt_proj")):
            W[name], W[name + "_T"], W[name + "_b"] = f(sd[key + ".weight"]), ft(sd[key + ".weight"]), f(sd[key + ".bias"])
        W["ln_img_g"], W["ln_img_b"] = f(sd["ln_img.weight"]), f(sd["ln_img.bias"])
        W["ln_txt_g"], W["ln_txt_b"] = f(sd["ln_txt.weight"]), f(sd["ln_txt.bias"])
        W["default_txt"] = f(sd["default_txt_token"].reshape(1, 1, -1))
        w1, b1, w2, b2 = (f(t) for t in classifier)
        self.H, self.C = int(w1.shape[0]), int(w2.shape[0])
        W["c1"], W["c1_T"], W["c1_b"] = w1, w1.t().contiguous(), b1
        # the class dimension padded with zero rows / columns to the f32 linear's granularity (cout % 32, cin % 16)
        W["c2"], W["c2_b"] = _pad_rows(w2, 32), _pad_rows(b2, 32)
        W["c2_T"] = _pad_rows(w2, 16).t().contiguous()  # (H, Cpad): u = c W2 as a linear on W2^T
        self.Cpad = int(W["c2_T"].shape[1])
        self.W = W
        for dim, what in ((self.Ci, "img_dim"), (self.Ct, "txt_dim"), (D, "joint_dim")):
            if dim % 32 or (dim // self.heads) % 8 or dim // self.heads > ops.ATTENTION_BWD_MAX_DH:
                raise ValueError(f"explain_gradients: {what} = {dim} with {self.heads} heads is outside the f32 gradient "
                                 f"kernels (dim % 32 == 0, head width % 8 == 0 and <= {ops.ATTENTION_BWD_MAX_DH})")

    # ---- forward ----
    def text_side(self, txt):
        """txt (B, Lt, Ct) f32 -> the per-sample constants: TQ (B, Lt, 3D) = q_t2i | k_i2t | v_i2t and tproj (B, D)"""
        W, h, eps = self.W, self.heads, self.eps
        B, Lt, Ct = txt.shape
        X = (txt + W["t_pos"][:Lt]).reshape(B * Lt, Ct)
        qkv = ops.linear_f32(X, W["t_in"], W["t_in_b"])
        dh = Ct // h
        a = ops.attention_fwd(qkv[:, :Ct], qkv[:, Ct:2 * Ct], qkv[:, 2 * Ct:], B, Lt, Lt, h, dh, 1.0 / math.sqrt(dh))
        Z = ops.linear_f32(a, W["t_o"], W["t_o_b"], residual=X * W["t_alpha"])
        Te = ops.ln_rows(Z, W["t_g"], W["t_b"], eps)
        TQ = ops.linear_f32(Te, W["tq"], W["tq_b"]).view(B, Lt, 3 * self.D)
        tproj = ops.linear_f32(Te.view(B, Lt, Ct)[:, 0], W["tp"], W["tp_b"])
        return TQ, tproj

    def forward_sets(self, P, g_in, TQ, tproj, rep):
        """The layer's forward over N = B * rep patch sets, set n belonging to sample n // rep.  P (N, Np, Ci), g_in
        (N, Ci) the global vector of each set -> the saved intermediates (a dict; "seq" (N, Np + 2, D))."""
        W, h, eps, D, Ci = self.W, self.heads, self.eps, self.D, self.Ci
        N, Np, _ = P.shape
        Lt = TQ.shape[1]
        sc_p, sc_d = 1.0 / math.sqrt(Ci // h), 1.0 / math.sqrt(D // h)
        S = {}
        X = (P + W["p_pos"][:Np]).reshape(N * Np, Ci)
        S["qkv"] = qkv = ops.linear_f32(X, W["p_in"], W["p_in_b"])
        a = ops.attention_fwd(qkv[:, :Ci], qkv[:, Ci:2 * Ci], qkv[:, 2 * Ci:], N, Np, Np, h, Ci // h, sc_p)
        S["Zp"] = Zp = ops.linear_f32(a, W["p_o"], W["p_o_b"], residual=X * W["p_alpha"])
        Pe = ops.ln_rows(Zp, W["p_g"], W["p_b"], eps)
        S["PQ"] = PQ = ops.linear_f32(Pe, W["pq"], W["pq_b"])          # k_t2i | v_t2i | q_i2t
        PP = ops.linear_f32(Pe, W["pp"], W["pp_b"])
        # the text operands once per set (the attention kernels index q / k / v by sequence)
        S["TQx"] = TQx = (TQ if rep == 1 else TQ.repeat_interleave(rep, 0)).reshape(N * Lt, 3 * D)
        att1 = ops.attention_fwd(TQx[:, :D], PQ[:, :D], PQ[:, D:2 * D], N, Lt, Np, h, D // h, sc_d)
        t2i = ops.linear_f32(ops.x3_mean_rows(att1.view(N, Lt, D)), W["o1"], W["o1_b"])
        S["Zg"] = Zg = ops.linear_f32(g_in, W["g_w"], W["g_bias"])
        Ge = ops.ln_rows(Zg, W["g_g"], W["g_b"], eps)
        S["Z1"] = Z1 = ops.linear_f32(Ge, W["gp"], W["gp_b"], residual=t2i)
        a2 = ops.attention_fwd(PQ[:, 2 * D:], TQx[:, D:2 * D], TQx[:, 2 * D:], N, Np, Lt, h, D // h, sc_d)
        att2 = ops.linear_f32(a2, W["o2"], W["o2_b"])
        tp = tproj if rep == 1 else tproj.repeat_interleave(rep, 0)
        S["Z2"] = Z2 = tp + ops.x3_mean_rows(att2.view(N, Np, D))
        seq = torch.empty((N, Np + 2, D), dtype=torch.float32, device=P.device)
        seq[:, 0] = ops.ln_rows(Z1, W["ln_img_g"], W["ln_img_b"], eps)
        seq[:, 1:Np + 1] = (PP + att2).view(N, Np, D)
        seq[:, Np + 1] = ops.ln_rows(Z2.contiguous(), W["ln_txt_g"], W["ln_txt_b"], eps)
        S["seq"] = seq
        return S

    def token_logits(self, seq):
        """classifier(seq) on every token: (N, Np + 2, D) -> (N, Np + 2, C)"""
        W = self.W
        N, L, D = seq.shape
        hpre = ops.linear_f32(seq.reshape(N * L, D), W["c1"], W["c1_b"])
        return ops.linear_f32(ops.gelu_rows(hpre), W["c2"], W["c2_b"])[:, :self.C].reshape(N, L, self.C)

    # ---- backward ----
    def backward_sets(self, S, tok, cw, with_global):
        """dS/dP for one target per set: tok (N,) int64 the token of each set's target, cw (N, Cpad) its class-weight
        vector (score = sum_c cw[c] logits[tok, c]).  with_global: the global vector is mean_j P_j (IG) and carries
        gradient; else it is a constant (Grad-CAM).  -> (N, Np, Ci)."""
        W, h, eps, D, Ci = self.W, self.heads, self.eps, self.D, self.Ci
        seq = S["seq"]
        N, L, _ = seq.shape
        Np = L - 2
        Lt = S["TQx"].shape[0] // N
        sc_p, sc_d = 1.0 / math.sqrt(Ci // h), 1.0 / math.sqrt(D // h)
        rows = torch.arange(N, device=seq.device)
        # seed: dseq[tok] = W1^T (gelu'(h_tok) o W2^T c)
        hpre = ops.linear_f32(seq[rows, tok], W["c1"], W["c1_b"])
        dh_ = ops.gelu_bwd(hpre, ops.linear_f32(cw, W["c2_T"]))
        dseq = ops.linear_f32(dh_, W["c1_T"])                                     # (N, D)
        is0, is2 = (tok == 0)[:, None], (tok == Np + 1)[:, None]
        dx1, dx2 = dseq * is0, dseq * is2
        dPF = torch.zeros((N, Np, D), dtype=torch.float32, device=seq.device)
        mid = (tok >= 1) & (tok <= Np)
        dPF[rows, (tok - 1).clamp(0, Np - 1)] = dseq * mid[:, None]
        dPF = dPF.view(N * Np, D)
        dPQ = torch.empty((N * Np, 3 * D), dtype=torch.float32, device=seq.device)
        TQx, PQ = S["TQx"], S["PQ"]
        # x1 route: ln_img -> (t2i = mean_L att1 . Wo1^T) and (img_global_proj)
        dZ1 = ops.ln_bwd_rows(S["Z1"], W["ln_img_g"], dx1, eps)
        dm1 = ops.linear_f32(dZ1, W["o1_T"])
        dO1 = (dm1 / Lt)[:, None, :].expand(N, Lt, D).contiguous().view(N * Lt, D)  # a copy: rows at stride D
        ops.attention_bwd(TQx[:, :D], PQ[:, :D], PQ[:, D:2 * D], dO1, N, Lt, Np, h, D // h, sc_d, want=("dk", "dv"),
                          out={"dk": dPQ[:, :D], "dv": dPQ[:, D:2 * D]})
        dg = None
        if with_global:
            dGe = ops.linear_f32(dZ1, W["gp_T"])
            dg = ops.linear_f32(ops.ln_bwd_rows(S["Zg"], W["g_g"], dGe, eps), W["g_w_T"])   # (N, Ci)
        # x2 route and the patch tokens: att_i2t rows get dPF + dZ2 / Np
        dZ2 = ops.ln_bwd_rows(S["Z2"], W["ln_txt_g"], dx2, eps)
        dAtt2 = (dPF.view(N, Np, D) + (dZ2 / Np)[:, None, :]).view(N * Np, D)
        dA2 = ops.linear_f32(dAtt2, W["o2_T"])
        ops.attention_bwd(PQ[:, 2 * D:], TQx[:, D:2 * D], TQx[:, 2 * D:], dA2, N, Np, Lt, h, D // h, sc_d, want=("dq",),
                          out={"dq": dPQ[:, 2 * D:]})
        dPe = ops.linear_f32(dPF, W["pp_T"])
        ops.linear_f32(dPQ, W["pq_T"], residual=dPe, out=dPe)
        # the patch enhancer: Pe = LN(alpha X + out_proj(attn(in_proj(X)))), X = P + pos
        dZp = ops.ln_bwd_rows(S["Zp"], W["p_g"], dPe, eps)
        dA = ops.linear_f32(dZp, W["p_o_T"])
        qkv = S["qkv"]
        dqkv = torch.empty_like(qkv)
        ops.attention_bwd(qkv[:, :Ci], qkv[:, Ci:2 * Ci], qkv[:, 2 * Ci:], dA, N, Np, Np, h, Ci // h, sc_p,
                          out={"dq": dqkv[:, :Ci], "dk": dqkv[:, Ci:2 * Ci], "dv": dqkv[:, 2 * Ci:]})
        dX = dZp * W["p_alpha"]
        ops.linear_f32(dqkv, W["p_in_T"], residual=dX, out=dX)
        dP = dX.view(N, Np, Ci)
        if dg is not None:
            dP = dP + (dg / Np)[:, None, :]
        return dP

    def class_weights(self, n, classes=None):
        """(n, Cpad) class-weight rows: all ones over the C classes (Grad-CAM: the class sum), or e_class (IG)"""
        cw = torch.zeros((n, self.Cpad), dtype=torch.float32, device=self.device)
        if classes is None:
            cw[:, :self.C] = 1.0
        else:
            cw[torch.arange(n, device=self.device), classes] = 1.0
        return cw

    def bytes_per_set(self, Np, Lt):
        return 4 * ((14 * self.Ci + 12 * self.D) * Np + 6 * self.D * Lt)

    # ---- the two methods ----
    def gradcam(self, img_global, P, TQ, tproj, targets, image_size):
        """targets (B, T) int64 tokens -> (grads (B, T, Np, Ci), raw (B, T, Np), maps (B, T, H, W) or None,
        token_logits (B, Np + 2, C))"""
        B, Np, Ci = P.shape
        T = targets.shape[1]
        grads = torch.empty((T, B, Np, Ci), dtype=torch.float32, device=P.device)
        logits = torch.empty((B, Np + 2, self.C), dtype=torch.float32, device=P.device)
        bc = max(1, self.workspace_bytes // self.bytes_per_set(Np, TQ.shape[1]))
        for b0 in range(0, B, bc):
            sl = slice(b0, min(B, b0 + bc))
            S = self.forward_sets(P[sl], img_global[sl], TQ[sl], tproj[sl], 1)
            logits[sl] = self.token_logits(S["seq"])
            cw = self.class_weights(S["seq"].shape[0])
            for t in range(T):
                grads[t, sl] = self.backward_sets(S, targets[sl, t], cw, with_global=False)
        raw, maps = ops.attribution_maps(grads.view(T * B, Np, Ci), P, "gradcam", image_size=image_size,
                                         target_major=True)
        maps = None if maps is None else maps.view(T, B, *maps.shape[1:]).transpose(0, 1).contiguous()
        return grads.transpose(0, 1), raw.view(T, B, Np).transpose(0, 1).contiguous(), maps, logits

    def integrated_gradients(self, P, TQ, tproj, targets, steps, image_size):
        """targets (B, T) int64 (token = class) -> (raw (B, T, Np) = sum_e |(sum_s w_s dS/dP(alpha_s P)) o P|, maps
        (B, T, H, W) or None)"""
        B, Np, Ci = P.shape
        T, Sn = targets.shape[1], int(steps)
        al, wt = gauss_legendre(Sn)
        al = torch.tensor(al, dtype=torch.float32, device=P.device)
        wt = torch.tensor(wt, dtype=torch.float32, device=P.device)
        per_sample = Sn * self.bytes_per_set(Np, TQ.shape[1]) + 4 * T * Sn * Np * Ci
        bc = max(1, self.workspace_bytes // per_sample)
        raws, maps = [], []
        for b0 in range(0, B, bc):
            sl = slice(b0, min(B, b0 + bc))
            n = sl.stop - sl.start
            Ps = (P[sl, None] * al[None, :, None, None]).reshape(n * Sn, Np, Ci)   # set (b, s) = alpha_s P_b
            S = self.forward_sets(Ps, ops.x3_mean_rows(Ps), TQ[sl], tproj[sl], Sn)
            grads = torch.empty((T, n * Sn, Np, Ci), dtype=torch.float32, device=P.device)
            for t in range(T):
                tok = targets[sl, t].repeat_interleave(Sn)
                grads[t] = self.backward_sets(S, tok, self.class_weights(n * Sn, tok), with_global=True)
            r, m = ops.attribution_maps(grads.view(T * n * Sn, Np, Ci), P[sl], "ig", steps=Sn, step_w=wt,
                                        image_size=image_size, target_major=True)
            raws.append(r.view(T, n, Np).transpose(0, 1))
            maps.append(None if m is None else m.view(T, n, *m.shape[1:]).transpose(0, 1))
            del S, grads
        raw = torch.cat(raws).contiguous()
        return raw, (None if maps[0] is None else torch.cat(maps).contiguous())
