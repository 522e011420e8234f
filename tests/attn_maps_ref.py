"""Plain-torch restatement of the reference's return_attention maps (src/Model/fusion.py:412-433,
model.py:396-399), shared by test_attn_maps_cpu.py and test_attn_maps_gpu.py: the enhancers from
oracle/towers.py, then nn.MultiheadAttention's in_proj slices and its default returned weights
(softmax(q k^T / sqrt(dh)) averaged over the heads; eval, no key mask).  Runs in the dtype of its inputs."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from mmr_amd import synthetic
from oracle import towers as otw

from conftest import GOLDEN

KINDS = ("comb", "txt2img", "img2txt")


def mha_weights(q_in, k_in, sd, p, heads):
    E = sd[p + "in_proj_weight"].shape[1]
    W, b = sd[p + "in_proj_weight"], sd[p + "in_proj_bias"]
    q, k = F.linear(q_in, W[:E], b[:E]), F.linear(k_in, W[E:2 * E], b[E:2 * E])
    B, dh = q.shape[0], E // heads
    qh = q.view(B, -1, heads, dh).transpose(1, 2)
    kh = k.view(B, -1, heads, dh).transpose(1, 2)
    return (qh @ kh.transpose(-1, -2) / math.sqrt(dh)).softmax(-1).mean(1)


def attention_maps(img_global, img_patches, txt_feats, sd, heads, eps=1e-5):
    """{layer_{i}_comb (B, Np+2, Np+2), layer_{i}_txt2img (B, L, Np), layer_{i}_img2txt (B, Np, L)}."""
    nl = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("fusion_layers."))
    lin = lambda x, p: F.linear(x, sd[p + ".weight"], sd[p + ".bias"])  # noqa: E731
    out = {}
    for i in range(nl):
        p = f"fusion_layers.{i}."
        t_in = txt_feats if txt_feats is not None else sd[p + "default_txt_token"].expand(img_patches.shape[0], -1, -1)
        txt = otw.prefusion_enhancer(t_in, sd, p + "txt_self_attn.", heads, eps)
        pt = otw.prefusion_enhancer(img_patches, sd, p + "img_patch_self_attn.", heads, eps)
        seq = otw.cross_modal_fusion(img_global, img_patches, txt_feats, sd, p, heads, False, eps)
        seq = seq + sd["pos_encoder.pe"][:, :seq.shape[1]]
        out[f"layer_{i}_comb"] = mha_weights(seq, seq, sd, "self_attn.", heads)
        out[f"layer_{i}_txt2img"] = mha_weights(lin(txt, p + "query_txt"), lin(pt, p + "key_img"), sd,
                                                p + "attn_txt2img.", heads)
        out[f"layer_{i}_img2txt"] = mha_weights(lin(pt, p + "query_img"), lin(txt, p + "key_txt"), sd,
                                                p + "attn_img2txt.", heads)
    return out


def towers_mini():
    """towers_mini.npz -> (npz, {prefix: f32 state dict} for swin / bert / head)."""
    f = np.load(os.path.join(GOLDEN, "towers_mini.npz"), allow_pickle=False)
    w = {k[2:]: torch.from_numpy(synthetic.bf16_bits_to_f32(f[k]).copy()) for k in f.files if k.startswith("w:")}
    return f, {pre: {k[5:]: v for k, v in w.items() if k.startswith(pre + ".")} for pre in ("swin", "bert", "head")}


def max_abs(got, ref):
    return (got.detach().double().cpu() - ref.detach().double().cpu()).abs().max().item()
