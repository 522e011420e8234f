"""Swin-Tiny image tower and ClinicalBERT (BERT-base geometry) text tower on libmmr kernels.

Weights load from reference-style state dicts (timm key names for Swin — what
Backbones.__init__ builds with timm.create_model, fusion.py:81-110 — and HF BertModel key names
for the text tower, fusion.py:186) by load_swin_blocks / load_bert_layers (shared with the x3 towers,
towers_x3.py, which pass their own weight converter) and are laid out once for the device:
linear weights bf16 [out][in] (QKV fused into one [3C][C] GEMM), biases / LN / rel-pos tables f32,
the 4x4/s4 patch-embed conv as a [96][64] bf16 GEMM weight (K = 3*16 zero-padded to 64).

Per-block dataflow (all hand-written kernels, bf16 activations, f32 accumulation):
  Swin block   LN1 -> QKV GEMM(+bias) -> window attention (roll/partition/bias/mask/softmax/PV/
               reverse/roll fused) -> proj GEMM(+bias +residual) [for C = 96 the whole attention
               half is ONE kernel, mmr_swin_attn_block] -> LN2 -> fc1 GEMM(+bias, GELU)
               -> fc2 GEMM(+bias +residual); for C = 96 / 192 the MLP half is ONE fused kernel
               (mmr_swin_mlp: LN2 + fc1 + GELU + fc2 + residual, hidden kept on chip)
  PatchMerge   gather 2x2 + LN(4C) fused -> reduction GEMM (no bias)
  BERT layer   QKV GEMM(+bias) -> masked attention -> out GEMM(+bias) -> LN(+residual) ->
               FFN1 GEMM(+bias, GELU) -> FFN2 GEMM(+bias) -> LN(+residual)   (post-LN residual
               adds ride in the LayerNorm kernel, so the GEMMs run the residual-free epilogue)
"""

import torch

from . import ops

SWIN_T = dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, img_size=224,
              patch=4, in_chans=3)
# timm Swin names -> geometry (timm swin_transformer.py model defs); the reference's default is
# swin_base_patch4_window7_224 (fusion.py:45, model.py:124), the north star's Swin-Tiny
SWIN_ARCHS = {
    "swin_tiny_patch4_window7_224": SWIN_T,
    "swin_small_patch4_window7_224": dict(SWIN_T, depths=[2, 2, 18, 2]),
    "swin_base_patch4_window7_224": dict(SWIN_T, embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32]),
    "swin_large_patch4_window7_224": dict(SWIN_T, embed_dim=192, depths=[2, 2, 18, 2], num_heads=[6, 12, 24, 48]),
}
BERT_BASE = dict(vocab_size=28996, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                 intermediate_size=3072, max_position_embeddings=512, type_vocab_size=2)


def _bf(t, dev):
    return t.detach().to(device=dev, dtype=torch.bfloat16).contiguous()


def _f(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _w8(w, plain=False):
    """nn.Linear weight (bf16, device) -> its MX-fp8 operand (quantised once, at load).  plain: the
    layer's GEMM has no residual epilogue, so it takes 256 x 256 tiles (weight panels of 256 rows,
    layout 2) when N % 256 == 0 (measured faster, GELU included: FFN1 1035 -> 1191 TF/s); residual
    epilogues keep 256 x 192 (layout 1)."""
    return ops.quantize_mxfp8(w, layout=2 if plain and w.shape[0] % 256 == 0 else 1)


def _rw(w):
    """Resident-weight streaming image for the short-K linears (K = 64 / 192: patch embed, stage-2
    qkv / proj; tools/rw_bench.py: 1.1-1.4x the tuned GEMM there, slower at K = 384), else None."""
    return ops.rw_pack(w) if w.shape[1] in (64, 192) else None


def _pad_rows(t2, rows_p):
    """2-D rows zero-padded to rows_p (the MX-fp8 operands and GEMM tiles take 256-row multiples:
    a batch of any size — B = 1 serving, a ragged last batch — runs the same fp8 arithmetic on its
    real rows; the padded rows are discarded)."""
    if t2 is None or t2.shape[0] == rows_p:
        return t2
    out = torch.zeros((rows_p,) + tuple(t2.shape[1:]), dtype=t2.dtype, device=t2.device)
    out[:t2.shape[0]] = t2
    return out


def _rows256(x):
    rows = x.numel() // x.shape[-1]
    return rows, -(-rows // 256) * 256


def _timed(ev, name, fn, *args, **kw):
    """fn(*args, **kw) with a HIP event pair around it appended to ev[name] (ev None: just the call)."""
    if ev is None:
        return fn(*args, **kw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn(*args, **kw)
    e1.record()
    ev.setdefault(name, []).append((e0, e1))
    return out


def _mlp8(h, w1_8, b1, w2_8, b2, residual=None, h8=None, ev=None):
    """fc1 (+ GELU) -> fc2 on the MX-fp8 path with fc1's epilogue emitting fc2's fp8 operand
    (mmr_linear_mxfp8_q8): the hidden activation never exists in bf16.  h8: h's fp8 operand when
    the producing LayerNorm already emitted it (rows a multiple of 256).  ev: per-GEMM event dict
    ("ffn1" / "ffn2"), as BertTower.gemm_events."""
    K = h.shape[-1]
    rows, rp = _rows256(h)
    x8 = h8 if h8 is not None else ops.quantize_mxfp8(_pad_rows(h.reshape(-1, K), rp), layout=0, kp=w1_8.kp)
    f8 = _timed(ev, "ffn1", ops.linear_mxfp8_q8, x8, w1_8, b1, act=1)
    r = None if residual is None else _pad_rows(residual.reshape(rows, -1), rp)
    y = _timed(ev, "ffn2", ops.linear_mxfp8, f8, w2_8, b2, r)
    return (y if rp == rows else y[:rows]).reshape(tuple(h.shape[:-1]) + (y.shape[-1],))


def _ln8_ok(x, w8):
    """The LayerNorm can emit the fp8 operand itself: rows a multiple of 256, C of 32 (K padded to the
    weight's kp, e.g. stage 3's C = 384 -> 512, is written by the LayerNorm too)."""
    C = x.shape[-1]
    return w8 is not None and C % 32 == 0 and (x.numel() // C) % 256 == 0 and w8.kp >= C


def _lin(x, w, b=None, residual=None, act=0, w8=None):
    """nn.Linear through the bf16 GEMM, or through the MX-fp8 GEMM when the layer holds w8: the
    activation is quantised per 32-block (mmr_quantize_mxfp8) and the block-scaled MFMA GEMM
    applies bias / GELU / residual in f32 (BASELINE config 5's fp8 towers).  Rows are zero-padded
    to a multiple of 256 when needed (_pad_rows)."""
    if w8 is None:
        return ops.linear(x, w, b, residual=residual, act=act)
    K = x.shape[-1]
    rows, rp = _rows256(x)
    x8 = ops.quantize_mxfp8(_pad_rows(x.reshape(-1, K), rp), layout=0, kp=w8.kp)
    r = None if residual is None else _pad_rows(residual.reshape(rows, -1), rp)
    if rp == rows:
        return ops.linear_mxfp8(x8, w8, b, r, act=act, lead=tuple(x.shape[:-1]))
    y = ops.linear_mxfp8(x8, w8, b, r, act=act)
    return y[:rows].reshape(tuple(x.shape[:-1]) + (y.shape[-1],))


def _fused_stem_ok(pe_pack, image, g):
    """The one-pass stem (conv + LayerNorm, built for Swin-T's 4 x 4 / 3 -> 96 conv) takes this image."""
    return pe_pack is not None and image.shape[1] == 3 and image.shape[2] == image.shape[3] and (g * g) % 32 == 0


def _text_inputs(input_ids, attention_mask, dev, max_len):
    """(ids, mask) int64 on dev, contiguous; mask defaults to ones; L truncated to max_len
    (max_position_embeddings, like fusion.py:315-320)."""
    ids = input_ids.to(dev, torch.int64)
    if attention_mask is None:
        attention_mask = torch.ones_like(ids)
    mask = attention_mask.to(dev, torch.int64)
    if ids.shape[1] > max_len:
        ids, mask = ids[:, :max_len], mask[:, :max_len]
    return ids.contiguous(), mask.contiguous()


def load_swin_blocks(sd, cfg, dev, conv):
    """timm Swin state dict -> one dict per stage: "blocks" (one dict per block: the linears' "<name>_w"
    = conv(weight, dev), f32 "<name>_b", LayerNorms "n1g" / "n1b" / "n2g" / "n2b", the block's "shift" and
    its (heads, ws*ws, ws*ws) attention "bias" with the shift mask folded in), the stage's resolution "res"
    and window "ws", and from stage 1 on the PatchMerging "ds_g" / "ds_b" / "ds_w".  conv is _bf (bf16
    towers) or towers_x3._x3.  The shift / window / resolution schedule lives here only; each tower adds
    its own packs and fp8 operands to these dicts."""
    stages = []
    res = cfg["img_size"] // cfg["patch"]
    ws0 = cfg["window_size"]
    for i, depth in enumerate(cfg["depths"]):
        st = {"blocks": []}
        if i > 0:
            res //= 2
            p = f"layers.{i}.downsample."
            st["ds_g"], st["ds_b"] = _f(sd[p + "norm.weight"], dev), _f(sd[p + "norm.bias"], dev)
            st["ds_w"] = conv(sd[p + "reduction.weight"], dev)
        ws = min(ws0, res)
        st["res"], st["ws"] = res, ws
        for j in range(depth):
            p = f"layers.{i}.blocks.{j}."
            shift = 0 if (j % 2 == 0 or res <= ws0) else ws0 // 2
            table = _f(sd[p + "attn.relative_position_bias_table"], dev)
            st["blocks"].append({
                "shift": shift,
                "bias": ops.swin_attn_bias(table, cfg["num_heads"][i], ws, res, shift),
                "n1g": _f(sd[p + "norm1.weight"], dev), "n1b": _f(sd[p + "norm1.bias"], dev),
                "qkv_w": conv(sd[p + "attn.qkv.weight"], dev), "qkv_b": _f(sd[p + "attn.qkv.bias"], dev),
                "proj_w": conv(sd[p + "attn.proj.weight"], dev), "proj_b": _f(sd[p + "attn.proj.bias"], dev),
                "n2g": _f(sd[p + "norm2.weight"], dev), "n2b": _f(sd[p + "norm2.bias"], dev),
                "fc1_w": conv(sd[p + "mlp.fc1.weight"], dev), "fc1_b": _f(sd[p + "mlp.fc1.bias"], dev),
                "fc2_w": conv(sd[p + "mlp.fc2.weight"], dev), "fc2_b": _f(sd[p + "mlp.fc2.bias"], dev),
            })
        stages.append(st)
    return stages


def load_bert_layers(sd, cfg, dev, conv):
    """HF BertModel state dict -> one dict per encoder layer: "qkv_w" (query | key | value stacked into one
    [3C][C] weight), "o_w", "i_w", "f_w" = conv(weight, dev), their f32 biases "<name>_b" and the two
    post-LayerNorms "ln1_g" / "ln1_b" / "ln2_g" / "ln2_b".  conv as in load_swin_blocks."""
    layers = []
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        qkv_w = torch.cat([sd[p + f"attention.self.{n}.weight"] for n in ("query", "key", "value")], 0)
        qkv_b = torch.cat([sd[p + f"attention.self.{n}.bias"] for n in ("query", "key", "value")], 0)
        layers.append({
            "qkv_w": conv(qkv_w, dev), "qkv_b": _f(qkv_b, dev),
            "o_w": conv(sd[p + "attention.output.dense.weight"], dev),
            "o_b": _f(sd[p + "attention.output.dense.bias"], dev),
            "ln1_g": _f(sd[p + "attention.output.LayerNorm.weight"], dev),
            "ln1_b": _f(sd[p + "attention.output.LayerNorm.bias"], dev),
            "i_w": conv(sd[p + "intermediate.dense.weight"], dev), "i_b": _f(sd[p + "intermediate.dense.bias"], dev),
            "f_w": conv(sd[p + "output.dense.weight"], dev), "f_b": _f(sd[p + "output.dense.bias"], dev),
            "ln2_g": _f(sd[p + "output.LayerNorm.weight"], dev), "ln2_b": _f(sd[p + "output.LayerNorm.bias"], dev),
        })
    return layers


class SwinTower:
    """timm SwinTransformer.forward_features semantics (see oracle/towers.py for the restatement).
    fp8_stages: stages whose linears (qkv, proj, fc1, fc2 and the incoming PatchMerging reduction)
    run as MX-fp8 GEMMs (config 5 uses (2, 3); the batch must make B * tokens a multiple of 256)."""

    def __init__(self, sd, cfg=SWIN_T, device="cuda", fused_mlp=True, fused_attn=True, fp8_stages=()):
        self.cfg = dict(SWIN_T, **cfg)
        self.fp8_stages = tuple(fp8_stages)
        self.fused_mlp = fused_mlp
        self.fused_attn = fused_attn
        dev = torch.device(device)
        self.device = dev
        E = self.cfg["embed_dim"]
        w = sd["patch_embed.proj.weight"].reshape(E, -1)          # [E][cin*16], (c, ky, kx) order
        wp = torch.zeros((E, 64), dtype=torch.float32)
        wp[:, :w.shape[1]] = w
        self.pe_w, self.pe_b = _bf(wp, dev), _f(sd["patch_embed.proj.bias"], dev)
        self.pe_rw = _rw(self.pe_w)
        self.pe_g, self.pe_beta = _f(sd["patch_embed.norm.weight"], dev), _f(sd["patch_embed.norm.bias"], dev)
        # the fused stem (mmr_patch_embed_ln_bf16) for Swin-T's 4 x 4 / 3 -> 96 conv: its pack built from the
        # bf16-rounded weight, so the hi image IS the bf16 conv weight
        self.pe_pack = (ops.x3_patch_embed_pack(self.pe_w[:, :w.shape[1]].float().contiguous())
                        if self.cfg["patch"] == 4 and tuple(w.shape) == (96, 48) else None)
        self.stages = load_swin_blocks(sd, self.cfg, dev, _bf)
        for i, st in enumerate(self.stages):
            fp8 = i in self.fp8_stages
            if i > 0:
                st["ds_w8"] = _w8(st["ds_w"], plain=True) if fp8 else None
            # the one-kernel attention half is built for C = 96 with 3 heads of 32 and 7 x 7 windows
            sab = (self.fused_attn and not fp8 and E * 2 ** i == 96 and self.cfg["num_heads"][i] == 3
                   and st["ws"] == 7)
            for bk in st["blocks"]:
                for n in ("qkv", "proj", "fc1", "fc2"):
                    bk[n + "_w8"] = _w8(bk[n + "_w"], plain=n in ("qkv", "fc1")) if fp8 else None
                for n in ("qkv", "proj"):  # short-K linears (stage 2): resident-weight streaming kernel
                    bk[n + "_rw"] = _rw(bk[n + "_w"]) if not fp8 else None
                bk["mlp_pack"] = ops.swin_mlp_pack(bk["fc1_w"], bk["fc2_w"]) if self.fused_mlp and not fp8 else None
                bk["attn_pack"] = (ops.swin_attn_block_pack(bk["qkv_w"], bk["qkv_b"], bk["proj_w"], bk["proj_b"],
                                                            bk["n1g"], bk["n1b"]) if sab else None)
        self.norm_g, self.norm_b = _f(sd["norm.weight"], dev), _f(sd["norm.bias"], dev)
        self.num_features = E * 2 ** (len(self.cfg["depths"]) - 1)

    def tokens(self, image):
        """(B,3,H,W) f32 -> (B, h, w, C) bf16 tokens BEFORE the final norm."""
        cfg = self.cfg
        image = image.to(self.device, torch.float32).contiguous()
        g = cfg["img_size"] // cfg["patch"]
        if _fused_stem_ok(self.pe_pack, image, g):
            x = ops.patch_embed_ln_bf16(image, self.pe_pack, self.pe_b, self.pe_g, self.pe_beta, 1e-5)
        else:
            cols = ops.patch_im2col(image, cfg["patch"])
            x = (ops.linear_rw(cols, self.pe_rw, self.pe_b) if self.pe_rw is not None
                 else ops.linear(cols, self.pe_w, self.pe_b))                 # (B, g*g, E)
            x = ops.layernorm(x, self.pe_g, self.pe_beta, 1e-5).view(image.shape[0], g, g, -1)
        for i, st in enumerate(self.stages):
            if i > 0:
                x = self._downsample(x, st)
            H = x.shape[1]
            heads = cfg["num_heads"][i]
            ws = min(cfg["window_size"], H)
            for bk in st["blocks"]:
                x = self._mlp_half(self._attn_half(x, bk, H, heads, ws), bk)
        return x

    def _downsample(self, x, st):
        """PatchMerging into stage st: gather 2 x 2 + LayerNorm(4C) -> reduction GEMM (no bias)."""
        w8 = st["ds_w8"]
        B, H2 = x.shape[0], x.shape[1] // 2
        if (w8 is not None and (B * H2 * H2) % 256 == 0 and w8.kp == 4 * x.shape[-1]
                and w8.kp <= 2048):  # the gather + LN writes the reduction's fp8 operand
            _, m8 = ops.patch_merge_ln_q8(x, st["ds_g"], st["ds_b"], 1e-5)
            return ops.linear_mxfp8(m8, w8, None, lead=(B, H2, H2))
        return _lin(ops.patch_merge_ln(x, st["ds_g"], st["ds_b"], 1e-5), st["ds_w"], w8=w8)

    def _attn_half(self, x, bk, H, heads, ws):
        """x + proj(W-MSA(norm1(x))) of one block: one kernel where the block holds attn_pack (C = 96), the
        fp8 chain where the LayerNorm can emit the QKV operand, else LN -> QKV -> window attention -> proj
        (resident-weight linears at short K, else the bf16 / fp8 GEMM)."""
        if bk["attn_pack"] is not None:
            return ops.swin_attn_block(x, bk["attn_pack"], bk["bias"], ws, bk["shift"], 1e-5)
        if _ln8_ok(x, bk["qkv_w8"]):  # fp8 stage: the LN emits the QKV operand (no bf16 rows)
            lead = tuple(x.shape[:-1])
            _, h8 = ops.layernorm_q8(x, None, bk["n1g"], bk["n1b"], 1e-5, kp=bk["qkv_w8"].kp, want_y=False)
            qkv = ops.linear_mxfp8(h8, bk["qkv_w8"], bk["qkv_b"], lead=lead)
            # the attention core writes the proj operand (no bf16 rows, no quantise pass)
            a8 = ops.swin_window_attention_q8(qkv, bk["bias"], H, heads, ws, bk["shift"], kp=bk["proj_w8"].kp)
            return ops.linear_mxfp8(a8, bk["proj_w8"], bk["proj_b"], x, lead=lead)
        h = ops.layernorm(x, bk["n1g"], bk["n1b"], 1e-5)
        qkv = (ops.linear_rw(h, bk["qkv_rw"], bk["qkv_b"]) if bk["qkv_rw"] is not None
               else _lin(h, bk["qkv_w"], bk["qkv_b"], w8=bk["qkv_w8"]))
        a = ops.swin_window_attention(qkv, bk["bias"], H, heads, ws, bk["shift"])
        if bk["proj_rw"] is not None:
            return ops.linear_rw(a, bk["proj_rw"], bk["proj_b"], residual=x)
        return _lin(a, bk["proj_w"], bk["proj_b"], residual=x, w8=bk["proj_w8"])

    def _mlp_half(self, x, bk):
        """x + fc2(GELU(fc1(norm2(x)))) of one block: one kernel where the block holds mlp_pack, else the fp8
        pair with fc1 emitting fc2's operand (the LayerNorm emitting fc1's where it can), else two GEMMs."""
        if bk["mlp_pack"] is not None:
            return ops.swin_mlp(x, bk["n2g"], bk["n2b"], bk["mlp_pack"], bk["fc1_b"], bk["fc2_b"], 1e-5)
        w8 = bk["fc1_w8"]
        if _ln8_ok(x, w8) and w8.layout == 2:
            _, h8 = ops.layernorm_q8(x, None, bk["n2g"], bk["n2b"], 1e-5, kp=w8.kp, want_y=False)
            return _mlp8(x, w8, bk["fc1_b"], bk["fc2_w8"], bk["fc2_b"], residual=x, h8=h8)
        h = ops.layernorm(x, bk["n2g"], bk["n2b"], 1e-5)
        if w8 is not None and w8.layout == 2:
            return _mlp8(h, w8, bk["fc1_b"], bk["fc2_w8"], bk["fc2_b"], residual=x)
        h = _lin(h, bk["fc1_w"], bk["fc1_b"], act=1, w8=w8)
        return _lin(h, bk["fc2_w"], bk["fc2_b"], residual=x, w8=bk["fc2_w8"])

    def forward_features(self, image):
        """timm forward_features: (B, h, w, C) NHWC after the final norm (bf16)."""
        x = self.tokens(image)
        return ops.layernorm(x, self.norm_g, self.norm_b, 1e-5)

    def head(self, tok, want_patches=True):
        """Backbones.forward image branch (fusion.py:259-265) from pre-norm tokens (B, h, w, C), one fused
        pass: (img_global, img_patches or None, pool) f32 — pool = mean over [global; patches]."""
        B, H, W, C = tok.shape
        patches, glob, pool = ops.swin_head(tok.view(B, H * W, C), self.norm_g, self.norm_b, 1e-5,
                                            want_patches=want_patches)
        return glob, patches, pool


def _ln_fold(w, b, gamma, beta):
    """A linear that consumes LayerNorm(y) rewritten on the raw y (ops.linear_ln ln_mode 1):
    LN(y) W^T + b = rstd (y W'^T) - rstd mean c + d with W' = bf16(W diag(gamma)), c = row sums of W'
    (as stored), d = W beta + b.  w bf16 [N, K]; b, gamma, beta f32."""
    wf = (w.double() * gamma.double()[None, :]).to(torch.bfloat16).contiguous()
    c = wf.double().sum(1).float().contiguous()
    d = (w.double() @ beta.double() + b.double()).float().contiguous()
    return wf, c, d


class BertTower:
    """HF BertModel(input_ids, attention_mask).last_hidden_state semantics (eval).  fp8: the four
    linears of every layer run as MX-fp8 GEMMs (config 5; B * L must be a multiple of 256)."""

    def __init__(self, sd, cfg=BERT_BASE, device="cuda", fp8=False):
        self.cfg = dict(BERT_BASE, **cfg)
        self.fp8 = fp8
        dev = torch.device(device)
        self.device = dev
        self.word = _f(sd["embeddings.word_embeddings.weight"], dev)
        self.pos = _f(sd["embeddings.position_embeddings.weight"], dev)
        self.type0 = _f(sd["embeddings.token_type_embeddings.weight"][0], dev)
        self.eg, self.eb = _f(sd["embeddings.LayerNorm.weight"], dev), _f(sd["embeddings.LayerNorm.bias"], dev)
        self.layers = load_bert_layers(sd, self.cfg, dev, _bf)
        for ly in self.layers:
            for n in ("qkv", "o", "i", "f"):
                ly[n + "_w8"] = _w8(ly[n + "_w"], plain=True) if fp8 else None
        self.hidden = self.word.shape[1]
        # bf16 towers: every LayerNorm but the embedding's and the last is folded into the GEMMs around
        # it (ops.linear_ln): FFN1 and the next layer's QKV read the raw residual stream with W' =
        # W diag(gamma), c = row sums of W', d = W beta + b; O-proj / FFN2 normalise their raw residual
        # in the epilogue and emit the row statistics the next consumer needs
        self.ln_fold = not fp8 and self.hidden % 192 == 0
        if self.ln_fold:
            for i, ly in enumerate(self.layers):
                ly["i_wf"], ly["i_c"], ly["i_d"] = _ln_fold(ly["i_w"], ly["i_b"], ly["ln1_g"], ly["ln1_b"])
                if i > 0:
                    prev = self.layers[i - 1]
                    ly["qkv_wf"], ly["qkv_c"], ly["qkv_d"] = _ln_fold(ly["qkv_w"], ly["qkv_b"], prev["ln2_g"],
                                                                      prev["ln2_b"])
        # optional dict name -> list of (start, end) torch.cuda.Event pairs around every launch of the
        # four GEMMs of a layer ("qkv", "o", "ffn1", "ffn2"): the bench's per-kernel roofline (events
        # ride torch's current stream = the launch stream)
        self.gemm_events = None

    def forward(self, input_ids, attention_mask=None):
        """(B, L) ids/mask -> (B, L, C) bf16 last_hidden_state.  L is truncated to
        max_position_embeddings like fusion.py:315-320.  Picks the layer stack: LayerNorm-folded bf16
        (_forward_folded), the fp8 fast path (_forward_fp8), else _forward_plain."""
        ids, mask = _text_inputs(input_ids, attention_mask, self.device, self.cfg["max_position_embeddings"])
        rows, C = ids.numel(), self.hidden
        if self.ln_fold and rows % 256 == 0 and ops.linear_ln_parts(rows, C, 2) > 0:
            return self._forward_folded(ids, mask)
        if (self.fp8 and C % 256 == 0 and C <= 1024 and rows % 256 == 0
                and all(ly["qkv_w8"].kp == C and ly["i_w8"].layout == 2 for ly in self.layers)):
            return self._forward_fp8(ids, mask)
        return self._forward_plain(ids, mask)

    def _forward_folded(self, ids, mask):
        """The bf16 layer stack with the LayerNorms folded into the GEMMs (see __init__): per layer
        QKV (fold LN2 of the previous layer) -> attention -> O-proj (+ LN2(previous raw output),
        statistics) -> FFN1 (fold LN1, GELU) -> FFN2 (+ LN1(raw O-proj output), statistics); one
        LayerNorm at the end materialises last_hidden_state.  Same maths as _forward_plain:
        HF BertLayer (reference fusion.py:322-325), the normalised rows just never round-trip HBM."""
        heads = self.cfg["num_attention_heads"]
        C, eps = self.hidden, 1e-12
        ev, gemm_ln = self.gemm_events, ops.linear_ln
        h0 = ops.bert_embed(ids, self.word, self.pos, self.type0, self.eg, self.eb, eps)
        y2 = cf2 = None
        for i, ly in enumerate(self.layers):
            if i == 0:
                qkv = _timed(ev, "qkv", _lin, h0, ly["qkv_w"], ly["qkv_b"])
            else:
                qkv, _ = _timed(ev, "qkv", gemm_ln, y2, ly["qkv_wf"], ly["qkv_d"], ln_mode=1, coef=cf2, v1=ly["qkv_c"])
            ctx = ops.bert_attention(qkv, mask, heads, C // heads)
            if i == 0:
                y1, st1 = _timed(ev, "o", gemm_ln, ctx, ly["o_w"], ly["o_b"], residual=h0, want_stats=True)
            else:
                prev = self.layers[i - 1]
                y1, st1 = _timed(ev, "o", gemm_ln, ctx, ly["o_w"], ly["o_b"], residual=y2, ln_mode=2, coef=cf2,
                                  v1=prev["ln2_g"], v2=prev["ln2_b"], want_stats=True)
            cf1 = ops.ln_row_coef(st1, C, eps)
            f1, _ = _timed(ev, "ffn1", gemm_ln, y1, ly["i_wf"], ly["i_d"], act=1, ln_mode=1, coef=cf1, v1=ly["i_c"])
            y2, st2 = _timed(ev, "ffn2", gemm_ln, f1, ly["f_w"], ly["f_b"], residual=y1, ln_mode=2, coef=cf1,
                             v1=ly["ln1_g"], v2=ly["ln1_b"], want_stats=True)
            cf2 = ops.ln_row_coef(st2, C, eps)
        last = self.layers[-1]
        return ops.layernorm(y2, last["ln2_g"], last["ln2_b"], eps)

    def _forward_fp8(self, ids, mask):
        """The fp8 fast path (rows a multiple of 256): every LayerNorm also emits the next GEMM's MX-fp8
        operand (the embedding LayerNorm the first QKV's), the attention O-proj's, FFN1 FFN2's.
        gemm_events, when set, wrap the very launches the untimed forward makes."""
        heads, ev = self.cfg["num_attention_heads"], self.gemm_events
        dh = self.hidden // heads
        h, h8 = ops.bert_embed_q8(ids, self.word, self.pos, self.type0, self.eg, self.eb, 1e-12)
        lead = tuple(h.shape[:-1])
        for ly in self.layers:
            qkv = _timed(ev, "qkv", ops.linear_mxfp8, h8, ly["qkv_w8"], ly["qkv_b"], lead=lead)
            if dh % 32 == 0 and ly["o_w8"].kp == self.hidden:  # the attention emits O-proj's operand
                _, c8 = ops.bert_attention(qkv, mask, heads, dh, q8=True, bf16=False)
                a = _timed(ev, "o", ops.linear_mxfp8, c8, ly["o_w8"], ly["o_b"], lead=lead)
            else:
                ctx = ops.bert_attention(qkv, mask, heads, dh)
                a = _timed(ev, "o", _lin, ctx, ly["o_w"], ly["o_b"], w8=ly["o_w8"])
            h, h8 = ops.layernorm_q8(a, h, ly["ln1_g"], ly["ln1_b"], 1e-12)
            f = _mlp8(h, ly["i_w8"], ly["i_b"], ly["f_w8"], ly["f_b"], h8=h8, ev=ev)
            h, h8 = ops.layernorm_q8(f, h, ly["ln2_g"], ly["ln2_b"], 1e-12)
        return h

    def _forward_plain(self, ids, mask):
        """HF BertLayer as written: GEMMs (bf16, or MX-fp8 on zero-padded rows where the layer holds w8) with
        the post-LN residual adds in the LayerNorm kernel."""
        heads, ev = self.cfg["num_attention_heads"], self.gemm_events
        # a set gemm_events selects FFN1 / FFN2 as two separately quantised GEMMs here on purpose (bench.py's
        # per-GEMM roofline reads that chain); only the untimed forward takes the _mlp8 pair
        pair8 = ev is None
        h = ops.bert_embed(ids, self.word, self.pos, self.type0, self.eg, self.eb, 1e-12)
        for ly in self.layers:
            qkv = _timed(ev, "qkv", _lin, h, ly["qkv_w"], ly["qkv_b"], w8=ly["qkv_w8"])
            ctx = ops.bert_attention(qkv, mask, heads, self.hidden // heads)
            a = _timed(ev, "o", _lin, ctx, ly["o_w"], ly["o_b"], w8=ly["o_w8"])
            h = ops.add_layernorm(a, h, ly["ln1_g"], ly["ln1_b"], 1e-12)
            if pair8 and ly["i_w8"] is not None and ly["i_w8"].layout == 2:
                f = _mlp8(h, ly["i_w8"], ly["i_b"], ly["f_w8"], ly["f_b"])  # FFN1 emits FFN2's fp8 operand
            else:
                f = _timed(ev, "ffn1", _lin, h, ly["i_w"], ly["i_b"], act=1, w8=ly["i_w8"])
                f = _timed(ev, "ffn2", _lin, f, ly["f_w"], ly["f_b"], w8=ly["f_w8"])
            h = ops.add_layernorm(f, h, ly["ln2_g"], ly["ln2_b"], 1e-12)
        return h


# ---------------------------------------------------------------- synthetic weights (bench)
def init_swin_state(cfg=SWIN_T, seed=2709):
    """Random-init Swin state dict in timm naming (trunc-normal(0.02) linears, LN (1, 0))."""
    cfg = dict(SWIN_T, **cfg)
    g = torch.Generator().manual_seed(seed)

    def rn(*shape):
        return (torch.randn(*shape, generator=g) * 0.02).clamp_(-0.04, 0.04)
    E = cfg["embed_dim"]
    ws = cfg["window_size"]
    sd = {"patch_embed.proj.weight": rn(E, cfg["in_chans"], cfg["patch"], cfg["patch"]),
          "patch_embed.proj.bias": torch.zeros(E), "patch_embed.norm.weight": torch.ones(E),
          "patch_embed.norm.bias": torch.zeros(E)}
    C = E
    for i, depth in enumerate(cfg["depths"]):
        if i > 0:
            p = f"layers.{i}.downsample."
            sd[p + "norm.weight"], sd[p + "norm.bias"] = torch.ones(4 * C), torch.zeros(4 * C)
            sd[p + "reduction.weight"] = rn(2 * C, 4 * C)
            C *= 2
        for j in range(depth):
            p = f"layers.{i}.blocks.{j}."
            sd.update({p + "norm1.weight": torch.ones(C), p + "norm1.bias": torch.zeros(C),
                       p + "attn.qkv.weight": rn(3 * C, C), p + "attn.qkv.bias": rn(3 * C),
                       p + "attn.relative_position_bias_table": rn((2 * ws - 1) ** 2, cfg["num_heads"][i]),
                       p + "attn.proj.weight": rn(C, C), p + "attn.proj.bias": rn(C),
                       p + "norm2.weight": torch.ones(C), p + "norm2.bias": torch.zeros(C),
                       p + "mlp.fc1.weight": rn(4 * C, C), p + "mlp.fc1.bias": rn(4 * C),
                       p + "mlp.fc2.weight": rn(C, 4 * C), p + "mlp.fc2.bias": rn(C)})
    sd["norm.weight"], sd["norm.bias"] = torch.ones(C), torch.zeros(C)
    return sd


def init_bert_state(cfg=BERT_BASE, seed=2710):
    cfg = dict(BERT_BASE, **cfg)
    g = torch.Generator().manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g) * 0.02
    C, I = cfg["hidden_size"], cfg["intermediate_size"]
    sd = {"embeddings.word_embeddings.weight": rn(cfg["vocab_size"], C),
          "embeddings.position_embeddings.weight": rn(cfg["max_position_embeddings"], C),
          "embeddings.token_type_embeddings.weight": rn(cfg["type_vocab_size"], C),
          "embeddings.LayerNorm.weight": torch.ones(C), "embeddings.LayerNorm.bias": torch.zeros(C)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            sd[p + f"attention.self.{n}.weight"] = rn(C, C)
            sd[p + f"attention.self.{n}.bias"] = rn(C)
        sd.update({p + "attention.output.dense.weight": rn(C, C), p + "attention.output.dense.bias": rn(C),
                   p + "attention.output.LayerNorm.weight": torch.ones(C),
                   p + "attention.output.LayerNorm.bias": torch.zeros(C),
                   p + "intermediate.dense.weight": rn(I, C), p + "intermediate.dense.bias": rn(I),
                   p + "output.dense.weight": rn(C, I), p + "output.dense.bias": rn(C),
                   p + "output.LayerNorm.weight": torch.ones(C), p + "output.LayerNorm.bias": torch.zeros(C)})
    return sd
