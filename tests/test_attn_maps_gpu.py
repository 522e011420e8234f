"""GPU: the attention maps of return_attention=True (csrc/attn_probs.hip, FusionStack / MultiModalRetrievalModel).

Bars (written per test):
  * kernels vs f64 of the same inputs: max|err| <= 5e-5 * max|ref| — the bound test_x3_attention_vs_f64 holds
    the x3 core to; the bf16 entry's products of bf16 inputs are exact in f32, so it gets the same bound —
    every row sums to 1 within 1e-5, padding columns of the output rows untouched, two launches bitwise equal;
  * FusionStack / the whole model vs the f32 restatement (attn_maps_ref.py) and the reference's own maps
    (tests/golden/attn_mini.npz): x3 2e-4 * max|ref|, bf16 4e-2 * max|ref| — the bounds the project holds
    this chain's embeddings to (test_x3_mini_towers_match_reference_golden, test_fusion_gpu.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from attn_maps_ref import KINDS, attention_maps, max_abs, towers_mini
from mmr_amd import ops, synthetic
from mmr_amd.fusion import FusionStack
from mmr_amd.model import Backbones, MultiModalRetrievalModel, init_fusion_state, init_head_state
from mmr_amd.towers import BERT_BASE, SWIN_T

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"x3": 2e-4, "bf16": 4e-2}
SENTINEL = -7.5

CASES = [(2, 128, 49, 4, 16),    # the mini model's cross shape; dh below one MFMA K-step pair
         (2, 49, 128, 8, 96),    # the bench model's cross shape
         (2, 51, 51, 8, 96),     # comb; ragged in both dimensions
         (2, 1, 49, 8, 96),      # lq = 1
         (2, 49, 1, 8, 96),      # lk = 1: exactly 1.0
         (1, 33, 65, 1, 32),     # one head; crosses the 32- and 64-wide tile edges
         (2, 130, 70, 2, 48),    # several query tiles; dh not a multiple of 32
         (1, 40, 300, 3, 128),   # several key blocks
         (1, 33, 65, 1, 192)]    # bf16 only


@pytest.mark.parametrize("kind", ["bf16", "x3"])
@pytest.mark.parametrize("b,lq,lk,heads,dh", CASES)
def test_probs_kernel_vs_f64(kind, b, lq, lk, heads, dh):
    if kind == "x3" and dh > 128:
        with pytest.raises(Exception, match="head_dim 192"):  # the x3 entry takes dh <= 128
            z = torch.zeros(b * lq, heads * dh, device=DEV)
            ops.x3_attention_probs(z, z, b, lq, lq, heads, dh, 1.0)
        return
    g = torch.Generator().manual_seed(b * 1000 + lq + lk + dh)
    C = heads * dh
    q = torch.randn(b * lq, 3 * C, generator=g) * 0.7            # strided views of packed rows
    kv = torch.randn(b * lk, 3 * C, generator=g) * 0.7
    if kind == "bf16":
        q, kv = q.to(torch.bfloat16), kv.to(torch.bfloat16)
    scale = 1.0 / math.sqrt(dh)
    qh = q[:, :C].double().view(b, lq, heads, dh).transpose(1, 2)
    kh = kv[:, C:2 * C].double().view(b, lk, heads, dh).transpose(1, 2)
    ref = (qh @ kh.transpose(-1, -2) * scale).softmax(-1).mean(1)
    qd, kvd = q.to(DEV), kv.to(DEV)
    fn = ops.mha_probs if kind == "bf16" else ops.x3_attention_probs
    buf = torch.full((b, lq, lk + 4), SENTINEL, dtype=torch.float32, device=DEV)  # ldp = lk + 4
    fn(qd[:, :C], kvd[:, C:2 * C], b, lq, lk, heads, dh, scale, out=buf)
    buf2 = torch.full_like(buf, SENTINEL)
    fn(qd[:, :C], kvd[:, C:2 * C], b, lq, lk, heads, dh, scale, out=buf2)
    alloc = fn(qd[:, :C], kvd[:, C:2 * C], b, lq, lk, heads, dh, scale)            # allocates (b, lq, lk)
    torch.cuda.synchronize()
    got = buf[..., :lk].cpu()
    rep = {"rel": max_abs(got, ref) / ref.abs().max().item(), "rowsum": (got.double().sum(-1) - 1).abs().max().item()}
    print(json.dumps(rep))
    assert torch.equal(buf[..., lk:], torch.full_like(buf[..., lk:], SENTINEL)), "padding columns overwritten"
    assert rep["rel"] <= 5e-5
    assert rep["rowsum"] <= 1e-5
    assert torch.equal(buf, buf2)
    assert alloc.shape == (b, lq, lk) and alloc.dtype == torch.float32 and torch.equal(alloc.cpu(), got)
    if lk == 1:
        assert torch.equal(got, torch.ones_like(got))


FS_SHAPE = dict(B=3, Lt=128, Np=49, C=768, D=768, heads=8, layers=3)


@pytest.fixture(scope="module")
def fusion_case():
    """Fixed backbone features + head weights (test_fusion_stack_vs_oracle_on_backbone_features' setup) and the
    f32 restatement of the maps, with and without text; computed once, read-only."""
    s = FS_SHAPE
    g = torch.Generator().manual_seed(11)
    hs = init_head_state(s["C"], s["C"], s["D"], 21)
    hs.update(init_fusion_state(s["C"], s["C"], s["D"], s["heads"], s["layers"], 22))
    G = torch.randn(s["B"], s["C"], generator=g)
    P = torch.randn(s["B"], s["Np"], s["C"], generator=g)
    T = torch.randn(s["B"], s["Lt"], s["C"], generator=g).to(torch.bfloat16).float()
    with torch.no_grad():
        ref = {True: attention_maps(G, P, T, hs, s["heads"]), False: attention_maps(G, P, None, hs, s["heads"])}
    return hs, G, P, T, ref


def _expected_shapes(B, Lt, Np, layers):
    shp = {"comb": (B, Np + 2, Np + 2), "txt2img": (B, Lt, Np), "img2txt": (B, Np, Lt)}
    return {f"layer_{i}_{k}": shp[k] for i in range(layers) for k in KINDS}


@pytest.mark.parametrize("text", [True, False])
@pytest.mark.parametrize("tower_dtype", ["bf16", "x3"])
def test_fusion_stack_attention_maps(fusion_case, tower_dtype, text):
    """return_attention leaves the joint embedding bitwise unchanged and returns the 9 maps, each within the
    mode's bound of the f32 restatement; without text (default token, Lt = 1) img2txt has one key and is
    exactly 1 (txt2img is then one query row over the Np patch keys: a distribution, held to the same bound)."""
    hs, G, P, T, refs = fusion_case
    s = FS_SHAPE
    fs = FusionStack(hs, s["heads"], device=DEV, tower_dtype=tower_dtype)
    args = (G.to(DEV), P.to(DEV), T.to(DEV) if text else None)
    plain = fs.forward(*args).clone()
    joint, attn = fs.forward(*args, return_attention=True)
    again = fs.forward(*args).clone()
    torch.cuda.synchronize()
    assert torch.equal(joint, plain) and torch.equal(again, plain)
    want = _expected_shapes(s["B"], s["Lt"] if text else 1, s["Np"], s["layers"])
    assert list(attn) == list(want)  # the reference's key order
    errs = {}
    for k, v in attn.items():
        assert v.shape == want[k] and v.dtype == torch.float32 and v.is_cuda, k
        ref = refs[text][k]
        errs[k] = max_abs(v, ref) / ref.abs().max().item()
        assert (v.double().sum(-1) - 1).abs().max().item() <= 1e-5, k
    print(json.dumps({tower_dtype: errs}))
    assert max(errs.values()) <= TOL[tower_dtype], errs
    if not text:
        for i in range(s["layers"]):
            assert torch.equal(attn[f"layer_{i}_img2txt"], torch.ones_like(attn[f"layer_{i}_img2txt"]))


@pytest.mark.parametrize("tower_dtype", ["x3", "bf16"])
def test_model_attention_maps_match_reference_golden(tower_dtype):
    """The reference's own return_attention maps (attn_mini.npz, from its forward on the towers_mini.npz model)
    reproduced end to end — towers, fusion stack, maps — with text and with the default text token."""
    f, w = towers_mini()
    gold = np.load(os.path.join(GOLDEN, "attn_mini.npz"), allow_pickle=False)
    cfg = json.loads(bytes(f["cfg"]).decode())
    scfg = dict(SWIN_T, embed_dim=cfg["swin"]["embed_dim"], depths=cfg["swin"]["depths"],
                num_heads=cfg["swin"]["num_heads"])
    bb = Backbones(swin_state=w["swin"], bert_state=w["bert"], swin_cfg=scfg, bert_cfg=dict(BERT_BASE, **cfg["bert"]),
                   device=DEV, tower_dtype=tower_dtype)
    image = torch.from_numpy(synthetic.image_from_u8(f["img_u8"])).to(DEV)
    ids = torch.from_numpy(f["input_ids"]).to(DEV)
    mask = torch.from_numpy(f["attention_mask"]).to(DEV)
    m = MultiModalRetrievalModel(joint_dim=cfg["joint_dim"], num_heads=cfg["num_heads"], model_type="multimodal",
                                 backbones=bb, head_state=w["head"], device=DEV, use_shared_ffn=False)
    assert m(image, ids, mask)["attn"] is None
    errs = {}
    for tag, args in (("text", (image, ids, mask)), ("notext", (image, None, None))):
        o = m(*args, return_attention=True)
        names = [k[len(tag) + 1:] for k in gold.files if k.startswith(tag + "_layer_")]
        assert o["attn"]["layer_0_comb"] is not None and sorted(o["attn"]) == sorted(names)
        for k, v in o["attn"].items():
            ref = torch.from_numpy(gold[f"{tag}_{k}"])
            assert isinstance(v, torch.Tensor) and v.device.type == "cpu" and v.dtype == torch.float32, k
            assert v.shape == ref.shape, k
            errs[f"{tag}_{k}"] = max_abs(v, ref) / ref.abs().max().item()
    print(json.dumps({tower_dtype: errs}))
    assert max(errs.values()) <= TOL[tower_dtype], errs
    mt = MultiModalRetrievalModel(joint_dim=cfg["joint_dim"], num_heads=cfg["num_heads"], model_type="text",
                                  backbones=bb, head_state=w["head"], device=DEV, use_shared_ffn=False)
    assert mt(image, ids, mask, return_attention=True)["attn"] == {}
    assert mt(image, ids, mask)["attn"] is None
