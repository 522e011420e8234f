"""CPU: the attention-map fixture (tests/golden/attn_mini.npz, written by make_attn_golden.py from the
reference's forward(..., return_attention=True)) against the plain-torch restatement the GPU tests compare
with, and the argument checks of mmr_mha_probs / mmr_x3_attention_probs (no GPU needed: they reject before
touching the device)."""
import ctypes
import json
import os

import numpy as np
import torch

import __graft_entry__ as ge  # noqa: F401  (puts the repository root on sys.path)
from attn_maps_ref import KINDS, attention_maps, max_abs, towers_mini

from conftest import GOLDEN


def test_fixture_matches_restatement():
    """f32 restatement on towers_mini.npz's stored features and head weights == every map of attn_mini.npz
    to 1e-5 absolute (the project's bound for exact-f32 paths; probabilities are <= 1), with and without
    text.  The restatement's own f32-vs-f64 distance is printed: the yardstick for how close an
    fp32-faithful GPU path can be expected to come to the fixture."""
    f, w = towers_mini()
    gold = np.load(os.path.join(GOLDEN, "attn_mini.npz"), allow_pickle=False)
    cfg = json.loads(bytes(f["cfg"]).decode())
    G, P, T = (torch.from_numpy(f[k]) for k in ("img_global", "img_patches", "txt_feats"))
    head64 = {k: v.double() for k, v in w["head"].items()}
    rep = {}
    with torch.no_grad():
        for tag, t in (("text", T), ("notext", None)):
            m32 = attention_maps(G, P, t, w["head"], cfg["num_heads"])
            m64 = attention_maps(G.double(), P.double(), None if t is None else t.double(), head64, cfg["num_heads"])
            assert sorted(m32) == sorted(f"layer_{i}_{k}" for i in range(cfg["num_fusion_layers"]) for k in KINDS)
            for k, v in m32.items():
                ref = torch.from_numpy(gold[f"{tag}_{k}"])
                assert v.shape == ref.shape and v.dtype == torch.float32, k
                rep[f"{tag}_{k}"] = {"vs_fixture": max_abs(v, ref), "f32_vs_f64": max_abs(v, m64[k]),
                                     "max_ref": ref.abs().max().item()}
    print(json.dumps(rep))
    assert max(r["vs_fixture"] for r in rep.values()) <= 1e-5, rep
    # default text token: img2txt has ONE key, its softmax is exactly 1; txt2img is one query row over the
    # Np patch keys (a distribution, not ones)
    for i in range(cfg["num_fusion_layers"]):
        assert np.array_equal(gold[f"notext_layer_{i}_img2txt"], np.ones((2, 49, 1), np.float32))
        assert gold[f"notext_layer_{i}_txt2img"].shape == (2, 1, 49)


def test_probs_argument_checks():
    from mmr_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)  # non-NULL, 16-B aligned, never dereferenced: every call below is rejected first
    for fn, name in ((L.mmr_mha_probs, b"mmr_mha_probs"), (L.mmr_x3_attention_probs, b"mmr_x3_attention_probs")):
        assert fn(None, 768, p, 768, p, 49, 2, 128, 49, 8, 96, 0.1, None) == 1
        assert b"NULL" in L.mmr_last_error() and name in L.mmr_last_error()
        assert fn(p, 768, None, 768, p, 49, 2, 128, 49, 8, 96, 0.1, None) == 1
        assert fn(p, 768, p, 768, None, 49, 2, 128, 49, 8, 96, 0.1, None) == 1
        assert fn(p, 768, p, 768, p, 49, 2, 128, 49, 8, 60, 0.1, None) == 1      # head_dim % 8
        assert b"head_dim 60" in L.mmr_last_error()
        assert fn(p, 768, p, 768, p, 48, 2, 128, 49, 8, 96, 0.1, None) == 1      # ldp < lk
        assert b"ldp=48" in L.mmr_last_error()
        assert fn(p, 768, p, 768, p, 49, 2, 0, 49, 8, 96, 0.1, None) == 1        # lq = 0
        assert fn(p, 768, p, 760, p, 49, 2, 128, 49, 8, 96, 0.1, None) == 1      # ldk < heads*dh
        assert fn(p, 770, p, 768, p, 49, 2, 128, 49, 8, 96, 0.1, None) == 1      # ldq off the 16-B grid
        assert fn(ctypes.c_void_p(68), 768, p, 768, p, 49, 2, 128, 49, 8, 96, 0.1, None) == 1  # q misaligned
        # the per-head softmax statistics live in LDS: more heads than fit is unsupported, not invalid
        assert fn(p, 2048, p, 2048, p, 49, 2, 128, 49, 224, 8, 0.1, None) == 4
        assert b"heads=224" in L.mmr_last_error()
        assert fn(p, 768, p, 768, p, 49, 0, 128, 49, 8, 96, 0.1, None) == 0      # b = 0: MMR_OK, no launch
    assert L.mmr_x3_attention_probs(p, 1280, p, 1280, p, 49, 2, 128, 49, 8, 160, 0.1, None) == 1  # x3: dh <= 128
    assert b"head_dim 160" in L.mmr_last_error()
    assert L.mmr_mha_probs(p, 1600, p, 1600, p, 49, 2, 128, 49, 8, 200, 0.1, None) == 1           # bf16: dh <= 192
