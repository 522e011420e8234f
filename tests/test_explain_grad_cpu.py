"""CPU: the restatement of the gradient explanations (explain_grad_ref.py) against the reference's own recorded maps
(tests/golden/explain_grad_mini.npz), the fixture's conditions, and mutants of the restatement that the bound used
by the GPU tests has to reject.

Bound: deviation from the f64 restatement <= 8 x the deviation of the f32 restatement from it (absolute for maps in
[0, 1], relative to max-abs for gradients and raw vectors)."""
import functools
import os

import numpy as np
import pytest
import torch

import explain_grad_ref as gr
from attn_maps_ref import towers_mini

from conftest import GOLDEN

HEADS = 4


@functools.lru_cache(maxsize=None)
def fixture():
    f, w = towers_mini()
    G, P, T = (torch.from_numpy(np.asarray(f[k], np.float32)) for k in ("img_global", "img_patches", "txt_feats"))
    g = np.load(os.path.join(GOLDEN, "explain_grad_mini.npz"), allow_pickle=False)
    return G[0], P[0], T[0], w["head"], g, tuple(int(s) for s in g["image_size"])


@functools.lru_cache(maxsize=None)
def gradcam(token, dtype, mutant=None):
    G, P, T, hsd, _, size = fixture()
    return gr.gradcam(G, P, T, hsd, HEADS, token, size, dtype, mutant=mutant)


@functools.lru_cache(maxsize=None)
def ig(token, dtype, steps=50, mutant=None):
    G, P, T, hsd, _, size = fixture()
    return gr.integrated_gradients(P, T, hsd, HEADS, token, size, steps, dtype, mutant=mutant)


def test_golden_is_arrays_only():
    g = fixture()[4]
    assert sorted(g.files) == ["description", "gradcam_maps", "gradcam_tokens", "ig_maps", "ig_steps", "ig_tokens",
                               "image_size"]
    assert b"stand-in" in bytes(g["description"])
    assert os.path.getsize(os.path.join(GOLDEN, "explain_grad_mini.npz")) < 1 << 20


def test_gradcam_restatement_matches_the_reference():
    g = fixture()[4]
    for i, t in enumerate(int(t) for t in g["gradcam_tokens"]):
        r64, r32 = gradcam(t, torch.float64), gradcam(t, torch.float32)
        d32 = gr.abs_dev(r32["map"], r64["map"])
        d = gr.abs_dev(g["gradcam_maps"][i], r64["map"])
        print(f"gradcam t={t}: recorded {d:.3e} f32 restatement {d32:.3e}; raw f32 {gr.rel_dev(r32['raw'], r64['raw']):.3e}"
              f" grad f32 {gr.rel_dev(r32['grad'], r64['grad']):.3e}")
        assert d <= gr.BOUND_FACTOR * d32, (t, d, d32)
        # fixture conditions: the relu leaves a map that is neither empty nor full, the normalisation is well conditioned
        raw = r64["raw"]
        assert int((raw > 0).sum()) >= 8 and int((raw <= 0).sum()) >= 8, t
        assert gr.cond(gr.upsample(torch.relu(raw), fixture()[5])) <= 64


def test_ig_restatement_matches_the_reference():
    g = fixture()[4]
    steps = int(g["ig_steps"])
    for i, t in enumerate(int(t) for t in g["ig_tokens"]):
        r64, r32 = ig(t, torch.float64, steps), ig(t, torch.float32, steps)
        d32 = gr.abs_dev(r32["map"], r64["map"])
        d = gr.abs_dev(g["ig_maps"][i], r64["map"])
        print(f"ig t={t}: recorded {d:.3e} f32 restatement {d32:.3e}; raw f32 {gr.rel_dev(r32['raw'], r64['raw']):.3e}")
        assert d <= gr.BOUND_FACTOR * d32, (t, d, d32)
        assert gr.cond(r64["raw"]) <= 64


@pytest.mark.parametrize("mutant", gr.MUTANTS)
def test_mutants_are_rejected(mutant):
    """each wrong variant, computed in f64, misses the bound that the f32 restatement sets (token 0 for the IG global
    path: the global vector reaches x1 only)"""
    rejected = 0
    if mutant not in ("ig_global", "rectangle"):
        t = 25
        r64, r32, mu = gradcam(t, torch.float64), gradcam(t, torch.float32), gradcam(t, torch.float64, mutant)
        keys = ("map",) if mutant == "order" else ("grad", "raw", "map")
        for k in keys:
            dev = gr.abs_dev if k == "map" else gr.rel_dev
            d, d32 = dev(mu[k], r64[k]), dev(r32[k], r64[k])
            print(f"gradcam {mutant} {k}: mutant {d:.3e} bound {gr.BOUND_FACTOR * d32:.3e}")
            assert d > gr.BOUND_FACTOR * d32, (mutant, k)
            rejected += 1
    t = 0 if mutant == "ig_global" else 25
    r64, r32, mu = ig(t, torch.float64, 8), ig(t, torch.float32, 8), ig(t, torch.float64, 8, mutant)
    keys = ("map",) if mutant == "order" else ("grad", "raw", "map")
    for k in keys:
        dev = gr.abs_dev if k == "map" else gr.rel_dev
        d, d32 = dev(mu[k], r64[k]), dev(r32[k], r64[k])
        print(f"ig {mutant} {k}: mutant {d:.3e} bound {gr.BOUND_FACTOR * d32:.3e}")
        assert d > gr.BOUND_FACTOR * d32, (mutant, k)
        rejected += 1
    assert rejected
