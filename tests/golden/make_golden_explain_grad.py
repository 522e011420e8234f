"""Gradient-explanation fixture: the REFERENCE's own compute_gradcam_map_for_target and compute_ig_map_for_target
(src/Model/explain.py:170-427, multimodal form) on its CrossModalFusion and classifier, loaded with the last fusion
layer and classifier weights of towers_mini.npz and run on that fixture's recorded features (sample 0).  Run by hand
in the build container like make_golden.py (whose stub loader it imports); never run by the test suite, bench.py or
smoke().  Writes tests/golden/explain_grad_mini.npz — arrays only.

Captum is not installed in the build container.  The reference imports `IntegratedGradients` from captum.attr; this
generator puts its own small stand-in under that name: zero-baseline-or-given-baseline Integrated Gradients with
Captum's default "gausslegendre" rule (alphas (1 + x) / 2, step sizes omega / 2 for numpy.polynomial.legendre
.leggauss(n_steps)), the scaled inputs run through the forward function internal_batch_size at a time, `target`
indexing the output's columns, attributions = (sum_s w_s grad_s) * (inputs - baselines).  The IG record therefore pins the reference's
forward function (_forward_patches_batchfirst: img_global = mean of the patches, the classifier on every token,
logits[:, t] indexed again by target=t) and its reductions (L1 over channels, min-max, clamp, bilinear) — it does not
pin Captum.

Records (f32, as the reference returns them): "gradcam_tokens" (5,) = 0, 1, 25, 49, 50 and "gradcam_maps" (5, 28,
28); "ig_tokens" (3,) = 0, 1, 25 and "ig_maps" (3, 28, 28) at the method's default steps = 50 ("ig_steps");
"image_size"; "description"."""
import contextlib
import importlib
import io
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import make_golden as mg  # noqa: E402
from attn_maps_ref import towers_mini  # noqa: E402

OUT = mg.OUT
SIZE = (28, 28)
GRADCAM_TOKENS = (0, 1, 25, 49, 50)
IG_TOKENS = (0, 1, 25)


class GaussLegendreIG:
    """the stand-in registered as captum.attr.IntegratedGradients (see the module docstring)"""

    def __init__(self, forward_func):
        self.forward_func = forward_func

    def attribute(self, inputs, baselines=None, n_steps=50, internal_batch_size=None, target=None):
        import torch
        baselines = torch.zeros_like(inputs) if baselines is None else baselines
        x, w = np.polynomial.legendre.leggauss(int(n_steps))
        alphas = torch.tensor(0.5 * (1.0 + x), dtype=inputs.dtype)
        steps = torch.tensor(0.5 * w, dtype=inputs.dtype)
        assert inputs.shape[0] == 1
        shape = (-1,) + (1,) * (inputs.dim() - 1)
        scaled = (baselines + alphas.view(shape) * (inputs - baselines)).detach()
        # internal_batch_size scaled inputs per forward call (the reference passes 1: its forward function closes
        # over a batch-1 txt_feats), as Captum's _batch_attribution does
        chunk = int(internal_batch_size or n_steps)
        grads = []
        for i in range(0, int(n_steps), chunk):
            part = scaled[i:i + chunk].clone().requires_grad_(True)
            out = self.forward_func(part)
            grads.append(torch.autograd.grad(out[:, int(target)].sum(), part)[0])
        total = (torch.cat(grads) * steps.view(shape)).sum(0, keepdim=True)
        return total * (inputs - baselines)


def main():
    import torch
    mg.install_stubs()
    sys.modules["captum.attr"].IntegratedGradients = GaussLegendreIG
    mg._pkg("Model", mg.REF / "Model")
    fusion = importlib.import_module("Model.fusion")
    explain = importlib.import_module("Model.explain")
    assert explain.IntegratedGradients is GaussLegendreIG
    f, w = towers_mini()
    hsd = w["head"]
    nl = 1 + max(int(k.split(".")[1]) for k in hsd if k.startswith("fusion_layers."))
    p = f"fusion_layers.{nl - 1}."
    D, heads = int(hsd["img_proj.weight"].shape[0]), 4
    G, P, T = (torch.from_numpy(np.asarray(f[k], np.float32)) for k in ("img_global", "img_patches", "txt_feats"))
    layer = fusion.CrossModalFusion(P.shape[2], T.shape[2], joint_dim=D, num_heads=heads)
    layer.load_state_dict({k[len(p):]: v for k, v in hsd.items() if k.startswith(p)})
    C = int(hsd["classifier.3.weight"].shape[0])
    cls = torch.nn.Sequential(torch.nn.Linear(D, 4 * D), torch.nn.GELU(), torch.nn.Dropout(0.1),
                              torch.nn.Linear(4 * D, C), torch.nn.Dropout(0.1))   # model.py:271-277
    cls.load_state_dict({k[len("classifier."):]: v for k, v in hsd.items() if k.startswith("classifier.")})
    layer.eval(), cls.eval()
    eng = explain.ExplanationEngine(layer, cls, image_size=SIZE)
    g, pt, tt = G[:1], P[:1], T[:1]
    rec = {"image_size": np.asarray(SIZE, np.int32), "gradcam_tokens": np.asarray(GRADCAM_TOKENS, np.int32),
           "ig_tokens": np.asarray(IG_TOKENS, np.int32), "ig_steps": np.asarray(50, np.int32)}
    with contextlib.redirect_stdout(io.StringIO()):
        rec["gradcam_maps"] = np.stack([np.asarray(eng.compute_gradcam_map_for_target(g, pt.clone(), tt, t), np.float32)
                                        for t in GRADCAM_TOKENS])
        rec["ig_maps"] = np.stack([np.asarray(eng.compute_ig_map_for_target(g, pt, tt, target_idx=t), np.float32)
                                   for t in IG_TOKENS])
    assert rec["gradcam_maps"].shape == (5,) + SIZE and rec["ig_maps"].shape == (3,) + SIZE
    rec["description"] = np.frombuffer(
        b"reference compute_gradcam_map_for_target / compute_ig_map_for_target on towers_mini sample 0, last fusion "
        b"layer + classifier; IntegratedGradients is the generator's Gauss-Legendre stand-in, not Captum", np.uint8)
    np.savez_compressed(OUT / "explain_grad_mini.npz", **rec)
    size = (OUT / "explain_grad_mini.npz").stat().st_size
    assert size < 1 << 20, size
    print("wrote explain_grad_mini.npz", size, "bytes")


if __name__ == "__main__":
    main()
