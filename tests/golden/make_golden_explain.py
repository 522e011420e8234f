"""Explanation fixture: the REFERENCE's ExplanationEngine.explain (attention family) and compare_maps, run by hand
in the build container like make_golden.py (whose stub loader it imports; never run by the test suite, bench.py or
smoke()).  Writes tests/golden/explain_mini.npz — arrays only.

Explanation records.  ExplanationEngine(None, None, image_size).explain(None, patches, txt, maps, targets=[]) — with
no targets it never touches Captum — once per sample (the reference explains sample 0 of what it is given):
  text_{b} / notext_{b}    the last-layer maps of attn_mini.npz (T = 128 / the default token, T = 1), b = 0, 1, at
                           (28, 28); final_patch_map also at (224, 224) ("..._final224")
  syn_{Np}_{Lc}_{T}        synthetic maps, Np in {4, 9}, Lc in {Np, Np + 2, 30}, T in {1, 5, Lc, 128} (Lt = T), at
                           (8, 8): txt2img / img2txt row-stochastic, comb row-stochastic with its rows scaled by
                           distinct factors (a row-stochastic comb has all row sums 1: the reference's row-window
                           search would be decided by f32 rounding)
  per record "<name>:in_txt2img" ... the inputs (synthetic only; attn_mini's stay in attn_mini.npz) and
  "<name>:<key>" the reference's outputs; "<name>:keys" = the dictionary's key order, '|'-joined bytes, with a
  trailing '=None' where the value is None
Alignment records.  compare_maps (helper.py:173-209) at topk_frac 0.05 and 0.20 on pairs of "al_maps" (28 x 28:
the four recorded final_patch_maps, a constant map, a map of +-0 with plateau ties, a gaussian map and its
negation), once on the f32 arrays as run ("al_f32") and once on their exact f64 copies ("al_f64"): (P, 2, 3) =
pearson, spearman, iou per fraction; "al_pairs" (P, 2), a self-pair included.
Fixture conditions (asserted here and again by tests/test_explain_cpu.py through the restatement): the best and
second-best window sums differ by >= 1e-3; every normalised vector has max / (max - min) <= 64 (attn_mini's token
vector with text: 73.4, held to <= 128); every constant test is decided with f32 means on either side
(explain_ref.fixture_conditions)."""
import contextlib
import importlib
import io
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import make_golden as mg  # noqa: E402
import explain_ref as er  # noqa: E402

OUT = mg.OUT
KEYS = ("txt2img", "img2txt", "comb_img", "comb_txt", "final_patch_map", "final_token_map")


def reference():
    mg.install_stubs()
    mg._pkg("Model", mg.REF / "Model")
    ex = importlib.import_module("Model.explain")
    for name in ("matplotlib", "matplotlib.pyplot", "PIL", "PIL.Image", "sklearn", "sklearn.metrics"):
        try:
            importlib.import_module(name)
        except Exception:  # helper.py imports them at module level only
            mg._pkg(name, Image=None, roc_auc_score=None, average_precision_score=None)
    sys.modules["DataHandler"].parse_openi_xml = None
    helper = mg._load_file("Helpers.helper", mg.REF / "Helpers" / "helper.py")
    return ex.ExplanationEngine, helper.compare_maps


def synthetic_maps(npatch, lc, T, seed):
    import torch
    g = torch.Generator().manual_seed(seed)

    def sm(r, c):
        return torch.softmax(torch.randn(1, r, c, generator=g, dtype=torch.float64) * 3.0, -1)
    comb = sm(lc, lc) * (0.5 + torch.rand(1, lc, 1, generator=g, dtype=torch.float64))
    return sm(T, npatch).float(), sm(npatch, T).float(), comb.float()


def conditions(name, t2i, i2t, comb, T):
    # attn_mini with text: t_img is nearly uniform over the 128 tokens, the token vector's max / (max - min) is 73.4
    er.fixture_conditions(er.explain_sample(t2i, i2t, comb, T), name, row_search=not name.startswith("notext"),
                          token_cond=128.0 if name.startswith("text") else 64.0)


def record(Engine, rec, name, t2i, i2t, comb, T, size, store_inputs):
    import torch
    conditions(name, t2i[0].numpy(), i2t[0].numpy(), comb[0].numpy(), T)
    npatch = t2i.shape[2]
    eng = Engine(None, None, image_size=size)
    with contextlib.redirect_stdout(io.StringIO()):
        out = eng.explain(None, torch.zeros(1, npatch, 4), torch.zeros(1, T, 4),
                          {"txt2img": t2i, "img2txt": i2t, "comb": comb}, targets=[])
    am = out["attention_map"]
    assert out["ig_maps"] == {} and out["gradcam_maps"] == {}
    rec[f"{name}:keys"] = np.frombuffer("|".join(k + ("=None" if am[k] is None else "") for k in am).encode(), np.uint8)
    for k, v in am.items():
        if v is not None:
            rec[f"{name}:{k}"] = np.asarray(v, np.float32)
    if store_inputs:
        rec[f"{name}:in_txt2img"], rec[f"{name}:in_img2txt"], rec[f"{name}:in_comb"] = (x[0].numpy() for x in
                                                                                       (t2i, i2t, comb))
    return am


def main():
    import torch
    Engine, compare_maps = reference()
    attn = np.load(OUT / "attn_mini.npz", allow_pickle=False)
    rec, finals = {}, []
    for tag, T in (("text", 128), ("notext", 1)):
        for b in range(2):
            t2i, i2t, comb = (torch.from_numpy(attn[f"{tag}_layer_1_{k}"][b:b + 1]) for k in ("txt2img", "img2txt", "comb"))
            am = record(Engine, rec, f"{tag}_{b}", t2i, i2t, comb, T, (28, 28), False)
            finals.append(am["final_patch_map"])
            big = Engine(None, None, image_size=(224, 224))
            with contextlib.redirect_stdout(io.StringIO()):
                o = big.explain(None, torch.zeros(1, 49, 4), torch.zeros(1, T, 4),
                                {"txt2img": t2i, "img2txt": i2t, "comb": comb}, targets=[])
            if tag == "text":  # (224, 224) for two samples only
                rec[f"{tag}_{b}:final224"] = np.asarray(o["attention_map"]["final_patch_map"], np.float32)
    for npatch in (4, 9):
        for lc in (npatch, npatch + 2, 30):
            for T in sorted({1, 5, lc, 128}):
                t2i, i2t, comb = synthetic_maps(npatch, lc, T, 7000 + 100 * npatch + 10 * lc + T)
                record(Engine, rec, f"syn_{npatch}_{lc}_{T}", t2i, i2t, comb, T, (8, 8), True)
    # alignment
    g = np.random.default_rng(41)
    maps = [np.asarray(f, np.float32) for f in finals]
    maps.append(np.full((28, 28), 0.25, np.float32))
    z = np.where(g.random((28, 28)) < 0.5, 0.0, -0.0).astype(np.float32)
    z[::3, ::2] = 1.5
    z[1::4, 1::3] = -2.0
    maps.append(z)
    maps.append(g.standard_normal((28, 28)).astype(np.float32))
    maps.append(-maps[-1])
    maps = np.stack(maps)
    pairs = np.array([(0, 1), (0, 2), (1, 3), (2, 3), (0, 0), (0, 4), (5, 6), (5, 5), (6, 7), (6, 1), (4, 4), (5, 0)],
                     np.int64)
    res = {"al_f32": np.zeros((len(pairs), 2, 3)), "al_f64": np.zeros((len(pairs), 2, 3))}
    for p, (a, b) in enumerate(pairs):
        for j, frac in enumerate((0.05, 0.20)):
            for tag, cast in (("al_f32", np.float32), ("al_f64", np.float64)):
                with contextlib.redirect_stdout(io.StringIO()):
                    o = compare_maps(maps[a].astype(cast), maps[b].astype(cast), topk_frac=frac)
                assert list(o) == ["pearson", "spearman", er.iou_key(frac)]
                res[tag][p, j] = [o["pearson"], o["spearman"], o[er.iou_key(frac)]]
    rec.update(al_maps=maps.reshape(len(maps), -1), al_pairs=pairs, **res)
    np.savez_compressed(OUT / "explain_mini.npz", **rec)
    size = (OUT / "explain_mini.npz").stat().st_size
    assert size <= 600 * 1024, size
    print("wrote explain_mini.npz", len(rec), "arrays", size, "bytes")


if __name__ == "__main__":
    main()
