"""Classifier / predict() fixture: the REFERENCE model's forward(...)["logits"] and predict() on the mini
geometry of towers_mini.npz, run by hand in the build container like make_attn_golden.py (whose stub loader
it shares through make_golden.py; it is never run by the test suite, bench.py or smoke()).  Writes
tests/golden/predict_mini.npz — arrays only.

For each model_type ("text", "image", "multimodal") the reference's MultiModalRetrievalModel(joint_dim=64,
num_heads=4, num_classes=43, num_fusion_layers=2, model_type=mt) is built as make_golden.gen_towers builds
it, every non-backbone weight is loaded from towers_mini.npz ("w:head.*", bf16 bit patterns: the classifier
is w:head.classifier.0.* / .3.*, 64 -> 256 -> 43) and its backbones are replaced by a stub that returns the
stored img_global / img_patches / txt_feats.  Its joint_emb must reproduce towers_mini.npz's {mt}_joint_emb
(asserted before anything is written).

Stored per model_type: {mt}_logits (2, 43) f32; predict()'s outputs at (threshold 0.5, K 5) as
{mt}_t50_k5_{probs,preds,topk_idx,topk_vals} and at (threshold 0.3, K 43) as {mt}_t30_k43_*: probs f32
(2, 43), preds int32 (2, 43), topk_idx int64 (2, K), topk_vals f32 (2, K)."""
import importlib
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden as mg  # noqa: E402

OUT = mg.OUT
SETTINGS = (("t50_k5", 0.5, 5), ("t30_k43", 0.3, 43))


def reference_module():
    import torch
    from transformers import BertConfig, BertModel
    torch.manual_seed(mg.SEED)
    tmp = Path(tempfile.mkdtemp(prefix="mmr_predict_golden_"))
    bert_dir = tmp / "bert"
    BertModel(BertConfig(**mg.BERT_MINI, hidden_act="gelu", layer_norm_eps=1e-12)).save_pretrained(str(bert_dir))
    mg._pkg("Retrieval", mg.REF / "Retrieval")
    rr = types.ModuleType("Retrieval.reranker")
    rr.Reranker = None
    sys.modules["Retrieval.reranker"] = rr
    retr = mg._load_file("Retrieval.retrieval", mg.REF / "Retrieval" / "retrieval.py")
    sys.modules["Retrieval"].RetrievalEngine = retr.RetrievalEngine
    sys.modules["Retrieval"].make_retrieval_engine = retr.make_retrieval_engine
    mg._pkg("Model", mg.REF / "Model")
    mg._pkg("Model.explain", ExplanationEngine=None)
    importlib.import_module("Model.fusion")
    model_mod = importlib.import_module("Model.model")
    model_mod.EMBEDDINGS_DIR = tmp  # training=True writes dummy files (model.py:316-323)
    return model_mod, bert_dir


def main():
    import torch
    mg.install_stubs()
    f = np.load(OUT / "towers_mini.npz", allow_pickle=False)
    model_mod, bert_dir = reference_module()
    head = {k[len("w:head."):]: torch.from_numpy(mg.odata.bf16_bits_to_f32(f[k]).copy()) for k in f.files
            if k.startswith("w:head.")}
    assert head["classifier.0.weight"].shape == (256, 64) and head["classifier.3.weight"].shape == (43, 256)
    feats = tuple(torch.from_numpy(f[k]) for k in ("img_global", "img_patches", "txt_feats"))

    class StoredFeatures(torch.nn.Module):  # Backbones.forward's return value from the stored features
        def forward(self, image, input_ids=None, attention_mask=None):
            return (feats[0], feats[1]), (feats[2] if input_ids is not None else None)

    image = torch.zeros(2, 3, 224, 224)
    ids, mask = torch.from_numpy(f["input_ids"]), torch.from_numpy(f["attention_mask"])
    rec = {}
    for mt in ("text", "image", "multimodal"):
        m = model_mod.MultiModalRetrievalModel(
            joint_dim=64, num_heads=4, num_classes=43, num_fusion_layers=2, img_backbone="swin",
            swin_name="swin_mini", bert_name="bert_mini", bert_local_dir=str(bert_dir), pretrained=False,
            training=True, use_shared_ffn=False, use_cls_only=False, model_type=mt)
        res = m.load_state_dict(head, strict=False)
        assert not res.unexpected_keys, res.unexpected_keys
        assert all(k.startswith("backbones.") for k in res.missing_keys), res.missing_keys
        m.backbones = StoredFeatures()
        m.eval()
        with torch.no_grad():
            o = m(image, ids, mask)
            ref = f[f"{mt}_joint_emb"]
            err = np.abs(o["joint_emb"].numpy() - ref).max()
            assert err <= 1e-6 * np.abs(ref).max(), (mt, err, np.abs(ref).max())
            assert o["logits"].dtype == torch.float32 and tuple(o["logits"].shape) == (2, 43)
            rec[f"{mt}_logits"] = o["logits"].numpy()
            for tag, thr, k in SETTINGS:
                p = m.predict(image, ids, mask, threshold=thr, K=k)
                rec[f"{mt}_{tag}_probs"] = np.asarray(p["probs"], np.float32)
                rec[f"{mt}_{tag}_preds"] = np.asarray(p["preds"], np.int32)
                rec[f"{mt}_{tag}_topk_idx"] = np.asarray(p["topk_idx"], np.int64)
                rec[f"{mt}_{tag}_topk_vals"] = np.asarray(p["topk_vals"], np.float32)
        print(mt, "joint_emb max|err|", float(err))
    np.savez_compressed(OUT / "predict_mini.npz", **rec)
    print("wrote predict_mini.npz", {k: v.shape for k, v in rec.items()})


if __name__ == "__main__":
    main()
