"""Attention-map fixture: the REFERENCE model's forward(..., return_attention=True) on the mini geometry of
towers_mini.npz, run by hand in the build container like make_golden.py (whose stub loader it imports; it
is never run by the test suite, bench.py or smoke()).  Writes tests/golden/attn_mini.npz — arrays only.

The reference's MultiModalRetrievalModel(model_type="multimodal", joint_dim=64, num_heads=4,
num_fusion_layers=2) is built as make_golden.gen_towers builds it, every non-backbone weight is loaded
from towers_mini.npz ("w:head.*", bf16 bit patterns) and its backbones are replaced by a stub that returns
the stored img_global / img_patches / txt_feats — so the run needs neither the towers' weights nor their
third-party stand-ins, and its joint_emb must reproduce towers_mini.npz's multimodal_joint_emb (asserted
before anything is written: the weights and features are wired as in the original run).

Stored: text_layer_{i}_{comb,txt2img,img2txt} (2,51,51) / (2,128,49) / (2,49,128) and text_joint_emb from
the run on txt_feats; notext_* from a run with input_ids = None (the learnable default text token, Lt = 1:
(2,1,49) / (2,49,1))."""
import importlib
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden as mg  # noqa: E402

OUT = mg.OUT


def reference_model():
    import torch
    from transformers import BertConfig, BertModel
    torch.manual_seed(mg.SEED)
    tmp = Path(tempfile.mkdtemp(prefix="mmr_attn_golden_"))
    bert_dir = tmp / "bert"
    BertModel(BertConfig(**mg.BERT_MINI, hidden_act="gelu", layer_norm_eps=1e-12)).save_pretrained(str(bert_dir))
    # the package stubs of make_golden.gen_towers (Model / Retrieval without their heavy __init__)
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
    m = model_mod.MultiModalRetrievalModel(
        joint_dim=64, num_heads=4, num_classes=43, num_fusion_layers=2, img_backbone="swin", swin_name="swin_mini",
        bert_name="bert_mini", bert_local_dir=str(bert_dir), pretrained=False, training=True, use_shared_ffn=False,
        use_cls_only=False, model_type="multimodal")
    return m


def main():
    import torch
    mg.install_stubs()
    f = np.load(OUT / "towers_mini.npz", allow_pickle=False)
    m = reference_model()
    head = {k[len("w:head."):]: torch.from_numpy(mg.odata.bf16_bits_to_f32(f[k]).copy()) for k in f.files
            if k.startswith("w:head.")}
    res = m.load_state_dict(head, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.startswith("backbones.") for k in res.missing_keys), res.missing_keys
    feats = tuple(torch.from_numpy(f[k]) for k in ("img_global", "img_patches", "txt_feats"))

    class StoredFeatures(torch.nn.Module):  # Backbones.forward's return value from the stored features
        def forward(self, image, input_ids=None, attention_mask=None):
            return (feats[0], feats[1]), (feats[2] if input_ids is not None else None)

    m.backbones = StoredFeatures()
    m.eval()
    image = torch.zeros(2, 3, 224, 224)
    ids, mask = torch.from_numpy(f["input_ids"]), torch.from_numpy(f["attention_mask"])
    rec = {}
    with torch.no_grad():
        for tag, args in (("text", (image, ids, mask)), ("notext", (image, None, None))):
            o = m(*args, return_attention=True)
            rec[f"{tag}_joint_emb"] = o["joint_emb"].numpy()
            assert sorted(o["attn"]) == sorted(f"layer_{i}_{k}" for i in range(2) for k in ("comb", "txt2img", "img2txt"))
            for k, v in o["attn"].items():
                assert v.dtype == torch.float32
                rec[f"{tag}_{k}"] = v.numpy()
    ref = f["multimodal_joint_emb"]
    err = np.abs(rec["text_joint_emb"] - ref).max()
    assert err <= 1e-6 * np.abs(ref).max(), (err, np.abs(ref).max())
    np.savez_compressed(OUT / "attn_mini.npz", **rec)
    print("wrote attn_mini.npz", {k: v.shape for k, v in rec.items()}, "joint_emb max|err|", float(err))


if __name__ == "__main__":
    main()
