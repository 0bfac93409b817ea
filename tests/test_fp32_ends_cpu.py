"""CPU checks of the `fp32_ends` switch (fp32 front and back end of the VQA fine-tuning route): the entry point resolves it, the mirrors
and the engine reject the combinations it is not built for -- before anything touches a device."""
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg(name):
    return importlib.import_module("vl-bert_amd." + name)


def test_finetune_entry_resolves_fp32_full():
    fe = pkg("common.finetune_entry")
    cfg = os.path.join(ROOT, "tests", "fixtures", "vqa_small.yaml")
    r = fe.main("vqa", ["--cfg", cfg, "--compute", "fp32-full", "--dry-run"])
    assert r["compute"] == "fp32-full" and r["task"] == "vqa" and r["precomputed"]
    assert fe.main("vqa", ["--cfg", cfg, "--compute", "fp32", "--dry-run"])["compute"] == "fp32"      # keeps its meaning
    for task in ("vcr", "refcoco"):      # the other tasks' routes are not built in fp32
        with pytest.raises(NotImplementedError, match="fp32-full"):
            fe.main(task, ["--cfg", os.path.join(ROOT, "tests", "fixtures", "%s_small.yaml" % task), "--compute", "fp32-full", "--dry-run"])


class _A(dict):
    __getattr__ = dict.__getitem__


def _vqa_conf(**vl):
    vlbert = _A(hidden_size=128, visual_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=512,
                max_position_embeddings=64, type_vocab_size=3, visual_region_classes=50, visual_ln=True, with_pooler=False,
                hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, initializer_range=0.02, object_word_embed_mode=2)
    vlbert.update(vl)
    return _A(NETWORK=_A(IMAGE_FEAT_PRECOMPUTED=True, IMAGE_SEMANTIC=False, BLIND=False, NO_GROUNDING=False, ENABLE_CNN_REG_LOSS=False,
                         CLASSIFIER_TYPE="mlm", CLASSIFIER_DROPOUT=0.1, CLASSIFIER_HIDDEN_SIZE=96, IMAGE_FINAL_DIM=128, VLBERT=vlbert),
              DATASET=_A(ANSWER_VOCAB_SIZE=37))


def test_mirrors_reject_fp32_ends_without_fp32_encoder(monkeypatch):
    monkeypatch.delenv("VLB_ENCODER_FP32", raising=False)
    monkeypatch.delenv("VLB_FP32_ENDS", raising=False)
    VLB = pkg("common.visual_linguistic_bert")
    VQA = pkg("vqa.modules.resnet_vlbert_for_vqa")
    with pytest.raises(ValueError, match="fp32_ends requires fp32_encoder"):
        VLB.VisualLinguisticBert(_vqa_conf(fp32_ends=True).NETWORK.VLBERT)
    with pytest.raises(ValueError, match="fp32_ends requires fp32_encoder"):
        VQA.ResNetVLBERT(_vqa_conf(fp32_ends=True))
    monkeypatch.setenv("VLB_FP32_ENDS", "1")                           # the environment variable is the same switch
    with pytest.raises(ValueError, match="fp32_ends requires fp32_encoder"):
        VQA.ResNetVLBERT(_vqa_conf())
    assert VLB.fp32_flags(_A(fp32_encoder=True)) == (True, True)
    monkeypatch.delenv("VLB_FP32_ENDS")
    assert VLB.fp32_flags(_A(fp32_encoder=True)) == (True, False)


def test_mirrors_name_the_routes_fp32_ends_is_not_built_for(monkeypatch):
    monkeypatch.delenv("VLB_ENCODER_FP32", raising=False)
    monkeypatch.delenv("VLB_FP32_ENDS", raising=False)
    VLB = pkg("common.visual_linguistic_bert")
    VQA = pkg("vqa.modules.resnet_vlbert_for_vqa")
    both = dict(fp32_encoder=True, fp32_ends=True)
    with pytest.raises(NotImplementedError, match="pooler"):
        VLB.VisualLinguisticBert(_vqa_conf(with_pooler=True, **both).NETWORK.VLBERT)
    with pytest.raises(NotImplementedError, match="pre-training heads"):
        VLB.VisualLinguisticBertForPretraining(_vqa_conf(**both).NETWORK.VLBERT, with_rel_head=False)
    conf = _vqa_conf(**both)
    conf.NETWORK["IMAGE_FEAT_PRECOMPUTED"] = False
    with pytest.raises(NotImplementedError, match="image branch"):
        VQA.ResNetVLBERT(conf)
    RC = pkg("refcoco.modules.resnet_vlbert_for_refcoco")
    with pytest.raises(NotImplementedError, match="VQA fine-tuning route only"):
        RC.ResNetVLBERT(_vqa_conf(**both))


def test_engine_rejects_unsupported_fp32_ends_combinations():
    E = pkg("engine")
    ok = dict(core=True, core_heads=False, core_sequence=True, encoder_fp32=True, fp32_ends=True, device="cpu")
    cases = [
        (dict(core=False), {}, "core=False"),                                           # the pre-training engine, its heads and losses
        (dict(core_heads=True), {}, "MLM / MVRC / relationship heads"),
        (dict(core_sequence=False), {}, "returned separately"),
        (dict(encoder_fp32=False), {}, "encoder_fp32=False"),
        ({}, dict(with_pooler=True), "pooler"),                                          # VCR
        (dict(image_size=(64, 64)), {}, "image branch"),
        (dict(dp_mode="sharded"), {}, "sharded optimizer"),
    ]
    for kw, ckw, what in cases:
        mc = E.ModelConfig(num_hidden_layers=2, **ckw)
        with pytest.raises(ValueError, match="fp32_ends") as ei:
            E.PretrainEngine(mc, 2, 12, 5, **dict(ok, **kw))
        assert what in str(ei.value), (what, str(ei.value))
    with pytest.raises(ValueError, match="at most 256"):                                 # beyond the fp32 encoder's 256 positions
        E.PretrainEngine(E.ModelConfig(num_hidden_layers=2), 2, 200, 100, max_seq=512, **ok)
