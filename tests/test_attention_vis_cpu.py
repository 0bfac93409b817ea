"""What of the attention-map feature can be checked without a GPU: the entry point's configuration plumbing
(vl-bert_amd/pretrain/vis_attention_maps.py --dry-run, the coco_captions refusal, train_end2end's pointer to it), the mirror's parameter
names against the live reference module where the reference tree exists, and the compile-outcome contract of
vl-bert_amd/csrc/attention_probs.hip in both builds (tools/isa_lint.py; hipcc cross-compiles gfx950 here)."""
import importlib
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "fixtures", "attention_vis_small.yaml")
REFERENCE = os.environ.get("VLBERT_REFERENCE_ROOT", "/root/reference")
has_reference = pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="reference tree not present (GPU box)")

spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(ROOT, "tools", "isa_lint.py"))
L = importlib.util.module_from_spec(spec)
spec.loader.exec_module(L)
SRC = os.path.join(ROOT, "vl-bert_amd", "csrc", "attention_probs.hip")


def entry():
    return importlib.import_module("vl-bert_amd.pretrain.vis_attention_maps")


def test_dry_run_prints_the_resolved_configuration(capsys, tmp_path):
    r = entry().main(["--cfg", FIXTURE, "--save-dir", str(tmp_path), "--dry-run"])
    shown = json.loads(capsys.readouterr().out)
    assert shown["resolved"]["module"] == "ResNetVLBERTForAttentionVis" and shown["NETWORK.VLBERT"]["num_hidden_layers"] == 2
    assert r["layers"] == 2 and r["heads"] == 12 and r["per_gpu_batch"] == 1 and not r["e2e"] and not r["data"] and r["steps"] == 2
    assert r["save_dir"] == os.path.join(str(tmp_path), "attention_probs") and r["compute"] == "bf16"
    assert not os.listdir(str(tmp_path))                       # nothing is written
    assert entry().main(["--cfg", FIXTURE, "--dry-run", "--compute", "fp16", "--steps", "5", "--batch-images", "3"])["per_gpu_batch"] == 3


def _with(tmp_path, **edits):
    import yaml
    with open(FIXTURE) as f:
        cfg = yaml.safe_load(f)
    for k, v in edits.items():
        cfg[k] = v
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def test_coco_captions_is_refused_with_the_documented_message(tmp_path):
    path = _with(tmp_path, DATASET=dict(DATASET="coco_captions", DATASET_PATH="./data/coco", VAL_IMAGE_SET="val"))
    with pytest.raises(NotImplementedError, match="pycocotools"):
        entry().main(["--cfg", path, "--data", "--dry-run"])
    assert entry().main(["--cfg", path, "--dry-run"])["dataset"] == "coco_captions"       # synthetic batches: the DATASET section is not read
    with pytest.raises(NotImplementedError, match="ResNetVLBERTForAttentionVis"):
        entry().main(["--cfg", _with(tmp_path, MODULE="ResNetVLBERTForPretraining"), "--dry-run"])


def test_a_configured_checkpoint_that_is_missing_is_an_error_before_any_gpu_work(tmp_path):
    import yaml
    with open(FIXTURE) as f:
        cfg = yaml.safe_load(f)
    cfg["NETWORK"]["PARTIAL_PRETRAIN"] = str(tmp_path / "no-such.model")
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    with pytest.raises(FileNotFoundError, match="PARTIAL_PRETRAIN"):
        entry().main(["--cfg", path, "--save-dir", str(tmp_path / "maps")])
    assert not os.path.exists(str(tmp_path / "maps"))


def test_ranks_name_their_synthetic_samples_apart():
    import torch
    V, syn = entry(), importlib.import_module("vl-bert_amd.synthetic")
    r = dict(per_gpu_batch=2, text_len=8, regions=4, steps=3, e2e=False)
    index = [[int(b[2][i][-1]) for b in V._synthetic_batches(r, rank, syn, torch) for i in range(2)] for rank in (0, 1)]
    assert index == [list(range(6)), list(range(6, 12))]
    assert V.image_id_of(V._SyntheticSet(12), 7) == "synthetic_000007"


def test_train_end2end_names_the_entry_point_for_this_module():
    te = importlib.import_module("vl-bert_amd.pretrain.train_end2end")
    with pytest.raises(NotImplementedError, match=r"vl-bert_amd\.pretrain\.vis_attention_maps"):
        te.main(["--cfg", FIXTURE, "--dry-run"])


@has_reference
def test_the_reference_yaml_resolves():
    r = entry().main(["--cfg", os.path.join(REFERENCE, "cfgs", "pretrain", "vis_attention_maps_coco.yaml"), "--dry-run"])
    assert r["module"] == "ResNetVLBERTForAttentionVis" and r["e2e"] and r["layers"] == 12 and r["heads"] == 12 and r["per_gpu_batch"] == 1
    assert r["dataset"] == "coco_captions" and r["partial_pretrain"].endswith("vl-bert-base-e2e.model") and r["prefix_changes"] == []


@has_reference
def test_mirror_parameter_names_equal_the_reference_modules_state_dict_keys(tmp_path):
    """The reference's own ResNetVLBERTForAttentionVis, imported live and built on the CPU for the fixture configuration."""
    from oracle import ref_import
    from oracle import vlbert_oracle as O
    ref_import.import_reference()
    from pretrain.modules.resnet_vlbert_for_attention_vis import ResNetVLBERTForAttentionVis as Ref
    te = importlib.import_module("vl-bert_amd.pretrain.train_end2end")
    M = importlib.import_module("vl-bert_amd.pretrain.modules.resnet_vlbert_for_attention_vis")
    for edits in ({}, {"WITH_MVRC_LOSS": False}):
        config = te.load_config(FIXTURE)
        config.NETWORK.update(edits)
        vl = config.NETWORK.VLBERT
        ocfg = O.VLBertConfig(hidden_size=vl.hidden_size, num_hidden_layers=vl.num_hidden_layers, num_attention_heads=vl.num_attention_heads,
                              intermediate_size=vl.intermediate_size, vocab_size=vl.vocab_size,
                              max_position_embeddings=vl.max_position_embeddings)
        rc = ref_import.make_reference_config(ocfg, ref_import.make_vocab_dir(str(tmp_path / "vocab"), 200))
        for k in ("IMAGE_FEAT_PRECOMPUTED", "MASK_RAW_PIXELS", "WITH_MVRC_LOSS", "IMAGE_FINAL_DIM"):
            rc.NETWORK[k] = config.NETWORK[k]
        ref_keys = set(Ref(rc).state_dict().keys())
        assert set(M.parameter_names(config)) == ref_keys, sorted(set(M.parameter_names(config)) ^ ref_keys)
        assert ("object_mask_word_embedding.weight" in ref_keys) == bool(config.NETWORK.WITH_MVRC_LOSS)


def stated_vgpr_budget():
    with open(SRC) as f:
        head = f.read().split("#include")[0]
    m = re.search(r"at most (\d+) VGPRs", head)
    assert m, "the header of attention_probs.hip must state its register budget"
    assert re.search(r"LDS \d+ KB", head), "the header of attention_probs.hip must state its LDS budget"
    return int(m.group(1))


@pytest.mark.skipif(not L.available(), reason="hipcc not installed")
@pytest.mark.parametrize("defines", [(), ("-DVLB_ACT_F16",)], ids=["bf16", "f16"])
def test_attention_probs_kernel_compiles_clean(defines):
    budget = stated_vgpr_budget()
    assert budget <= 64           # one 32-key group's scores at a time: half of what waves_per_eu(4, 4) would allow
    ks = L.kernels(L.compile_isa(SRC, defines))
    assert len(ks) == 1, sorted(ks)
    k = L.find(ks, "attn_probs_kernel")
    assert k["spill"] == 0 and k["scratch"] == 0, (k["spill"], k["scratch"])
    assert k["vgpr"] + k["agpr"] <= budget, (k["vgpr"], k["agpr"])
    assert not L.landing_register_violations(k["body"])
    assert L.serialized_loads(k["body"]) == 0
    assert not any(re.match(r"^\s+scratch_", l) for l in k["body"])
