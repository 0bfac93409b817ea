"""CPU checks of the `fp32_full` switch (pre-training in full fp32): the engine and the module mirror name what the switch is not built
for before anything touches a device, the entry point resolves `--compute fp32-full`, and the float64 references of
tests/fp32_full_ref.py agree with the oracle's own loss and front-end functions."""
import importlib
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import vlbert_oracle as O
from tests import fp32_full_ref as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "fixtures", "pretrain_small.yaml")


def pkg(name):
    return importlib.import_module("vl-bert_amd." + name)


@pytest.mark.parametrize("kw, cfg_kw, named", [
    (dict(core=True), {}, "core=True"),
    (dict(encoder_fp32=False), {}, "encoder_fp32=False"),
    (dict(image_size=(64, 64)), {}, "the image branch"),
    (dict(), dict(e2e=True), "the image branch"),
    (dict(B_aux=2), dict(multitask=True), "B_aux > 0"),
    (dict(), dict(with_pooler=True), "with_pooler / with_rel_loss"),
    (dict(), dict(with_pooler=True, with_rel_loss=True), "with_pooler / with_rel_loss"),
    (dict(dp_mode="sharded"), {}, "the sharded optimizer"),
    (dict(loss_scale="dynamic"), {}, "a loss scaler"),
    (dict(loss_scale=4096.0), {}, "a loss scaler"),
    (dict(T=200, R=100, max_seq=512), {}, "at most 256"),
])
def test_engine_names_what_fp32_full_is_not_built_for(kw, cfg_kw, named):
    E = pkg("engine")
    kw = dict(kw)
    T, R = kw.pop("T", 8), kw.pop("R", 4)
    args = dict(encoder_fp32=True, fp32_full=True)
    args.update(kw)
    with pytest.raises(ValueError, match="fp32_full.*unsupported here.*" + named.replace("(", r"\(")):
        E.PretrainEngine(E.ModelConfig(num_hidden_layers=2, **cfg_kw), 2, T, R, device="cpu", **args)


def test_engine_names_every_unsupported_piece_at_once():
    E = pkg("engine")
    with pytest.raises(ValueError) as e:
        E.PretrainEngine(E.ModelConfig(num_hidden_layers=2, multitask=True, with_pooler=True), 2, 8, 4, device="cpu", fp32_full=True, B_aux=1,
                         dp_mode="sharded", loss_scale="dynamic")
    for named in ("encoder_fp32=False", "B_aux > 0", "with_pooler", "sharded", "loss scaler"):
        assert named in str(e.value), named


def test_fp32_full_check_is_static_and_has_eval_step_refusal():
    """eval_step() of an fp32_full engine raises by name (checked on the source: the engine itself needs a GPU to be built)."""
    E = pkg("engine")
    E.PretrainEngine._check_fp32_full(E.ModelConfig(), 64, 36, False, True, None, "allreduce", 0, None)      # the supported call: silent
    E.PretrainEngine._check_fp32_full(E.ModelConfig(), 64, 36, False, True, None, "allreduce", 0, 1.0)

    class Stub:      # the refusal is the fp32 heads' (the engine's `back` under fp32_full), asked before anything runs
        core, back = False, object.__new__(pkg("pretrain_f32").PretrainF32)
    with pytest.raises(ValueError, match="eval_step: not built for an fp32_full engine"):
        E.PretrainEngine.eval_step(Stub())


def test_train_end2end_resolves_fp32_full():
    tr = pkg("pretrain.train_end2end")
    r = tr.main(["--cfg", CFG, "--compute", "fp32-full", "--dry-run"])
    assert r["compute"] == "fp32-full" and not r["e2e"] and not r["multitask"] and r["per_gpu_batch"] == 4
    assert tr.main(["--cfg", CFG, "--compute", "fp32", "--dry-run"])["compute"] == "fp32"      # keeps its meaning
    assert tr.main(["--cfg", CFG, "--compute", "cfg", "--dry-run"])["compute"] == "fp32"       # TRAIN.FP16: false
    assert tr.main(["--cfg", CFG, "--dry-run"])["compute"] == "bf16"
    with pytest.raises(ValueError, match="fp32-full: validation"):
        tr.main(["--cfg", CFG, "--compute", "fp32-full", "--val-steps", "2", "--dry-run"])


def test_module_mirror_names_what_fp32_full_is_not_built_for(monkeypatch):
    monkeypatch.delenv("VLB_ENCODER_FP32", raising=False)
    monkeypatch.delenv("VLB_FP32_FULL", raising=False)
    tr, M = pkg("pretrain.train_end2end"), pkg("pretrain.modules")
    config = tr.load_config(CFG)
    config.NETWORK.VLBERT["fp32_full"] = True
    with pytest.raises(NotImplementedError, match="fp32_full.*without fp32_encoder"):
        M.ResNetVLBERTForPretraining(config)
    config.NETWORK.VLBERT["fp32_encoder"] = True
    with pytest.raises(NotImplementedError, match="fp32_full.*multitask"):
        M.ResNetVLBERTForPretrainingMultitask(config)
    config.NETWORK.VLBERT["with_pooler"] = True
    with pytest.raises(NotImplementedError, match="fp32_full.*with_pooler"):
        M.ResNetVLBERTForPretraining(config)
    config.NETWORK.VLBERT["with_pooler"] = False
    del config.NETWORK.VLBERT["fp32_full"], config.NETWORK.VLBERT["fp32_encoder"]
    monkeypatch.setenv("VLB_FP32_FULL", "1")                           # the environment variables are the same switches
    with pytest.raises(NotImplementedError, match="fp32_full.*without fp32_encoder"):
        M.ResNetVLBERTForPretraining(config)


def test_loss_references_agree_with_the_oracle():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 37, generator=g) * 3
    labels = torch.tensor([4, -1, 36, 0, -1, 12])
    loss, grad, n = RF.ce_ref(x, labels, gscale=2.0)
    xo = x.clone().requires_grad_(True)
    lo = F.cross_entropy(xo, labels, ignore_index=-1)      # the call of O.pretrain_forward
    (2.0 * lo).backward()
    assert n == 4 and abs(float(loss) - float(lo.detach())) < 1e-6 and float((grad - xo.grad).abs().max()) < 1e-6
    assert float(grad[1].abs().max()) == 0.0
    sel = torch.tensor([0, 2, 3, 5, 1, 4])                           # compacted: the labelled rows first, padding (-1) behind them
    xc, lc = x[sel], labels[sel]
    l0, l1, gc = RF.ce_compact_ref(xc, lc, 4, 0, gscale=2.0)         # one group = the plain form
    assert abs(float(l0) - float(loss)) < 1e-12 and float(l1) == 0.0 and float((gc - grad[sel]).abs().max()) < 1e-12
    la, lb, _ = RF.ce_compact_ref(xc, lc, 2, 2)
    assert abs(float(la) * 2 + float(lb) * 2 - float(loss) * 4) < 1e-9      # the groups' sums add up
    assert RF.ce_ref(x, torch.full((6,), -1))[0] == 0 and float(RF.ce_ref(x, torch.full((6,), -1))[1].abs().max()) == 0.0
    t = torch.zeros(5, 37)
    t[0, 3], t[0, 9] = 0.6, 0.4
    t[2, 1] = 1.0
    t[3, 2] = 0.5                                                   # invalid: sums to 0.5
    ls, gs, tsum, nv = RF.soft_ce_ref(x[:5], t)
    xo = x[:5].clone().requires_grad_(True)
    lo = O.soft_cross_entropy(xo, t)
    lo.backward()
    assert nv == 2 and abs(float(ls) - float(lo.detach())) < 1e-6 and float((gs - xo.grad).abs().max()) < 1e-6
    assert float(gs[3].abs().max()) == 0.0 and float(RF.soft_ce_ref(x[:5], torch.zeros(5, 37))[0]) == 0.0
    assert float(O.soft_cross_entropy(x[:5], torch.zeros(5, 37))) == 0.0


def test_front_end_reference_agrees_with_the_oracle():
    """front_ref (float64, packed layout of S rows) against O.fast_rcnn_precomputed + O.vl_embedding (fp32, trimmed layout), eval mode."""
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64, vocab_size=128,
                         max_position_embeddings=64, visual_region_classes=16)
    params = O.init_params(cfg, seed=5)
    batch = list(syn.make_batch(3, 12, 6, seed=6, ragged=True))
    batch[2] = batch[2] % 120 * (batch[2] > 0)
    boxes, im_info, text, _, _, mvrc_ops, _ = batch
    S = 12 + 6 + 1
    ref = RF.front_ref(params, cfg, batch, S, torch.zeros(3, S, 64))
    box_mask = boxes[:, :, 0] > -1.5
    b2 = boxes.clone()
    b2[:, :, 4:][mvrc_ops == 1] = params["object_mask_visual_embedding.weight"][0]
    obj_reps = O.fast_rcnn_precomputed(params, cfg, b2, box_mask, im_info, False)
    ling = params["object_linguistic_embeddings.weight"][0].expand(3, 6, -1).clone()
    ling[mvrc_ops == 1] = params["object_mask_word_embedding.weight"][0]
    emb, mask, _, _ = O.vl_embedding(params, cfg, text, torch.zeros_like(text), obj_reps[:, 0:1].expand(-1, 12, -1), text > 0,
                                     torch.cat((obj_reps, ling), -1), box_mask, False)
    L = emb.shape[1]
    assert float((ref["obj_reps"] - obj_reps.double()).abs().max()) < 1e-5
    assert float(((ref["out"][:, :L] - emb.double()) * mask[..., None]).abs().max()) < 1e-4
    assert bool((RF.valid_rows(text > 0, box_mask, S)[:, :L] == mask).all())
