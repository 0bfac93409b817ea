"""RefCOCO+ grounding head on the MI355X: the kernels of csrc/grounding.hip against fp32 torch on the same 16-bit inputs, the module
mirror against the fixture of the reference's own module (tests/golden/refcoco/refcoco_small.npz) and the CPU restatement, the
training entry point in a child process, and PARTIAL_PRETRAIN with the shipped prefix changes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vlbert_oracle as O
from tests import refcoco_oracle as RO
from tests.gpu_util import act_dtype, dev, pkg, report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "refcoco", "refcoco_small.npz")
TAG = 2003
RO_HEAD = ["final_mlp.0.dense.weight", "final_mlp.0.dense.bias", "final_mlp.2.weight", "final_mlp.2.bias", "object_linguistic_embeddings.weight"]


def rel_fro(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / max(b.norm(), 1e-12))


def _head_inputs(B, R, R0, H, seed):
    g = torch.Generator().manual_seed(seed)
    ops = pkg("ops")
    gx = (torch.randn(B * R, H, generator=g) * 0.7).to(ops.BF16).to(dev())
    dg = (torch.rand(B * R, H, generator=g) * 1.2 - 0.1).to(ops.BF16).to(dev())
    w2 = (torch.randn(H, generator=g) / H ** 0.5).to(dev())
    b2 = torch.randn(1, generator=g).to(dev())
    nbox = torch.randint(1, R + 1, (B,), generator=g)
    nbox[0] = R
    boxes = torch.rand(B, R0, 4, generator=g) * 100
    boxes[torch.arange(R0)[None, :] >= nbox[:, None]] = -2.0
    label = (torch.rand(B, R0, generator=g) < 0.3).float()
    label[boxes[:, :, 0] < -1.5] = -1.0
    return gx, dg, w2, b2, boxes.to(dev()), label.to(dev())


def _keep_mask(rows, H, p, seed):
    """the 0/1 mask of vlb_dropout_bf16 on a contiguous [rows, H] tensor under (seed, TAG)"""
    ops = pkg("ops")
    ones = torch.ones(rows, H, dtype=ops.BF16, device=dev())
    return (ops.dropout_bf16(ones, torch.empty_like(ones), p, seed, TAG) != 0).float()


@pytest.mark.parametrize("B,R,R0,H,p", [(3, 7, 9, 128, 0.0), (3, 7, 9, 128, 0.1), (4, 100, 104, 768, 0.1)])
def test_grounding_kernels_match_torch(B, R, R0, H, p):
    ops = pkg("ops")
    gx, dg, w2, b2, boxes, label = _head_inputs(B, R, R0, H, 7 + H)
    seed = torch.tensor([12345], dtype=torch.int32, device=dev())
    thr = 0 if p <= 0 else min(int(p * 65536.0 + 0.5), 65535)
    scale = 65536.0 / (65536.0 - thr) if thr else 1.0
    mask = _keep_mask(B * R, H, p, seed) if p > 0 else torch.ones(B * R, H, device=dev())
    x1 = gx.float() * mask * scale
    # score forward: every B x max_len row, -10000 beyond max_len
    logits = torch.full((B, R0), 7.0, device=dev())
    ops.ground_score_fwd(gx, w2, b2, logits, B, R, drop_p=p, seed=seed, tag=TAG)
    ref = (x1.double() @ w2.double() + b2.double()).view(B, R)
    assert (logits[:, R:] == -10000.0).all()
    err = float((logits[:, :R].double() - ref).abs().max())
    assert err <= 1e-5 * float(ref.abs().max()), err
    # masked BCE against torch on the masked set
    loss = torch.empty((), device=dev())
    dlogit = torch.full((B * R,), 3.0, device=dev())
    ops.ground_bce(logits, boxes, label, R, loss, dlogit)
    xl = logits[:, :R].clone().requires_grad_(True)
    m = boxes[:, :R, 0] > -1.5
    tl = F.binary_cross_entropy_with_logits(xl[m], label[:, :R][m])
    tl.backward()
    tl_v = float(tl.detach())
    assert abs(float(loss) - tl_v) <= 1e-5 * abs(tl_v), (float(loss), tl_v)
    assert torch.allclose(dlogit.view(B, R), xl.grad, rtol=1e-5, atol=1e-5 * float(xl.grad.abs().max()))
    assert (dlogit.view(B, R)[~m] == 0).all()
    # score backward: du within 1 ulp of the 16-bit type, dw2 / db2 within 1e-5, bitwise reproducible
    gl = torch.tensor([0.37], device=dev())
    outs = []
    for _ in range(2):
        du = torch.full((B * R, H), 5.0, dtype=ops.BF16, device=dev())
        dw2, db2 = torch.full((H,), 9.0, device=dev()), torch.full((1,), 9.0, device=dev())
        ops.ground_score_bwd(gl, dlogit, gx, dg, w2, du, dw2, db2, drop_p=p, seed=seed, tag=TAG)
        outs.append((du, dw2, db2))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    du, dw2, db2 = outs[0]
    s = (0.37 * dlogit.double())[:, None]
    du_ref = s * w2.double()[None, :] * (mask * scale).double() * dg.double()
    fi = torch.finfo(act_dtype())
    ulp = fi.eps                                           # 2^-7 (bfloat16) | 2^-10 (fp16)
    sub = max(1e-30, fi.tiny * fi.eps)                     # 1 ulp of a subnormal result: 2^-24 in fp16 (|du| here goes below 2^-14)
    assert ((du.double() - du_ref).abs() <= du_ref.abs() * ulp + sub).all()
    dw2_ref = (s * x1.double()).sum(0)
    assert float((dw2.double() - dw2_ref).abs().max()) <= 1e-5 * float(dw2_ref.abs().max())
    assert abs(float(db2) - float(s.sum())) <= 1e-5 * max(abs(float(s.sum())), 1e-6)


def test_grounding_bce_without_valid_boxes_is_nan_with_zero_gradient():
    ops = pkg("ops")
    B, R, R0 = 2, 3, 5
    boxes = torch.full((B, R0, 4), -2.0, device=dev())
    logits = torch.randn(B, R0, device=dev())
    label = torch.zeros(B, R0, device=dev())
    loss = torch.zeros((), device=dev())
    dlogit = torch.full((B * R,), 3.0, device=dev())
    ops.ground_bce(logits, boxes, label, R, loss, dlogit)
    assert torch.isnan(loss) and (dlogit == 0).all()


def test_grounding_pick_box_matches_torch_argmax():
    """first index on ties; a padded row inside max_len can win (its logit is final_mlp(0)) and is picked as the reference picks it"""
    ops = pkg("ops")
    B, R0, ld = 3, 9, 6
    g = torch.Generator().manual_seed(3)
    boxes = torch.rand(B, R0, ld, generator=g) * 200
    boxes[1, 4:] = -2.0
    logits = torch.randn(B, R0, generator=g)
    logits[:, 7:] = -10000.0
    logits[0, 2] = logits[0, 5] = 5.0                      # tie
    logits[1, 4:7] = 3.0                                   # padded rows inside max_len = 7 win (ties among them too)
    logits[2, 0] = 5.5
    im_info = torch.tensor([[400.0, 300.0, 0.8, 1.25], [400.0, 300.0, 1.5, 0.5], [400.0, 300.0, 1.0, 2.0]])
    pred = torch.empty(B, 4, device=dev())
    idx = torch.empty(B, dtype=torch.int64, device=dev())
    ops.ground_pick_box(logits.to(dev()), boxes.to(dev()), im_info.to(dev()), pred, idx)
    ri = logits.argmax(1)
    rp = boxes[torch.arange(B), ri, :4].clone()
    rp[:, [0, 2]] /= im_info[:, 2:3]
    rp[:, [1, 3]] /= im_info[:, 3:4]
    assert idx.cpu().tolist() == ri.tolist() == [2, 4, 0]
    assert torch.equal(pred.cpu(), rp)


def _refcoco_config(cfg, drop):
    class A(dict):
        __getattr__ = dict.__getitem__
    vl = A(hidden_size=cfg.hidden_size, visual_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
           num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size, vocab_size=cfg.vocab_size,
           max_position_embeddings=cfg.max_position_embeddings, type_vocab_size=3, visual_ln=True, with_pooler=False,
           hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, initializer_range=0.02, visual_scale_text_init=0.0,
           visual_scale_object_init=0.0, object_word_embed_mode=2)
    return A(NETWORK=A(IMAGE_FEAT_PRECOMPUTED=True, IMAGE_SEMANTIC=False, IMAGE_FINAL_DIM=cfg.hidden_size, BLIND=False, NO_GROUNDING=False,
                       ENABLE_CNN_REG_LOSS=False, CLASSIFIER_DROPOUT=drop, VLBERT=vl))


def test_refcoco_module_mirror_vs_reference_fixture_and_oracle():
    M = pkg("refcoco.modules.resnet_vlbert_for_refcoco")
    z = np.load(FIXTURE, allow_pickle=False)
    cfg = RO.small_config()
    params = RO.init_refcoco_params(cfg, int(z["pseed"]))
    net = M.ResNetVLBERT(_refcoco_config(cfg, 0.0), device="cuda:0")
    sd = net.state_dict()
    ref_keys = [str(k) for k in z["sd_keys"]]
    assert set(sd) == set(ref_keys), set(sd) ^ set(ref_keys)
    for k, s in zip(ref_keys, z["sd_shapes"]):
        assert tuple(sd[k].shape) == tuple(int(d) for d in str(s).split(",") if d), k
    net.load_state_dict(params)
    net.train()
    for m in (net.vlbert, net.image_feature_extractor):          # deterministic comparison: every dropout off (as in the fixture)
        m.eval()
    boxes, im_info, expression, label = [torch.from_numpy(z[k]).to(dev()) for k in ("boxes", "im_info", "expression", "label")]
    outputs, loss = net.train_forward(None, boxes, im_info, expression, label)
    ml = 7                                                          # max_len of the fixture batch; columns 7, 8 are padding
    report("refcoco label_logits vs reference fixture", outputs["label_logits"][:, :ml], torch.from_numpy(z["logits"][:, :ml]), 2e-2, 2e-2)
    assert (outputs["label_logits"][:, ml:] == -10000.0).all() and (z["logits"][:, ml:] == -10000.0).all()
    assert torch.equal(outputs["label"].cpu(), torch.from_numpy(z["label_out"]))
    assert abs(float(outputs["cls_loss"].detach()) - float(z["loss"])) < 1e-2 * float(z["loss"])
    loss.backward()
    got = dict(net.named_parameters())
    norms = dict(zip([str(k) for k in z["grad_names"]], z["grad_norms"]))
    for k, n in norms.items():
        gn = float(got[k].grad.double().norm())
        print("  refcoco d %s norm %.4e vs %.4e" % (k, gn, n))
        assert abs(gn - n) <= (0.15 if "obj_downsample" in k else 0.1) * n + 1e-6, k
    for k in RO_HEAD:
        e = rel_fro(got[k].grad, torch.from_numpy(z["grad_" + k]))
        print("  refcoco d %s rel-fro %.3e" % (k, e))
        assert e < 5e-2, k
    for k in ("vlbert.encoder.layer.1.output.dense.weight", "image_feature_extractor.obj_downsample.1.weight"):
        assert got[k].grad is not None and float(got[k].grad.norm()) > 0
    net.eval()
    inf = net(None, boxes, im_info, expression)
    report("refcoco inference logits", inf["label_logits"][:, :ml], torch.from_numpy(z["inf_logits"][:, :ml]), 2e-2, 2e-2)
    assert (inf["label_logits"][:, ml:] == -10000.0).all()
    assert torch.allclose(inf["pred_boxes"].cpu(), torch.from_numpy(z["pred_boxes"]), atol=1e-3)
    # classifier dropout 0.1 in eval mode = no dropout: the mirror against the CPU restatement
    net.cls_drop = 0.1
    inf2 = net(None, boxes, im_info, expression)
    out, _ = RO.refcoco_forward(params, cfg, *[torch.from_numpy(z[k]) for k in ("boxes", "im_info", "expression")],
                                classifier_dropout=0.1, train=False)
    report("refcoco eval logits (dropout 0.1) vs oracle", inf2["label_logits"][:, :ml], out["label_logits"][:, :ml], 2e-2, 2e-2)
    assert torch.allclose(inf2["pred_boxes"].cpu(), out["pred_boxes"], atol=1e-3)
    # classifier dropout on in training: runs, finite, different from the deterministic loss
    net.train()
    net.zero_grad()
    _, l2 = net.train_forward(None, boxes, im_info, expression, label)
    l2.backward()
    assert torch.isfinite(l2) and abs(float(l2.detach()) - float(loss.detach())) > 0
    assert torch.isfinite(got["final_mlp.2.weight"].grad).all()


def test_refcoco_entry_point_runs_the_reference_style_config(tmp_path):
    """`python -m vl-bert_amd.refcoco.train_end2end` on tests/fixtures/refcoco_small.yaml: image branch, AdamW + triangle schedule + clip
    1.0, TRAIN.FP16 false -> fp32 encoder on the f16 build (--compute cfg), 3 steps of 2 micro-batches, checkpoint to --model-dir."""
    cfg = os.path.join(ROOT, "tests", "fixtures", "refcoco_small.yaml")
    mdir = str(tmp_path / "model")
    cmd = [sys.executable, "-c", "import importlib,sys; sys.path.insert(0, %r); m = importlib.import_module('vl-bert_amd.refcoco.train_end2end'); "
           "net, opt, loss = m.main(%r); import math; assert math.isfinite(loss), loss; print('LR %%.9e LOSS %%.5f' %% (opt.param_groups[0]['lr'], loss))"
           % (ROOT, ["--cfg", cfg, "--steps", "3", "--compute", "cfg", "--model-dir", mdir])]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout[-1500:])
    print(r.stderr[-1500:])
    assert r.returncode == 0, r.stderr[-1500:]
    assert "compute fp32" in r.stdout and "step 3" in r.stdout
    line = next(l for l in r.stdout.splitlines() if l.startswith("LR "))
    lr3 = 8.0e-7 * 2 * 2 * (2.0 / 4.0)                         # warm-up 4 steps: the schedule at the last step run (k = 2)
    assert abs(float(line.split()[1]) - lr3) < 1e-6 * lr3, line
    ck = torch.load(os.path.join(mdir, "vl-bert_small_refcoco-0000.model"), map_location="cpu", weights_only=False)["state_dict"]
    z = np.load(FIXTURE, allow_pickle=False)
    ref = set(str(k) for k in z["sd_keys"])
    own = set(ck)
    body = lambda keys: {k for k in keys if not k.startswith("image_feature_extractor.")}
    assert body(own) == body(ref), body(own) ^ body(ref)          # the image branch adds the backbone in place of the features
    assert {"image_feature_extractor.obj_downsample.1.weight", "image_feature_extractor.obj_downsample.1.bias"} <= own
    assert any(k.startswith("image_feature_extractor.backbone.") for k in own)
    assert all(torch.isfinite(v).all() for v in ck.values() if v.is_floating_point())


def test_refcoco_partial_pretrain_fills_the_transform_from_the_mvrc_head():
    M = pkg("refcoco.modules.resnet_vlbert_for_refcoco")
    C = pkg("common.checkpoint")
    cfg = O.VLBertConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, vocab_size=300,
                         max_position_embeddings=64, visual_region_classes=50)
    net = M.ResNetVLBERT(_refcoco_config(cfg, 0.0), device="cuda:0")
    sd = torch.load(os.path.join(ROOT, "tests", "golden", "checkpoint", "ref_small-0000.model"), map_location="cpu", weights_only=False)
    sd = sd.get("state_dict", sd)
    changes = ["vlbert.mvrc_head.transform->final_mlp.0", "module.vlbert.mvrc_head.transform->module.final_mlp.0", "vlbert->vlbert",
               "module.vlbert->module.vlbert"]
    new = C.partial_pretrain_state_dict(sd, changes)
    new, _ = C.drop_shape_mismatches(new, net.state_dict())
    C.smart_partial_load(net, new)
    got = dict(net.named_parameters())
    for k in ("weight", "bias"):
        assert torch.equal(got["final_mlp.0.dense." + k].detach().cpu(), sd["vlbert.mvrc_head.transform.dense." + k].float())
    assert torch.equal(got["vlbert.word_embeddings.weight"].detach().cpu(), sd["vlbert.word_embeddings.weight"].float())
