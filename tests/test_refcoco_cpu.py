"""RefCOCO+ fine-tuning on the CPU: the restatement (tests/refcoco_oracle.py) against the fixture produced by the reference's own
module, the entry point's resolved configuration, and the C ABI of the grounding head.  No GPU."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import refcoco_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "refcoco", "refcoco_small.npz")
CFG = os.path.join(ROOT, "tests", "fixtures", "refcoco_small.yaml")
HEAD = ["final_mlp.0.dense.weight", "final_mlp.0.dense.bias", "final_mlp.2.weight", "final_mlp.2.bias", "object_linguistic_embeddings.weight"]
NEW_SYMBOLS = {"vlb_ground_score_fwd": "plipppliiifpus", "vlb_ground_bce": "plpllpliipps", "vlb_ground_score_bwd": "ppiplplipplppfpus",
               "vlb_ground_pick_box": "pliipllplpps"}


def load_case():
    z = np.load(FIXTURE, allow_pickle=False)
    cfg = RO.small_config()
    params = RO.init_refcoco_params(cfg, int(z["pseed"]))
    batch = tuple(torch.from_numpy(z[k]) for k in ("boxes", "im_info", "expression", "label"))
    return z, cfg, params, batch


def test_restatement_matches_reference_fixture():
    """logits at every origin_len column (padded rows inside max_len = final_mlp(0), -10000 beyond), loss, every gradient norm, the
    full head gradients, inference pred_boxes."""
    z, cfg, params, batch = load_case()
    boxes = batch[0]
    valid = (boxes[:, :, 0] > -1.5).numpy()
    max_len = int(valid.sum(1).max())
    assert max_len < boxes.shape[1] and not valid[:, :max_len].all()           # padding both inside and beyond max_len
    assert ((z["label"] == 1).sum(1) >= 1).all() and ((z["label"] == 1).sum(1) > 1).any()
    assert not np.allclose(z["im_info"][:, 2:], 1.0)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out, loss = RO.refcoco_forward(leaves, cfg, *batch)
    logits = out["label_logits"].detach().numpy()
    assert np.allclose(logits, z["logits"], atol=1e-5)
    assert (z["logits"][:, max_len:] == -10000.0).all()
    pad_in = ~valid[:, :max_len]
    assert np.allclose(z["logits"][:, :max_len][pad_in], z["logits"][:, :max_len][pad_in][0])   # one constant: final_mlp(0)
    assert abs(float(loss) - float(z["loss"])) < 1e-5
    loss.backward()
    for k, n in zip(z["grad_names"], z["grad_norms"]):
        g = leaves[str(k)].grad
        assert g is not None and abs(float(g.double().norm()) - n) <= 1e-4 * n + 1e-9, k
    for k in HEAD:
        assert np.allclose(leaves[k].grad.numpy(), z["grad_" + k], atol=1e-6, rtol=1e-4), k
    inf, _ = RO.refcoco_forward(params, cfg, *batch[:3])
    assert np.allclose(inf["pred_boxes"].numpy(), z["pred_boxes"], atol=1e-5)
    assert np.allclose(inf["label_logits"].numpy(), z["inf_logits"], atol=1e-5)
    assert set(str(k) for k in z["sd_keys"]) == set(params)


def test_text_preparation():
    ids, types, mask = RO.prepare_text(torch.tensor([[7, 8, 9], [5, 0, 0]]))
    assert ids.tolist() == [[101, 7, 8, 9, 102], [101, 5, 102, 0, 0]]
    assert not types.any() and mask.tolist() == [[True] * 5, [True, True, True, False, False]]


def test_dry_run_resolves_the_refcoco_yaml():
    tr = importlib.import_module("vl-bert_amd.refcoco.train_end2end")
    r = tr.main(["--cfg", CFG, "--dry-run", "--compute", "cfg"])
    assert r["task"] == "refcoco" and r["module"] == "ResNetVLBERT"
    assert (r["per_gpu_batch"], r["accumulate"], r["world"]) == (2, 2, 1)
    assert r["lr"] == pytest.approx(8.0e-7 * 1 * 2 * 2)
    assert r["optimizer"] == "AdamW" and r["clip_grad_norm"] == 1.0 and r["lr_schedule"] == "triangle" and r["warmup_steps"] == 4
    assert r["compute"] == "fp32" and r["precomputed"] is False


def test_refcoco_defaults_follow_the_reference_config():
    fe = importlib.import_module("vl-bert_amd.common.finetune_entry")
    c = fe.load_config("refcoco", None)
    assert c.NETWORK.IMAGE_FEAT_PRECOMPUTED is False and c.NETWORK.CLASSIFIER_DROPOUT == 0.1 and c.TRAIN.OPTIMIZER == "SGD"
    assert c.DATASET.ADD_IMAGE_AS_A_BOX is True


def test_synthetic_refcoco_batch_layout():
    syn = importlib.import_module("vl-bert_amd.synthetic")
    image, boxes, im_info, expression, label = syn.make_refcoco_batch(3, 10, 8, 64, 96, 5, "cpu")
    assert image.shape == (3, 3, 64, 96) and boxes.shape == (3, 10, 4) and im_info.shape == (3, 4)
    valid = boxes[:, :, 0] > -1.5
    assert valid[:, 0].all() and not valid.all() and (boxes[~valid] == -2).all()
    assert torch.equal(boxes[:, 0], torch.tensor([[0.0, 0.0, 95.0, 63.0]] * 3))
    assert (label[~valid] == -1).all() and ((label[valid] == 0) | (label[valid] == 1)).all() and (label[valid] == 1).sum() > 3
    assert not torch.allclose(im_info[:, 2:], torch.ones(3, 2))
    assert expression.shape == (3, 8) and (expression == 0).any()
    _, pb, _, _, _ = syn.make_refcoco_batch(2, 6, 5, 64, 96, 5, "cpu", precomputed=True)
    assert pb.shape == (2, 6, 4 + 2048)


def test_header_and_bindings_declare_the_grounding_entry_points():
    from tests.test_abi import header_prototypes
    lib = importlib.import_module("vl-bert_amd._lib")
    protos = header_prototypes()
    for name, sig in NEW_SYMBOLS.items():
        assert protos.get(name) == sig, name
        assert lib._SIGS.get(name) == sig, name
    build = open(os.path.join(ROOT, "vl-bert_amd", "csrc", "build.sh")).read()
    assert " grounding" in build.split("SRCS=")[1].split("\n")[0]
