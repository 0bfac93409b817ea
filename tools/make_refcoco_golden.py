"""Generate tests/golden/refcoco/refcoco_small.npz by running the REAL reference RefCOCO+ module
(refcoco.modules.resnet_vlbert_for_refcoco.ResNetVLBERT) on CPU.  Runs only where the reference tree exists:

    python tools/make_refcoco_golden.py

Modelled on run_vqa_case in oracle/make_golden.py (whose helpers it imports read-only): 2 layers, hidden 64, precomputed region
features, every dropout at 0, parameters from tests/refcoco_oracle.init_refcoco_params loaded through the reference's own
load_state_dict.  The batch has padded boxes inside max_len (a short sample) and beyond it (columns no sample fills), several
positives per sample and non-unit im_info ratios.  Stored: the inputs, label_logits (padded columns included), the loss, the norm of
every parameter gradient, the full head gradients, pred_boxes of inference_forward, and the reference's state-dict keys and shapes.
The restatement (tests/refcoco_oracle.py) is checked against the reference before the file is written.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import refcoco_oracle as RO  # noqa: E402

HEAD = ["final_mlp.0.dense.weight", "final_mlp.0.dense.bias", "final_mlp.2.weight", "final_mlp.2.bias", "object_linguistic_embeddings.weight"]


def make_batch(cfg):
    g = torch.Generator().manual_seed(31)
    B, R0, L = 3, 9, 7
    nbox = torch.tensor([7, 4, 6])                  # max_len 7 < R0 = 9: columns 7, 8 are padding in every sample
    x1 = torch.rand(B, R0, generator=g) * 300
    y1 = torch.rand(B, R0, generator=g) * 200
    wh = 20 + torch.rand(B, R0, 2, generator=g) * 120
    boxes = torch.cat((torch.stack((x1, y1, x1 + wh[..., 0], y1 + wh[..., 1]), -1), torch.rand(B, R0, 2048, generator=g)), -1)
    im_info = torch.tensor([[480.0, 360.0, 0.75, 0.8], [500.0, 375.0, 1.25, 1.1], [640.0, 420.0, 0.6, 1.5]])
    boxes[:, 0, :4] = torch.stack((torch.zeros(B), torch.zeros(B), im_info[:, 0] - 1, im_info[:, 1] - 1), -1)   # ADD_IMAGE_AS_A_BOX
    pad = torch.arange(R0)[None, :] >= nbox[:, None]
    boxes[pad] = -2.0
    expression = torch.randint(200, cfg.vocab_size, (B, L), generator=g)
    expression[torch.arange(L)[None, :] >= torch.tensor([L, 3, 5])[:, None]] = 0
    label = torch.zeros(B, R0)
    label[0, [1, 4]] = 1.0
    label[1, [2]] = 1.0
    label[2, [1, 3, 5]] = 1.0
    label[pad] = -1.0
    return boxes, im_info, expression, label


def main():
    ref_import.import_reference()
    from refcoco.modules.resnet_vlbert_for_refcoco import ResNetVLBERT as RefRefCOCO
    cfg = RO.small_config()
    vocab_dir = ref_import.make_vocab_dir(os.path.join(tempfile.gettempdir(), "vlb_vocab_refcoco"), cfg.vocab_size)
    rc = ref_import.make_reference_config(cfg, vocab_dir)
    for k, v in dict(CLASSIFIER_DROPOUT=0.0, IMAGE_FEAT_PRECOMPUTED=True, IMAGE_FROZEN_BN=True, ENABLE_CNN_REG_LOSS=False).items():
        setattr(rc.NETWORK, k, v)
        rc.NETWORK[k] = v
    torch.manual_seed(0)
    model = RefRefCOCO(rc)
    pseed = 29
    params = RO.init_refcoco_params(cfg, pseed)
    sd = model.state_dict()
    missing = [k for k in sd if k not in params and not k.endswith("num_batches_tracked")]
    assert not missing, missing
    model.load_state_dict({k: params[k] for k in sd}, strict=True)
    model.train()
    model.image_feature_extractor.obj_downsample[0].p = 0.0
    boxes, im_info, expression, label = make_batch(cfg)
    outputs, loss = model(None, boxes.clone(), im_info, expression, label)
    loss.backward()
    grads = {k: v.grad.detach() for k, v in model.named_parameters() if v.grad is not None}
    model.eval()
    with torch.no_grad():
        inf = model(None, boxes.clone(), im_info, expression)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out2, loss2 = RO.refcoco_forward(leaves, cfg, boxes, im_info, expression, label)
    loss2.backward()
    err = float((out2["label_logits"] - outputs["label_logits"]).abs().max())
    print("restatement vs reference: |d logits|max %.3e, loss %.6f vs %.6f" % (err, float(loss2), float(loss)))
    assert err < 1e-4 and abs(float(loss2) - float(loss)) < 1e-5
    for k in HEAD:
        assert torch.allclose(leaves[k].grad, grads[k], atol=1e-6, rtol=1e-4), k
    o3, _ = RO.refcoco_forward(params, cfg, boxes, im_info, expression)
    assert torch.allclose(o3["pred_boxes"], inf["pred_boxes"], atol=1e-5)
    keys = sorted(grads)
    sd_keys = [k for k in sd if not k.endswith("num_batches_tracked")]
    path = os.path.join(ROOT, "tests", "golden", "refcoco", "refcoco_small.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, pseed=pseed, boxes=boxes.numpy(), im_info=im_info.numpy(), expression=expression.numpy(), label=label.numpy(),
                        logits=outputs["label_logits"].detach().numpy(), label_out=outputs["label"].numpy(), loss=float(loss),
                        grad_names=np.array(keys), grad_norms=np.array([float(grads[k].double().norm()) for k in keys]),
                        pred_boxes=inf["pred_boxes"].numpy(), inf_logits=inf["label_logits"].numpy(),
                        sd_keys=np.array(sd_keys), sd_shapes=np.array([",".join(str(d) for d in sd[k].shape) for k in sd_keys]),
                        **{"grad_" + k: grads[k].numpy() for k in HEAD})
    print("-> %s (%.1f KB), %d gradient tensors" % (path, os.path.getsize(path) / 1024, len(keys)))


if __name__ == "__main__":
    main()
