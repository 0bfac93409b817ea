"""tests/golden/objectives/objectives_small.npz: the REAL reference's plain and multitask pre-training wrappers (imported through
oracle/ref_import.py, CPU, eval mode) under the objective switches NETWORK.WITH_MLM_LOSS / WITH_MVRC_LOSS / MLM_LOSS_NORM_IN_BATCH_FIRST /
MVRC_LOSS_NORM_IN_BATCH_FIRST.  Run where the reference tree exists:

    python tools/make_objectives_golden.py

Dimensions of tests/golden/multitask_small.npz (hidden 128, 2 layers, V = 512, C = 50; B = 3, T = 10, R = 5, 2 text-only samples of 14).
The batch is synthetic.make_batch's with the labels re-dealt: 1, 0 and 3 MLM labels and 1, 3 and 0 valid regions per caption sample, so that
a per-sample mean is not the batch mean.
Per case and wrapper: the losses, the gradient norm, named_parameters() in order, a strided sample of each logits tensor.  Parameters
are oracle.init_params(pseed) minus the absent heads' keys, so none are stored.
The reference's multitask wrapper cannot run without the MLM loss (its forward reads mlm_loss_wvc, assigned only under WITH_MLM_LOSS:
resnet_vlbert_for_pretraining_multitask.py:205, 283); that combination is recorded as unavailable and its key list comes from the
constructor alone.
"""
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from oracle.vlbert_oracle import VLBertConfig, init_params  # noqa: E402
from tests.objectives_ref import Switches, absent  # noqa: E402

synthetic = importlib.import_module("vl-bert_amd.synthetic")

CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=512,
           max_position_embeddings=64, visual_region_classes=50)
B, T, R, AUX, SEED, PSEED, SAMPLE = 3, 10, 5, (2, 14), 31, 13, 2048
MLM_COUNTS, MVRC_COUNTS = (1, 0, 3), (1, 3, 0)
CASES = {
    "mlm_only": Switches(with_mvrc_loss=False),
    "mvrc_only": Switches(with_mlm_loss=False),
    "both_norm": Switches(mlm_norm_in_batch_first=True, mvrc_norm_in_batch_first=True),
    "mlm_only_norm": Switches(with_mvrc_loss=False, mlm_norm_in_batch_first=True),
    "mvrc_only_norm": Switches(with_mlm_loss=False, mvrc_norm_in_batch_first=True),
    "both": Switches(),          # the default objective on the same batch: what a norm switch has to move
}


def make_batch(cfg):
    """synthetic.make_batch's batch with the labels re-dealt so that the per-sample mean differs from the batch mean: the caption samples
    carry 1, 0 and 3 MLM labels and 1, 3 and 0 valid regions (a sample without a label and one without a valid region stay)."""
    batch = [t.clone() for t in synthetic.make_batch(B, T, R, vocab_size=cfg.vocab_size, region_classes=cfg.visual_region_classes,
                                                     seed=SEED, ragged=True)]
    boxes, text, lab, soft = batch[0], batch[2], batch[4], batch[6]
    g = torch.Generator().manual_seed(SEED + 1)
    lab[:] = -1
    soft[:] = 0.0
    for b, n in enumerate(MLM_COUNTS):
        pos = (text[b] > 0).nonzero().view(-1)[1:1 + n]          # behind [CLS]
        assert pos.numel() == n
        lab[b, pos] = torch.randint(1000 % cfg.vocab_size, cfg.vocab_size, (n,), generator=g)
    for b, n in enumerate(MVRC_COUNTS):
        real = (boxes[b, :, 0] > -1.5).nonzero().view(-1)[:n]
        assert real.numel() == n
        soft[b, real] = torch.softmax(2.0 * torch.randn(n, cfg.visual_region_classes, generator=g), -1)
    return batch


def sample(t):
    t = t.detach().double().reshape(-1)
    return t[::max(1, t.numel() // SAMPLE)][:SAMPLE].float().numpy()


def run(name, sw, multitask, out):
    RefModel, _ = ref_import.import_reference()
    if multitask:
        RefModel = ref_import.import_reference_multitask()
    cfg = VLBertConfig(multitask=multitask, **CFG)
    vocab_dir = ref_import.make_vocab_dir(os.path.join(tempfile.gettempdir(), "vlb_vocab_objectives"), cfg.vocab_size)
    rc = ref_import.make_reference_config(cfg, vocab_dir)
    rc.NETWORK.WITH_MLM_LOSS, rc.NETWORK.WITH_MVRC_LOSS = sw.with_mlm_loss, sw.with_mvrc_loss
    rc.NETWORK.MLM_LOSS_NORM_IN_BATCH_FIRST, rc.NETWORK.MVRC_LOSS_NORM_IN_BATCH_FIRST = sw.mlm_norm_in_batch_first, sw.mvrc_norm_in_batch_first
    torch.manual_seed(0)
    model = RefModel(rc)
    tag = "%s/%s/" % ("multitask" if multitask else "plain", name)
    out[tag + "keys"] = np.array([n for n, _ in model.named_parameters()])
    out[tag + "switches"] = np.array([sw.with_mlm_loss, sw.with_mvrc_loss, sw.mlm_norm_in_batch_first, sw.mvrc_norm_in_batch_first])
    ran = not (multitask and not sw.with_mlm_loss)
    out[tag + "ran"] = np.array(ran)
    if not ran:
        print("%s: the reference cannot run this combination; key list only" % tag)
        return
    sd = {k: v for k, v in init_params(cfg, seed=PSEED).items() if not absent(k, sw)}
    if sw.with_mlm_loss:
        sd["vlbert.mlm_head.predictions.decoder.weight"] = sd["vlbert.word_embeddings.weight"]
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    model.eval()
    batch = make_batch(cfg)
    aux = synthetic.make_aux_text(AUX[0], AUX[1], vocab_size=cfg.vocab_size, seed=SEED) if multitask else ()
    outputs, loss = model(None, *[t.clone() for t in batch], *[t.clone() for t in aux])
    model.zero_grad()
    loss.backward()
    total = sum(float((p.grad.double() ** 2).sum()) for _, p in model.named_parameters() if p.grad is not None)
    out[tag + "loss"], out[tag + "grad_norm"] = float(loss), total ** 0.5
    for k in (("mlm_loss_wvc", "mlm_loss_aux", "mvrc_loss") if multitask else ("mlm_loss", "mvrc_loss")):
        out[tag + k] = float(outputs[k])
    for k in (("mlm_logits_wvc", "mlm_logits_aux", "mvrc_logits") if multitask else ("mlm_logits", "mvrc_logits")):
        if outputs[k] is not None:
            out[tag + k + "_shape"], out[tag + k + "_smp"] = np.array(outputs[k].shape), sample(outputs[k])
        else:
            out[tag + k + "_shape"] = np.zeros(0, dtype=np.int64)
    print("%s loss %.6f grad_norm %.6f (%d parameters)" % (tag, float(loss), total ** 0.5, len(out[tag + "keys"])))


def main():
    cfg = VLBertConfig(multitask=True, **CFG)
    out = {"cfg_keys": np.array(list(CFG)), "cfg_vals": np.array([float(v) for v in CFG.values()]), "B": B, "T": T, "R": R,
           "aux_shape": np.array(AUX), "seed": SEED, "pseed": PSEED, "cases": np.array(list(CASES)),
           "key_lists": np.array("named_parameters() of the imported reference modules")}
    for k, t in zip(("boxes", "im_info", "text", "relationship_label", "mlm_labels", "mvrc_ops", "mvrc_labels"), make_batch(cfg)):
        out["in_" + k] = t.numpy()
    aux = synthetic.make_aux_text(AUX[0], AUX[1], vocab_size=cfg.vocab_size, seed=SEED)
    out["in_aux_text"], out["in_aux_mlm_labels"] = aux[0].numpy(), aux[1].numpy()
    for multitask in (False, True):
        for name, sw in CASES.items():
            run(name, sw, multitask, out)
    d = os.path.join(ROOT, "tests", "golden", "objectives")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "objectives_small.npz")
    np.savez_compressed(path, **out)
    print("-> %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
