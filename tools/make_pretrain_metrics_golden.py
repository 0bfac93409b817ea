"""Generate tests/golden/metrics/pretrain_metrics_small.npz by running the REAL reference metric classes
(common/metrics/pretrain_metrics.py + composite_eval_metric.py) on CPU.  Runs only where the reference tree exists:

    python tools/make_pretrain_metrics_golden.py

Two configurations in the order pretrain/function/train.py:244-273 builds them -- "plain" (ResNetVLBERTForPretraining with
WITH_REL_LOSS, the default TRAIN.LOSS_LOGGERS) and "multi" (ResNetVLBERTForPretrainingMultitask, the LOSS_LOGGERS of the shipped
multitask YAMLs) -- are fed three small `outputs` dicts each.  The logits lie on the 1/8 grid of [-8, 8] (exact in bfloat16 and in
IEEE fp16) with planted ties of the row maximum; the soft labels hold ties, an all-zero row and a row summing to 1.2; the aux labels
of "multi" are all -1, so MLMAccAUX stays empty (nan).  The losses in the dicts are the true ones (F.cross_entropy(ignore_index=-1),
the reference's soft_cross_entropy).  Stored: the inputs, per-batch [hits, counted rows] as the reference's own sum_metric / num_inst
moved, the per-batch losses, and the composite's names and values.  Data only.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests.metrics_ref import grid_logits  # noqa: E402

V, C, T, R = 37, 11, 6, 4
MULTI_LOGGERS = [("mlm_loss_wvc", "MLMLossWVC"), ("mlm_loss_aux", "MLMLossAUX"), ("mvrc_loss", "MVRCLoss")]


def mlm_pair(rng, B, labelled=0.4):
    logits = grid_logits(rng, (B, T, V))
    label = np.where(rng.rand(B, T) < labelled, rng.randint(0, V, (B, T)), -1).astype(np.int64)
    if labelled > 0:
        label[0, 0], label[0, 1] = 5, 20
        logits[0, 0, 5] = logits[0, 0, 30] = 8.0          # tie, label on the FIRST occurrence: a hit
        logits[0, 1, 3] = logits[0, 1, 20] = 8.0          # tie, label on the second: a miss
    return logits, label


def mvrc_pair(rng, B):
    logits = grid_logits(rng, (B, R, C))
    label = rng.dirichlet(np.ones(C) * 0.3, (B, R)).astype(np.float32)
    label[0, 0] = 0.0                                      # invalid: sum 0
    label[0, 1] *= 1.2                                     # invalid: sum 1.2
    label[0, 2] = 0.0
    label[0, 2, [2, 7]] = 0.5                              # tie in the target: argmax = 2
    logits[0, 2, 2] = logits[0, 2, 9] = 8.0                # and in the logits: argmax = 2 -> hit
    return logits, label


def main():
    ref_import.install_stubs()
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from common.metrics import pretrain_metrics as PM
    from common.metrics.composite_eval_metric import CompositeEvalMetric
    from common.utils.misc import soft_cross_entropy
    rng = np.random.RandomState(17)
    store = {}
    for case in ("plain", "multi"):
        multi = case == "multi"
        ms = ([PM.MLMAccuracyWVC(), PM.MLMAccuracyAUX()] if multi else [PM.RelationshipAccuracy(), PM.MLMAccuracy()]) + [PM.MVRCAccuracy()]
        loggers = MULTI_LOGGERS if multi else [("relationship_loss", "RelLoss"), ("mlm_loss", "MLMLoss"), ("mvrc_loss", "MVRCLoss")]
        ms += [PM.LossLogger(o, display_name=d) for o, d in loggers]
        comp = CompositeEvalMetric()
        for m in ms:
            comp.add(m)
        rows = {"RelAcc": 3, "MLMAcc": 0, "MLMAccWVC": 0, "MLMAccAUX": 1, "MVRCAccuracy": 2}
        counts, losses = [], []
        for b, B in enumerate((3, 2, 3)):
            out = {}
            mvl, mvt = mvrc_pair(rng, B)
            out["mvrc_logits"], out["mvrc_label"] = torch.from_numpy(mvl), torch.from_numpy(mvt)
            out["mvrc_loss"] = soft_cross_entropy(out["mvrc_logits"].view(-1, C), out["mvrc_label"].view(-1, C))
            if multi:
                for sfx, frac in (("wvc", 0.4), ("aux", 0.0)):
                    lg, lb = mlm_pair(rng, B, frac)
                    out["mlm_logits_" + sfx], out["mlm_label_" + sfx] = torch.from_numpy(lg), torch.from_numpy(lb)
                    out["mlm_loss_" + sfx] = (F.cross_entropy(out["mlm_logits_" + sfx].view(-1, V), out["mlm_label_" + sfx].view(-1), ignore_index=-1)
                                              if frac > 0 else torch.zeros(()))
                out["relationship_loss"] = torch.zeros(())
            else:
                lg, lb = mlm_pair(rng, B)
                out["mlm_logits"], out["mlm_label"] = torch.from_numpy(lg), torch.from_numpy(lb)
                out["mlm_loss"] = F.cross_entropy(out["mlm_logits"].view(-1, V), out["mlm_label"].view(-1), ignore_index=-1)
                rl = grid_logits(rng, (B, 2))
                rl[0] = 1.5                                # tie -> argmax 0
                out["relationship_logits"] = torch.from_numpy(rl)
                out["relationship_label"] = torch.from_numpy(rng.randint(0, 2, (B,)).astype(np.int64))
                out["relationship_loss"] = F.cross_entropy(out["relationship_logits"], out["relationship_label"])
            before = {m.name: (float(m.sum_metric), float(m.num_inst)) for m in ms}
            comp.update(out)
            c = np.zeros((4, 2), dtype=np.int64)
            for m in ms:
                if m.name in rows:
                    c[rows[m.name]] = (float(m.sum_metric) - before[m.name][0], float(m.num_inst) - before[m.name][1])
            counts.append(c)
            # engine.losses layout: mlm (wvc), mvrc, mlm aux, relationship
            losses.append([float(out["mlm_loss_wvc" if multi else "mlm_loss"]), float(out["mvrc_loss"]),
                           float(out["mlm_loss_aux"]) if multi else 0.0, float(out["relationship_loss"])])
            for k, v in out.items():
                if v.dim() > 0:
                    store["%s_b%d_%s" % (case, b, k)] = v.numpy()
        names, values = comp.get()
        store[case + "_names"] = np.array(names)
        store[case + "_values"] = np.array(values, dtype=np.float64)
        store[case + "_counts"] = np.stack(counts)
        store[case + "_losses"] = np.array(losses, dtype=np.float32)
        store[case + "_loggers"] = np.array([",".join(p) for p in loggers])
        print(case, list(zip(names, values)))
    path = os.path.join(ROOT, "tests", "golden", "metrics", "pretrain_metrics_small.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, V=V, C=C, **store)
    print("-> %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
