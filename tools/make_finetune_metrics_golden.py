"""Generate tests/golden/metrics/finetune_metrics_small.npz and the small result files beside it by running the REAL reference
metric classes (common/metrics/{vqa,vcr,refcoco}_metrics.py + composite_eval_metric.py) on CPU and the json / pandas calls of the
reference's test.py tails.  Runs only where the reference tree and pandas exist:

    python tools/make_finetune_metrics_golden.py

Three cases -- "vqa" (SoftAcc + a LossLogger), "vcr" (Acc, AnsLoss, CNNRegLoss, PosFraction, a LossLogger, a LossLogger of an output
the module does not produce, JointAcc) and "refcoco" (RefAcc, ClsAcc, ClsPosAcc, ClsPosFrac, a LossLogger) -- are fed three small
seeded `outputs` dicts each.  The logits lie on the 1/8 grid of [-8, 8] with planted ties of the row maximum; the VQA scores come from
{0, 0.3, 0.6, 0.9, 1}; the VCR labels hold -1 and one label >= C; the RefCOCO+ labels hold -1 padding, -0.5, 0.7 and a gathered 0.5,
the logits zeros and a NaN.  Stored: the inputs, every metric's sum_metric / num_inst after every update, and the composite's names
and values.  The result files: a VQA json, the VCR Q2A / QA2R csv + npy and their merge, a RefCOCO+ json, with their inputs in the
npz.  Data only.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests.metrics_ref import grid_logits  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metrics")
BATCHES = (3, 2, 3)
A, C, R = 37, 4, 9


def vqa_outputs(rng, B):
    logits = grid_logits(rng, (B, A))
    label = np.zeros((B, A), np.float32)
    for b in range(B):
        cols = rng.choice(A, 5, replace=False)
        label[b, cols] = np.array([1.0, 0.9, 0.6, 0.3, 0.3], np.float32)
        logits[b, cols[rng.randint(0, 5)]] = 7.5              # the argmax lands on a scored answer more often than chance
    logits[0] = np.minimum(logits[0], 7.0)
    logits[0, [4, 30]] = 8.0                                  # tie: the lowest column wins
    label[0, 4], label[0, 30] = 0.6, 1.0
    lg, lb = torch.from_numpy(logits), torch.from_numpy(label)
    return {"label_logits": lg, "label": lb, "ans_loss": F.binary_cross_entropy_with_logits(lg, lb) * A}


def vcr_outputs(rng, B, b):
    out = {}
    for pre in ("", "answer_", "rationale_"):
        logits = grid_logits(rng, (B, C))
        label = rng.randint(0, C, (B,)).astype(np.int64)
        logits[0, [1, 3]] = 8.0                               # tie -> 1
        label[0] = 1 if pre != "rationale_" else 3
        if pre == "":
            label[1] = -1                                     # filtered
            if B > 2:
                label[2] = C + 1                              # counted, a miss
        out[pre + "label_logits"], out[pre + "label"] = torch.from_numpy(logits), torch.from_numpy(label)
    lg = out["label_logits"]
    onehot = torch.zeros_like(lg).scatter_(1, out["label"].clamp(min=0, max=C - 1).view(-1, 1), 1.0)
    out["ans_loss"] = F.binary_cross_entropy_with_logits(lg, onehot, reduction="none").mean(1)
    out["positive_fraction"] = torch.full((), 1.0 / C)
    if b != 1:                                                # the middle batch has no CNN regularisation loss
        out["cnn_regularization_loss"] = torch.tensor(float(rng.rand()) + 0.5)
    return out


def refcoco_outputs(rng, B):
    logits = grid_logits(rng, (B, R))
    label = (rng.rand(B, R) < 0.3).astype(np.float32)
    label[:, R - 2:] = -1.0                                   # padding
    logits[:, R - 2:] = -8.0
    label[0, 2], label[0, 3] = 0.7, -0.5                      # .long() -> 0, 0: both valid
    logits[0, 4], logits[0, 5] = 0.0, np.nan                  # pred 0, 0 (and the NaN wins the argmax)
    label[0, 5] = 1.0
    logits[1] = np.minimum(logits[1], 7.0)
    logits[1, 6] = 8.0
    label[1, 6] = 0.5                                         # the gathered label is exactly 0.5: a miss
    lg, lb = torch.from_numpy(logits), torch.from_numpy(label)
    keep = lb >= 0
    return {"label_logits": lg, "label": lb,
            "cls_loss": F.binary_cross_entropy_with_logits(torch.nan_to_num(lg)[keep], (lb[keep] > 0.5).float())}


def run_case(store, case, metrics, make):
    from common.metrics.composite_eval_metric import CompositeEvalMetric
    comp = CompositeEvalMetric()
    for m in metrics:
        comp.add(m)
    rng = np.random.RandomState({"vqa": 21, "vcr": 22, "refcoco": 23}[case])
    sums, insts = [], []
    for b, B in enumerate(BATCHES):
        out = make(rng, B, b)
        comp.update(out)
        sums.append([float(m.sum_metric) for m in metrics])
        insts.append([float(m.num_inst) for m in metrics])
        for k, v in out.items():
            store["%s_b%d_%s" % (case, b, k)] = v.numpy()
    names, values = comp.get()
    store[case + "_names"] = np.array(names)
    store[case + "_values"] = np.array(values, dtype=np.float64)
    store[case + "_sum_metric"] = np.array(sums, dtype=np.float64)          # [batch, metric], after the update
    store[case + "_num_inst"] = np.array(insts, dtype=np.float64)
    print(case, list(zip(names, values)))


def result_files(store):
    import pandas as pd
    rng = np.random.RandomState(31)
    # vqa/function/test.py:74-81
    vocab = ["yes", "no", "2", "white", "on the table", "café", "a \"quoted\" one"]
    q_ids = [int(q) for q in rng.randint(1, 10 ** 6, 6)]
    a_ids = [int(a) for a in rng.randint(0, len(vocab), 6)]
    result = [{'question_id': q_id, 'answer': vocab[a_id]} for q_id, a_id in zip(q_ids, a_ids)]
    with open(os.path.join(OUT, "vqa_result.json"), "w") as f:
        json.dump(result, f)
    store["vqa_question_ids"], store["vqa_answer_ids"], store["vqa_answer_vocab"] = np.array(q_ids), np.array(a_ids), np.array(vocab)
    # vcr/function/test.py:118-134, per task
    for task, n, width in (("Q2A", 5, 4), ("QA2R", 4, 16)):
        logits = torch.from_numpy((rng.randn(n, width) * 3).astype(np.float32))
        logits[0, 0], logits[0, 1] = 14.0, -9.0                              # probabilities near 1 and around 1e-10
        test_probs = np.concatenate([F.softmax(logits[:, k:k + 4].float(), dim=1).float().numpy() for k in range(0, width, 4)], axis=1)
        ids = ["test-%d" % i for i in range(5)]
        test_ids = np.concatenate([ids[:2], ids[2:n]], axis=0) if task == "Q2A" else np.array([ids[3], ids[0], ids[4], ids[1]])
        np.save(os.path.join(OUT, "vcr_result_%s.npy" % task), test_probs)
        if task == 'Q2A':
            columns = ['answer_{}'.format(i) for i in range(4)]
        else:
            columns = ['rationale_conditioned_on_a{}_{}'.format(i, j) for i in range(4) for j in range(4)]
        dataframe = pd.DataFrame(data=test_probs, columns=columns)
        dataframe['annot_id'] = test_ids
        dataframe = dataframe.set_index('annot_id', drop=True)
        dataframe.to_csv(os.path.join(OUT, "vcr_result_%s.csv" % task))
        store["vcr_%s_probs" % task], store["vcr_%s_annot_ids" % task] = test_probs, np.array(test_ids)
    # merge_result (:137-146)
    left_df = pd.read_csv(os.path.join(OUT, "vcr_result_Q2A.csv"))
    right_df = pd.read_csv(os.path.join(OUT, "vcr_result_QA2R.csv"))
    pd.merge(left_df, right_df, on='annot_id').to_csv(os.path.join(OUT, "vcr_result_merged.csv"), index=False)
    # refcoco/function/test.py:83-90
    ref_ids = [int(r) for r in rng.randint(1, 50000, 4)]
    boxes = torch.from_numpy((rng.rand(4, 4) * 300).astype(np.float32))
    pred_boxes = []
    pred_boxes.extend(boxes.detach().cpu().tolist())
    result = [{'ref_id': ref_id, 'box': box} for ref_id, box in zip(ref_ids, pred_boxes)]
    with open(os.path.join(OUT, "refcoco_result.json"), "w") as f:
        json.dump(result, f)
    store["refcoco_ref_ids"], store["refcoco_pred_boxes"] = np.array(ref_ids), boxes.numpy()


def main():
    ref_import.install_stubs()
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from common.metrics import refcoco_metrics as RM
    from common.metrics import vcr_metrics as CM
    from common.metrics import vqa_metrics as QM
    os.makedirs(OUT, exist_ok=True)
    store = {}
    run_case(store, "vqa", [QM.SoftAccuracy(), QM.LossLogger("ans_loss", display_name="AnsLoss")], lambda rng, B, b: vqa_outputs(rng, B))
    run_case(store, "vcr", [CM.Accuracy(), CM.AnsLoss(), CM.CNNRegLoss(), CM.PositiveFraction(), CM.LossLogger("ans_loss", display_name="AnsLossLog"),
                            CM.LossLogger("no_such_loss"), CM.JointAccuracy()], vcr_outputs)
    run_case(store, "refcoco", [RM.RefAccuracy(), RM.ClsAccuracy(), RM.ClsPosAccuracy(), RM.ClsPosFraction(),
                                RM.LossLogger("cls_loss", display_name="ClsLoss")], lambda rng, B, b: refcoco_outputs(rng, B))
    result_files(store)
    path = os.path.join(OUT, "finetune_metrics_small.npz")
    np.savez_compressed(path, A=A, C=C, R=R, **store)
    print("-> %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
