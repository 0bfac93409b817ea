"""Fine-tuning evaluation over the module mirrors: the validation loops of {vqa,vcr,refcoco}/function/val.py, test-time prediction
with the argmax / softmax taken on the device (vlb_argmax_eval mode 0), and the result-file tails of vqa/function/test.py:74-81,
vcr/function/test.py:118-146 and refcoco/function/test.py:20-33,86-100 as host functions that take the ids from the caller (the
dataset classes are not built).  The writers use json / csv / numpy only -- no pandas at run time -- and are pinned byte for byte to
files the reference's own json / pandas calls wrote (tests/golden/metrics/)."""
import csv
import json
import os

import numpy as np
import torch

from .. import ops


def _to_cuda(batch):
    """common/trainer.py to_cuda: tensors of the batch onto the current GPU (None entries and GPU tensors pass through)"""
    if not torch.cuda.is_available():
        return list(batch)
    return [b.cuda(non_blocking=True) if (torch.is_tensor(b) and not b.is_cuda) else b for b in batch]


def _split(batch, label_index_in_batch):
    """the label by index (a negative index counts from the end, as in the reference), the rest in order"""
    batch = _to_cuda(batch)
    skip = label_index_in_batch % len(batch)
    return batch[label_index_in_batch], [batch[i] for i in range(len(batch)) if i != skip]


@torch.no_grad()
def do_validation(net, val_loader, metrics, label_index_in_batch):
    """{vqa,vcr,refcoco}/function/val.py:6-18.  No host synchronisation of its own: the metrics keep their counters on the device
    until get()."""
    net.eval()
    metrics.reset()
    for batch in val_loader:
        label, datas = _split(batch, label_index_in_batch)
        outputs = net(*datas)
        outputs.update({"label": label})
        metrics.update(outputs)


@torch.no_grad()
def joint_validation(answer_net, rationale_net, answer_val_loader, rationale_val_loader, metrics, label_index_in_batch):
    """vcr/function/val.py:21-55: Q->A and QA->R nets side by side; the outputs of each under an `answer_` / `rationale_` prefix, plus
    `answer_pred` / `rationale_pred` (int32, vlb_argmax_eval mode 0) for vcr_metrics.JointAccuracy."""
    answer_net.eval()
    rationale_net.eval()
    metrics.reset()
    for a_batch, r_batch in zip(answer_val_loader, rationale_val_loader):
        a_label, a_datas = _split(a_batch, label_index_in_batch)
        r_label, r_datas = _split(r_batch, label_index_in_batch)
        a_outputs = answer_net(*a_datas)
        r_outputs = rationale_net(*r_datas)
        outputs = {"answer_" + k: v for k, v in a_outputs.items()}
        outputs.update({"rationale_" + k: v for k, v in r_outputs.items()})
        outputs.update({"answer_label": a_label, "rationale_label": r_label})
        for which in ("answer", "rationale"):
            logits = outputs[which + "_label_logits"]
            if torch.is_tensor(logits) and logits.is_cuda and logits.dim() == 2:
                pred = torch.empty((logits.shape[0],), dtype=torch.int32, device=logits.device)
                ops.argmax_eval(logits.float(), ops.ARGMAX_PREDICT, pred=pred)
                outputs[which + "_pred"] = pred
        metrics.update(outputs)


@torch.no_grad()
def predict(net, loader, task):
    """The prediction loops of the three test.py files without their dataset bookkeeping: every batch of `loader` is the argument list
    of the net's inference_forward.  task "vqa" -> answer ids int64 [N] (label_logits.argmax(1)); "vcr" -> probabilities fp32 [N, C]
    (F.softmax(label_logits.float(), 1)); "refcoco" -> pred_boxes fp32 [N, 4].  Argmax and softmax run on the device; the results of
    all batches are copied to the host once, at the end."""
    if task not in ("vqa", "vcr", "refcoco"):
        raise ValueError("predict: task %r (vqa, vcr, refcoco)" % (task,))
    net.eval()
    parts = []
    for batch in loader:
        outputs = net(*_to_cuda(batch))
        if task == "refcoco":
            parts.append(outputs["pred_boxes"].detach().float())
            continue
        logits = outputs["label_logits"].detach().float()
        rows, C = logits.shape
        if task == "vqa":
            pred = torch.empty((rows,), dtype=torch.int32, device=logits.device)
            ops.argmax_eval(logits, ops.ARGMAX_PREDICT, pred=pred)
            parts.append(pred)
        else:
            probs = torch.empty((rows, C), dtype=torch.float32, device=logits.device)
            ops.argmax_eval(logits, ops.ARGMAX_PREDICT, probs=probs)
            parts.append(probs)
    if not parts:
        return np.zeros((0,), dtype=np.int64 if task == "vqa" else np.float32)
    out = torch.cat(parts, 0).cpu().numpy()
    return out.astype(np.int64) if task == "vqa" else out


# ---- result files ----------------------------------------------------------------------------------------------------------
def _plain(v):
    return v.item() if hasattr(v, "item") else v


def write_vqa_result(path, question_ids, answer_ids, answer_vocab):
    """vqa/function/test.py:74-81: [{'question_id', 'answer'}, ...] with answer = answer_vocab[answer id]."""
    result = [{"question_id": _plain(q), "answer": answer_vocab[int(a)]} for q, a in zip(question_ids, answer_ids)]
    with open(path, "w") as f:
        json.dump(result, f)
    return path


def _float_text(v):
    """One cell as DataFrame.to_csv writes it: the shortest text that reads back to the same value of the column's own type."""
    return str(v)


def vcr_columns(task):
    if task == "Q2A":
        return ["answer_{}".format(i) for i in range(4)]
    if task == "QA2R":
        return ["rationale_conditioned_on_a{}_{}".format(i, j) for i in range(4) for j in range(4)]
    raise ValueError("Not Support Task {}".format(task))


def write_vcr_result(csv_path, npy_path, annot_ids, probs, task):
    """vcr/function/test.py:118-134: np.save of the probabilities, then the csv of DataFrame(probs, columns).set_index('annot_id')
    -- `annot_id` first, then answer_i (Q2A, 4 columns) or rationale_conditioned_on_a{i}_{j} (QA2R, 16 columns)."""
    probs = np.asarray(probs)
    columns = vcr_columns(task)
    if probs.ndim != 2 or probs.shape[1] != len(columns) or len(annot_ids) != probs.shape[0]:
        raise ValueError("write_vcr_result: probs %s for %d ids and %d %s columns" % (probs.shape, len(annot_ids), len(columns), task))
    np.save(npy_path, probs)
    with open(csv_path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["annot_id"] + columns)
        for a, row in zip(annot_ids, probs):
            w.writerow([_plain(a)] + [_float_text(v) for v in row])
    return csv_path


def _read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def _typed_columns(header, rows):
    """What pd.read_csv followed by to_csv does to the text of a column: all integers -> integers, all numbers -> float64 written by
    repr, anything else -> the text itself."""
    out = [list(r) for r in rows]
    for c in range(len(header)):
        cells = [r[c] for r in rows]
        for conv, fmt in ((int, str), (float, repr)):
            try:
                vals = [conv(x) for x in cells]
            except ValueError:
                continue
            for r, v in zip(out, vals):
                r[c] = fmt(v)
            break
    return out


def merge_vcr_results(q2a_csv, qa2r_csv, out_csv):
    """vcr/function/test.py:137-146 (merge_result): inner join of the two result files on annot_id in the left file's order,
    written without an index column."""
    lh, lrows = _read_csv(q2a_csv)
    rh, rrows = _read_csv(qa2r_csv)
    lrows, rrows = _typed_columns(lh, lrows), _typed_columns(rh, rrows)
    lk, rk = lh.index("annot_id"), rh.index("annot_id")
    right = {}
    for r in rrows:
        right.setdefault(r[rk], []).append([v for i, v in enumerate(r) if i != rk])
    output_dir = os.path.dirname(out_csv)
    if output_dir and not os.path.exists(output_dir):
        os.makedirs(output_dir)
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(lh + [h for i, h in enumerate(rh) if i != rk])
        for l in lrows:
            for r in right.get(l[lk], ()):
                w.writerow(l + r)
    return out_csv


def write_refcoco_result(path, ref_ids, pred_boxes):
    """refcoco/function/test.py:83-90: [{'ref_id', 'box': [x1, y1, x2, y2]}, ...]"""
    boxes = pred_boxes.detach().cpu().tolist() if torch.is_tensor(pred_boxes) else np.asarray(pred_boxes).tolist()
    result = [{"ref_id": _plain(r), "box": b} for r, b in zip(ref_ids, boxes)]
    with open(path, "w") as f:
        json.dump(result, f)
    return path


POSITIVE_THRESHOLD = 0.5


def calculate_iou(pred_boxes, gt_boxes):
    """refcoco/function/test.py:20-33: IoU of xyxy boxes in the inclusive-pixel (+1) convention"""
    x11, y11, x12, y12 = pred_boxes[:, 0], pred_boxes[:, 1], pred_boxes[:, 2], pred_boxes[:, 3]
    x21, y21, x22, y22 = gt_boxes[:, 0], gt_boxes[:, 1], gt_boxes[:, 2], gt_boxes[:, 3]
    xA, yA = np.maximum(x11, x21), np.maximum(y11, y21)
    xB, yB = np.minimum(x12, x22), np.minimum(y12, y22)
    inter = (xB - xA + 1).clip(0) * (yB - yA + 1).clip(0)
    area_a = (x12 - x11 + 1) * (y12 - y11 + 1)
    area_b = (x22 - x21 + 1) * (y22 - y21 + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area_a + area_b - inter)


def refcoco_accuracy(pred_boxes, gt_xywh):
    """refcoco/function/test.py:93-98: ground truth as the dataset's (x, y, w, h) -> xyxy by adding the corner, a prediction counts at
    IoU >= 0.5."""
    pred = np.array(pred_boxes, dtype=np.float64)
    gt = np.array(gt_xywh, dtype=np.float64)
    gt[:, [2, 3]] += gt[:, [0, 1]]
    iou = calculate_iou(pred, gt)
    return float((iou >= POSITIVE_THRESHOLD).sum() * 1.0 / iou.shape[0])
