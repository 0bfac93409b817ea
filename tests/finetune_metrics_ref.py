"""numpy restatement of the fine-tuning evaluation kernels (vl-bert_amd/csrc/finetune_metrics.hip), shared by
tests/test_finetune_metrics_cpu.py (against the reference's own metric classes through
tests/golden/metrics/finetune_metrics_small.npz) and tests/test_finetune_metrics_gpu.py (against the kernels, on the same fp32
logits).  Rules restated: columns >= C are padding and ignored; argmax as torch.argmax (np.argmax has the same rules: equal maxima ->
the lowest column, NaN is the largest value and the first NaN wins, a row of -inf -> column 0); mode 1 filters label == -1 only;
mode 2's sum is a sequential float64 loop over the rows; mode 3 is a strict > 0.5; the binary metrics truncate the label toward zero."""
import numpy as np

PREDICT, HARD, GATHER, GATHER_GT = 0, 1, 2, 3


def argmax_ref(logits, C):
    return np.argmax(np.asarray(logits, dtype=np.float32)[:, :C], axis=1).astype(np.int64)


def argmax_eval_ref(logits, C, mode, label=None, sum0=0, count0=0):
    """-> dict(pred [rows], score [rows] fp32 (None in mode 0), sum, count): sum / count continue from sum0 / count0 (mode 2: sum is a
    Python float = the float64 accumulator, added row by row)."""
    pred = argmax_ref(logits, C)
    rows = len(pred)
    if mode == PREDICT:
        return dict(pred=pred, score=None, sum=sum0, count=count0)
    if mode == HARD:
        label = np.asarray(label).astype(np.int64)
        score = (pred == label).astype(np.float32)
        return dict(pred=pred, score=score, sum=int(sum0) + int(score.sum()), count=int(count0) + int((label != -1).sum()))
    g = np.asarray(label, dtype=np.float32)[np.arange(rows), pred]
    if mode == GATHER:
        s = float(sum0)
        for r in range(rows):
            s += float(g[r])
        return dict(pred=pred, score=g, sum=s, count=int(count0) + rows)
    score = (g > np.float32(0.5)).astype(np.float32)
    return dict(pred=pred, score=score, sum=int(sum0) + int(score.sum()), count=int(count0) + rows)


def softmax_ref(logits, C):
    """float64 softmax of the fp32 logits' first C columns (rows holding NaN, or only -inf, come out NaN as in torch)."""
    x = np.asarray(logits, dtype=np.float32)[:, :C].astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)


def binary_cls_ref(logits, label, N):
    """-> [correct among lab >= 0, #(lab >= 0), correct among lab == 1, #(lab == 1)] (refcoco_metrics.py:36-72)."""
    x = np.asarray(logits, dtype=np.float32)[:, :N]
    lab = np.trunc(np.asarray(label, dtype=np.float32)[:, :N]).astype(np.int64)      # .long(): toward zero
    with np.errstate(invalid="ignore"):
        pred = (x > 0).astype(np.int64)                                                # NaN > 0 is False
    keep, pos = lab >= 0, lab == 1
    return [int((pred[keep] == lab[keep]).sum()), int(keep.sum()), int((pred[pos] == lab[pos]).sum()), int(pos.sum())]


def joint_hits_ref(pred_a, label_a, pred_r, label_r):
    pred_a, label_a, pred_r, label_r = (np.asarray(t).astype(np.int64) for t in (pred_a, label_a, pred_r, label_r))
    return [int(((pred_a == label_a) & (pred_r == label_r)).sum()), len(pred_a)]


def fp32_div(num, den):
    """sum_metric / num_inst as the reference divides them: two fp32 tensors."""
    return float(np.float32(num) / np.float32(den)) if den else float("nan")
