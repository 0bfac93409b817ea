"""numpy restatement of the validation kernels (vl-bert_amd/csrc/metrics.hip), shared by tests/test_metrics_cpu.py (against the
reference's own metric classes through tests/golden/metrics/pretrain_metrics_small.npz) and tests/test_metrics_gpu.py (against the
kernels, on the same 16-bit logits).  Rules restated: columns >= V are padding and ignored; an argmax tie goes to the LOWEST column
(np.argmax, like torch.argmax); hard labels outside [0, V) are not counted; a soft-label row counts iff |sum(target) - 1| < 0.1.
Losses are taken in float64."""
import numpy as np


def _lse(x):
    m = x.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def ce_eval_ref(logits, V, labels):
    """logits [rows, >= V] (any float dtype), labels [rows] int -> dict(loss = mean CE over the counted rows (nan if none),
    hits, n, pred = argmax per row, -1 where the row is not counted)."""
    x = np.asarray(logits, dtype=np.float64)[:, :V]
    labels = np.asarray(labels).astype(np.int64)
    keep = (labels >= 0) & (labels < V)
    pred = np.full(labels.shape, -1, dtype=np.int64)
    if not keep.any():
        return dict(loss=float("nan"), hits=0, n=0, pred=pred)
    xk, lk = x[keep], labels[keep]
    am = xk.argmax(axis=1)
    pred[keep] = am
    loss = (_lse(xk) - xk[np.arange(len(lk)), lk]).mean()
    return dict(loss=float(loss), hits=int((am == lk).sum()), n=int(keep.sum()), pred=pred)


def soft_ce_eval_ref(logits, C, target):
    """logits [rows, >= C], target [rows, >= C] -> dict(loss = mean over the valid rows of -sum_c log_softmax(x)_c t_c, hits, n, valid)."""
    x = np.asarray(logits, dtype=np.float64)[:, :C]
    t32 = np.asarray(target, dtype=np.float32)[:, :C]
    valid = np.abs(t32.sum(axis=1, dtype=np.float32) - np.float32(1.0)) < np.float32(0.1)
    if not valid.any():
        return dict(loss=float("nan"), hits=0, n=0, valid=valid)
    xv, tv = x[valid], t32[valid].astype(np.float64)
    loss = (_lse(xv) * tv.sum(axis=1) - (tv * xv).sum(axis=1)).mean()
    hits = int((xv.argmax(axis=1) == t32[valid].argmax(axis=1)).sum())
    return dict(loss=float(loss), hits=hits, n=int(valid.sum()), valid=valid)


def grid_logits(rng, shape, lo=-8.0, hi=8.0):
    """Random logits on the 1/8 grid of [lo, hi]: exactly representable in bfloat16 and in IEEE fp16."""
    return (rng.randint(int(lo * 8), int(hi * 8) + 1, size=shape) / 8.0).astype(np.float32)
