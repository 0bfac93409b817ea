"""Host restatement of the training-time counters (PretrainEngine(train_metrics=True).train_metric_acc), shared by
tests/test_train_metrics_gpu.py (on logits cloned from the engine before the fused loss kernels overwrite them) and
tests/test_train_metrics_cpu.py (against torch.argmax on the reference fixture's logits).  The rules are those of tests/metrics_ref.py:
`counts_ref` only routes every head to ce_eval_ref / soft_ce_eval_ref and keeps [hits, counted rows]."""
import numpy as np

from tests import metrics_ref as MR

ROWS = ("mlm", "mlm_aux", "mvrc", "relationship")      # PretrainEngine.METRIC_ROWS


def counts_ref(heads, V, C):
    """heads: {row name: (logits [rows, >= width], hard labels [rows] or soft targets [rows, >= C])} -> {row name: (hits, n)} for all
    four rows ((0, 0) for a head that is not given).  Widths: V for the two MLM rows, C for mvrc, 2 for relationship."""
    out = {k: (0, 0) for k in ROWS}
    for k, (logits, labels) in heads.items():
        if k == "mvrc":
            r = MR.soft_ce_eval_ref(logits, C, labels)
        else:
            r = MR.ce_eval_ref(logits, 2 if k == "relationship" else V, labels)
        out[k] = (r["hits"], r["n"])
    return out


def engine_heads(eng, mlm_logits, mvrc_logits, rel_logits=None):
    """The heads of one forward as counts_ref takes them, from logits CLONED before the losses ran (any float dtype, the engine's
    padded layout) and the engine's own label buffers.  With labelled-row compaction the MLM rows are the compacted ones: group 0 =
    the first counts[0] rows, group 1 = the labelled rows behind them."""
    V, C, nw = eng.cfg.vocab_size, eng.cfg.visual_region_classes, eng.B * eng.T
    f = lambda t: t.float().cpu().numpy()
    heads = {}
    if eng._mlm_compact_now:
        lab = eng.labels_c.cpu().numpy()
        lg = f(mlm_logits[:eng.mlm_cap])
        n0 = int(eng.counts[0])
        assert int(eng.counts[2]) == int((lab >= 0).sum()) - n0
        rows = np.arange(len(lab))
        heads["mlm"] = (lg[rows < n0], lab[rows < n0])
        heads["mlm_aux"] = (lg[rows >= n0], lab[rows >= n0])
    else:
        lab = eng.in_mlm_labels.view(-1).cpu().numpy()
        lg = f(mlm_logits[:eng.BT])
        heads["mlm"] = (lg[:nw], lab[:nw])
        if eng.Ba:
            heads["mlm_aux"] = (lg[nw:], lab[nw:])
    heads["mvrc"] = (f(mvrc_logits), eng.in_mvrc_labels.view(eng.BR, C).cpu().numpy())
    if eng.cfg.with_rel_loss:
        heads["relationship"] = (f(rel_logits), eng.in_rel_label.cpu().numpy())
    return heads
