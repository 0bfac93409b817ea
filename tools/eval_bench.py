#!/usr/bin/env python
"""Validation step at the headline dimensions (12 x 768, V = 30522, batch 256, 64 text + 36 regions, MLM compaction on):
PretrainEngine.eval_step() against what validation cost before it existed -- forward(train=False) (the fused forward+backward
losses) on an engine that keeps a copy of the logits, plus the torch argmax / compare over that copy -- and the loss tails alone on
the same logits.  Usage: python tools/eval_bench.py [batch]"""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
E = importlib.import_module("vl-bert_amd.engine")
ops = importlib.import_module("vl-bert_amd.ops")
syn = importlib.import_module("vl-bert_amd.synthetic")
from tools.clock_probe import sclk_sysfs  # noqa: E402


def timed(fn, n=10):
    """us per call between two stream events (the helper of tools/ld_pad_probe.py)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    B, T, R = (int(sys.argv[1]) if len(sys.argv) > 1 else 256), 64, 36
    batch = [t.cuda() for t in syn.make_batch(B, T, R, seed=1)]
    res = {}
    for keep in (False, True):
        eng = E.PretrainEngine(E.ModelConfig(), B, T, R, device="cuda:0", train=True, keep_logits=keep)
        eng.init_random(seed=0)
        eng.set_batch(*batch)
        V, C = eng.cfg.vocab_size, eng.cfg.visual_region_classes
        if not keep:
            res["eval_step()"] = timed(eng.eval_step)
            cap, cnt = eng.mlm_cap, eng.counts
            saved = eng.mlm_logits[:cap].clone()
            res["  tail: vlb_ce_eval, %d compacted rows" % cap] = timed(lambda: ops.ce_eval(
                eng.mlm_logits[:cap], V, eng.labels_c, eng.losses[0:1], eng.metric_acc[0], count0=cnt[0:1], count1=cnt[2:3],
                loss_out1=eng.losses[2:3], acc1=eng.metric_acc[1]))
            res["  tail: vlb_soft_ce_eval, %d rows" % eng.BR] = timed(lambda: ops.soft_ce_eval(
                eng.mvrc_logits, C, eng.in_mvrc_labels.view(eng.BR, C), eng.losses[1:2], eng.metric_acc[2]))
            res["  tail: vlb_ce_fwd_bwd_compact (logits re-used: gradients of gradients, same traffic)"] = timed(lambda: ops.ce_fwd_bwd_compact(
                eng.mlm_logits[:cap], V, eng.labels_c, cnt[0:1], cnt[2:3], eng.losses[0:1], eng.losses[2:3]))
            eng.mlm_logits[:cap].copy_(saved)
            res["  tail: vlb_soft_ce_fwd_bwd"] = timed(lambda: ops.soft_ce_fwd_bwd(
                eng.mvrc_logits, C, eng.in_mvrc_labels.view(eng.BR, C), eng.mvrc_tsum, cnt[1:2], eng.losses[1:2]))
            res["forward(train=False), compaction on (no logits kept: cannot give an accuracy)"] = timed(lambda: eng.forward(train=False))
        else:
            lab = eng.in_mlm_labels.view(-1)
            tgt = eng.in_mvrc_labels.view(eng.BR, C)

            def old():
                eng.forward(train=False)
                pm = eng.mlm_logits_copy[:, :V].argmax(1)
                keep_rows = lab >= 0
                hits = ((pm == lab) & keep_rows).sum()
                pv = eng.mvrc_logits_copy[:, :C].argmax(1)
                valid = (tgt.sum(1) - 1.0).abs() < 0.1
                return hits, keep_rows.sum(), ((pv == tgt.argmax(1)) & valid).sum(), valid.sum()
            res["forward(train=False) with kept logits + torch argmax / compare"] = timed(old)
        del eng
        torch.cuda.empty_cache()
    print("eval_bench: batch %d, sclk %s MHz" % (B, sclk_sysfs()))
    for k, v in res.items():
        print("%10.1f us  %s" % (v, k))


if __name__ == "__main__":
    main()
