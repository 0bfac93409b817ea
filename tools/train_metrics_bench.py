#!/usr/bin/env python
"""What the training-time metrics cost (PretrainEngine(train_metrics=True); the ACC forms of the fused loss kernels).

(a) The loss launches alone at the headline sizes -- MLM on the compaction capacity of batch 256 x 64 tokens (3328 rows x 30528),
    MVRC 9216 x 1608, relationship 256 x 8 -- in three variants: the existing entry point; the `_acc` entry point; and the existing
    entry point with a kept copy of the logits followed by vlb_ce_eval / vlb_soft_ce_eval on that copy, the only way to get the
    counters without the ACC forms (the compacted MLM launch keeps no copy, so that variant runs the one-group launch).
(b) The headline step: 12 base layers, batch 256 x (64 + 36), dropout on, graph replay, with train_metrics off and on.
    `--off-only` times the off engine alone and uses nothing newer than the engine's constructor: copied into a checkout of the
    parent commit (with that commit's library built), it times the launches this change leaves alone.

Device events around synchronised windows, every shape warmed first, the variants alternating inside one process, median with
min / max over the rounds; repeat the whole command for the run-to-run spread.  The sustained shader clock is bench.py's in-kernel probe.
Usage: python tools/train_metrics_bench.py [--part a|b|ab] [--off-only] [--batch 256] [--layers 12]"""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
E = importlib.import_module("vl-bert_amd.engine")
ops = importlib.import_module("vl-bert_amd.ops")
lib = importlib.import_module("vl-bert_amd._lib")
syn = importlib.import_module("vl-bert_amd.synthetic")

ROUNDS = 7


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, iters, warm):
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(window_ms(fn, iters))
    return times


def show(title, times, unit="us"):
    scale = 1000.0 if unit == "us" else 1.0
    print(title)
    for k, t in times.items():
        print("   %10.2f %s  (min %.2f, max %.2f over %d rounds)  %s" % (statistics.median(t) * scale, unit, min(t) * scale, max(t) * scale, len(t), k))


def part_a():
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    zf = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    zi = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)

    def logits(rows, ld):      # the 1/8 grid of [-8, 8]; every launch overwrites them with a (finite) gradient: restored per call below
        return torch.from_numpy((rng.randint(-64, 65, size=(rows, ld)) / 8.0).astype(np.float32)).to(ops.BF16).to(dev)

    # MLM: the compaction capacity of 256 x 64 text positions, every row labelled (the worst case for the loss kernels)
    V, cap = 30522, 3328
    src, x, cp = logits(cap, 30528), torch.empty((cap, 30528), dtype=ops.BF16, device=dev), torch.empty((cap, 30528), dtype=ops.BF16, device=dev)
    lab = torch.from_numpy(rng.randint(0, V, cap).astype(np.int64)).to(dev)
    counts, loss, acc = torch.tensor([cap - 700.0, 700.0, 0.0], device=dev), zf(2), zi(2, 2)

    def restore():
        x.copy_(src)

    mlm = {
        "restore the logits (a copy; part of every variant below)": restore,
        "vlb_ce_fwd_bwd_compact": lambda: (restore(), ops.ce_fwd_bwd_compact(x, V, lab, counts[0:1], counts[1:2], loss[0:1], loss[1:2])),
        "vlb_ce_fwd_bwd_compact, acc given": lambda: (restore(), ops.ce_fwd_bwd_compact(x, V, lab, counts[0:1], counts[1:2], loss[0:1], loss[1:2],
                                                                                 acc=acc[0], acc1=acc[1])),
        "vlb_ce_fwd_bwd + kept copy, then vlb_ce_eval on it": lambda: (restore(), ops.ce_fwd_bwd(x, V, lab, counts[2:3], loss[0:1], logits_copy=cp),
                                                                        ops.ce_eval(cp, V, lab, loss[1:2], acc[0])),
    }
    show("(a) MLM, %d x 30528 (V = %d), %s" % (cap, V, ops.BF16), alternate(mlm, 20, 5))

    C, rows = 1601, 9216
    src2, x2, cp2 = logits(rows, 1608), torch.empty((rows, 1608), dtype=ops.BF16, device=dev), torch.empty((rows, 1608), dtype=ops.BF16, device=dev)
    t = torch.from_numpy(rng.dirichlet(np.ones(C) * 0.2, rows).astype(np.float32)).to(dev)
    t[::7] = 0.0                                               # some invalid rows, as the masked regions leave them
    tsum, c2 = zf(rows), zf(1)
    restore2 = lambda: x2.copy_(src2)
    mvrc = {
        "restore the logits (a copy; part of every variant below)": restore2,
        "vlb_soft_ce_fwd_bwd": lambda: (restore2(), ops.soft_ce_fwd_bwd(x2, C, t, tsum, c2, loss[0:1])),
        "vlb_soft_ce_fwd_bwd, acc given": lambda: (restore2(), ops.soft_ce_fwd_bwd(x2, C, t, tsum, c2, loss[0:1], acc=acc[0])),
        "vlb_soft_ce_fwd_bwd + kept copy, then vlb_soft_ce_eval on it": lambda: (restore2(), ops.soft_ce_fwd_bwd(x2, C, t, tsum, c2, loss[0:1], logits_copy=cp2),
                                                                                  ops.soft_ce_eval(cp2, C, t, loss[1:2], acc[0])),
    }
    show("(a) MVRC, %d x 1608 (C = %d)" % (rows, C), alternate(mvrc, 50, 5))

    src3, x3, cp3 = logits(256, 8), torch.empty((256, 8), dtype=ops.BF16, device=dev), torch.empty((256, 8), dtype=ops.BF16, device=dev)
    lab3 = torch.from_numpy(rng.randint(0, 2, 256).astype(np.int64)).to(dev)
    restore3 = lambda: x3.copy_(src3)
    rel = {
        "restore the logits (a copy; part of every variant below)": restore3,
        "vlb_ce_fwd_bwd": lambda: (restore3(), ops.ce_fwd_bwd(x3, 2, lab3, c2, loss[0:1])),
        "vlb_ce_fwd_bwd, acc given": lambda: (restore3(), ops.ce_fwd_bwd(x3, 2, lab3, c2, loss[0:1], acc=acc[0])),
        "vlb_ce_fwd_bwd + kept copy, then vlb_ce_eval on it": lambda: (restore3(), ops.ce_fwd_bwd(x3, 2, lab3, c2, loss[0:1], logits_copy=cp3),
                                                                        ops.ce_eval(cp3, 2, lab3, loss[1:2], acc[0])),
    }
    show("(a) relationship, 256 x 8 (V = 2)", alternate(rel, 200, 10))


def part_b(B, L, off_only):
    def build(**kw):
        eng = E.PretrainEngine(E.ModelConfig(num_hidden_layers=L), B, 64, 36, device="cuda:0", train=True, seed=7, **kw)
        eng.init_random(seed=1, visual_ln_init=1.0)
        eng.set_batch(*[t.cuda() for t in syn.make_batch(B, 64, 36, seed=2, ragged=True)])
        for _ in range(3):
            eng.train_step()
        torch.cuda.synchronize()
        return eng, eng.make_step_graph()

    engines = {"train_metrics off": build()}
    if not off_only:
        engines["train_metrics on"] = build(train_metrics=True)
    times = alternate({k: g for k, (e, g) in engines.items()}, 10, 5)
    show("(b) step, %d layers, batch %d x (64 + 36), graph replay, library %s" % (L, B, lib.LIB_PATH), times, unit="ms")
    for k, (e, g) in engines.items():
        on = getattr(e, "train_metrics", False)      # (getattr: --off-only also runs inside an older checkout)
        print("   %s: loss %.4f%s" % (k, e.loss_values()["loss"], ("  counters %s" % e.train_metric_counts()) if on else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--layers", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("train_metrics_bench: no GPU visible (a timing needs the device)")
    print("train_metrics_bench: %s, %d rounds per variant, alternating" % (torch.cuda.get_device_name(0), ROUNDS))
    if "b" in args.part:
        part_b(args.batch, args.layers, args.off_only)
    if "a" in args.part and not args.off_only:
        part_a()
    if ops.BF16 == torch.bfloat16:
        import bench
        print("sustained shader clock (bench.sustained_clock_mhz): %s MHz" % bench.sustained_clock_mhz(ops, lib, torch.device("cuda:0")))


if __name__ == "__main__":
    main()
