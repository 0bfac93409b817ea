#!/usr/bin/env python
"""What the objective switches cost (NETWORK.WITH_MLM_LOSS / WITH_MVRC_LOSS / *_LOSS_NORM_IN_BATCH_FIRST; ends_16.Heads16).

(a) The row-weighted loss launches against the unweighted ones on the same tensors, at the headline sizes: MLM on 1024 compacted rows x
    30522 (vlb_ce_fwd_bwd_compact against vlb_ce_rowweight_fwd_bwd through sel_pos, and the per-sample weight kernel alone), MVRC on
    9216 rows x 1601 (vlb_soft_ce_fwd_bwd against vlb_soft_ce_rowweight_fwd_bwd, which holds the weight kernel).  The unweighted kernels
    are untouched by the switches, so they are the parent commit's.  The weighted row moves the same bytes plus one scalar load.
(b) The benched step (12 base layers, batch 256 x (64 + 36), dropout on, graph replay): the full objective against MLM only, MVRC only
    and both norm switches on, and a second default engine built last (the instance-to-instance difference inside one process).

Device events around synchronised windows, every shape warmed first, the variants alternating inside one process, median with min / max
over the rounds (the min-max of the unweighted variant is the run-to-run spread a difference has to exceed).
Usage: python tools/objectives_bench.py [--part a|b|ab] [--batch 256] [--layers 12]"""
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

    def logits(rows, ld):      # the 1/8 grid of [-8, 8]; every launch overwrites them with a (finite) gradient: restored per call below
        return torch.from_numpy((rng.randint(-64, 65, size=(rows, ld)) / 8.0).astype(np.float32)).to(ops.BF16).to(dev)

    # MLM: 256 samples x 64 positions, 1024 labelled rows (4 per sample), compacted in mlm_compact's order
    V, B, T, cap = 30522, 256, 64, 1024
    lab_full = np.full((B, T), -1, dtype=np.int64)
    for b in range(B):
        lab_full[b, rng.choice(T, 4, replace=False)] = rng.randint(0, V, 4)
    pos = np.flatnonzero(lab_full.reshape(-1) >= 0)
    assert pos.size == cap
    labels = torch.from_numpy(lab_full.reshape(-1)).to(dev)
    labels_c = torch.from_numpy(lab_full.reshape(-1)[pos]).to(dev)
    sel_pos = torch.from_numpy(pos.astype(np.int32)).to(dev)
    src, x = logits(cap, 30528), torch.empty((cap, 30528), dtype=ops.BF16, device=dev)
    counts, loss, w = torch.tensor([float(cap), 0.0], device=dev), zf(2), zf(B)
    restore = lambda: x.copy_(src)
    ops.sample_norm_weights(w, T, labels=labels, V=V)
    mlm = {
        "restore the logits (a copy; part of the two variants below)": restore,
        "vlb_ce_fwd_bwd_compact (unweighted)": lambda: (restore(), ops.ce_fwd_bwd_compact(x, V, labels_c, counts[0:1], counts[1:2], loss[0:1], loss[1:2])),
        "vlb_ce_rowweight_fwd_bwd through sel_pos": lambda: (restore(), ops.ce_rowweight_fwd_bwd(x, V, labels_c, w, T, loss[0:1], sel_pos=sel_pos)),
        "vlb_sample_norm_weights alone (256 x 64 labels)": lambda: ops.sample_norm_weights(w, T, labels=labels, V=V),
    }
    show("(a) MLM, %d compacted rows x 30528 (V = %d), %s" % (cap, V, ops.BF16), alternate(mlm, 20, 5))

    C, R = 1601, 36
    rows = 256 * R
    src2, x2 = logits(rows, 1608), torch.empty((rows, 1608), dtype=ops.BF16, device=dev)
    t = torch.from_numpy(rng.dirichlet(np.ones(C) * 0.2, rows).astype(np.float32)).to(dev)
    t[::7] = 0.0                                               # some invalid rows, as the masked regions leave them
    tsum, c2, w2 = zf(rows), zf(1), zf(256)
    restore2 = lambda: x2.copy_(src2)
    mvrc = {
        "restore the logits (a copy; part of the two variants below)": restore2,
        "vlb_soft_ce_fwd_bwd (unweighted)": lambda: (restore2(), ops.soft_ce_fwd_bwd(x2, C, t, tsum, c2, loss[0:1])),
        "vlb_soft_ce_rowweight_fwd_bwd (holds the weight kernel)": lambda: (restore2(), ops.soft_ce_rowweight_fwd_bwd(x2, C, t, tsum, w2, R, c2, loss[0:1])),
        "vlb_sample_norm_weights alone on tsum (256 x 36), the launch the weighted entry point adds": lambda: ops.sample_norm_weights(w2, R, tsum=tsum),
    }
    show("(a) MVRC, %d x 1608 (C = %d)" % (rows, C), alternate(mvrc, 50, 5))


def part_b(B, L):
    def build(**kw):
        eng = E.PretrainEngine(E.ModelConfig(num_hidden_layers=L, **kw), B, 64, 36, device="cuda:0", train=True, seed=7)
        eng.init_random(seed=1, visual_ln_init=1.0)
        eng.set_batch(*[t.cuda() for t in syn.make_batch(B, 64, 36, seed=2, ragged=True)])
        for _ in range(3):
            eng.train_step()
        torch.cuda.synchronize()
        return eng, eng.make_step_graph()

    engines = {"mlm + mvrc (the default step)": build(),
               "mlm only": build(with_mvrc_loss=False),
               "mvrc only": build(with_mlm_loss=False),
               "mlm + mvrc, both norm in batch first": build(mlm_norm_in_batch_first=True, mvrc_norm_in_batch_first=True),
               # the same default engine once more, built last: what another instance at other addresses costs or gains by itself
               "mlm + mvrc (the default step, a second engine built last)": build()}
    times = alternate({k: g for k, (e, g) in engines.items()}, 10, 5)
    show("(b) step, %d layers, batch %d x (64 + 36), graph replay, library %s" % (L, B, lib.LIB_PATH), times, unit="ms")
    for k, (e, g) in engines.items():
        print("   %s: %s" % (k, {n: round(v, 4) for n, v in e.loss_values().items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--layers", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("objectives_bench: no GPU visible (a timing needs the device)")
    print("objectives_bench: %s, %d rounds per variant, alternating" % (torch.cuda.get_device_name(0), ROUNDS))
    if "a" in args.part:
        part_a()
    if "b" in args.part:
        part_b(args.batch, args.layers)


if __name__ == "__main__":
    main()
