#!/usr/bin/env python
"""One pre-training train_step() at the north-star per-GPU shape (cfgs/pretrain/base_prec_withouttextonly_4x16G_fp32.yaml: 12 base
layers, 64 samples of 64 tokens + 36 regions, V = 30522, C = 1601, dropout on) with the fp32 encoder: the hybrid
(`encoder_fp32=True`: 16-bit front end, heads and losses) and `fp32_full` (everything fp32), in one process.
Both engines are built and warmed first; then ROUNDS rounds alternate them, each timing STEPS steps between two stream events.
Prints the median step time of each with its min / max over the rounds.
Usage: python tools/fp32_full_bench.py [batch] [layers]"""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
E = importlib.import_module("vl-bert_amd.engine")
syn = importlib.import_module("vl-bert_amd.synthetic")

WARM, ROUNDS, STEPS = 3, 5, 4


def build(B, L, **kw):
    eng = E.PretrainEngine(E.ModelConfig(num_hidden_layers=L), B, 64, 36, device="cuda:0", train=True, seed=7, encoder_fp32=True,
                           dp_mode="allreduce", **kw)
    eng.init_random(seed=1, visual_ln_init=1.0)
    eng.set_batch(*[t.cuda() for t in syn.make_batch(B, 64, 36, seed=2, ragged=True)])
    for _ in range(WARM):
        eng.train_step()
    torch.cuda.synchronize()
    return eng


def window_ms(eng):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        eng.train_step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    engines = {"hybrid (encoder_fp32)": build(B, L), "fp32_full": build(B, L, fp32_full=True)}
    times = {k: [] for k in engines}
    for _ in range(ROUNDS):
        for k, eng in engines.items():
            times[k].append(window_ms(eng))
    print("fp32_full_bench: %d layers, batch %d x (64 + 36), dropout on, %s build; %d rounds of %d steps, alternating" %
          (L, B, "fp16" if importlib.import_module("vl-bert_amd.ops").BF16 == torch.float16 else "bf16", ROUNDS, STEPS))
    for k, t in times.items():
        lv = engines[k].loss_values()
        print("%10.2f ms per step  (min %.2f, max %.2f)  %-24s loss %.4f" % (statistics.median(t), min(t), max(t), k, lv["loss"]))


if __name__ == "__main__":
    main()
