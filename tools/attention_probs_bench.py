#!/usr/bin/env python
"""Timing of vlb_attention_probs (csrc/attention_probs.hip) with device events at the two shapes that matter -- B=8, 12 heads, S=n=512
(the longest maps) and B=64, 12 heads, S=n=101 (the pre-training sequence) -- next to the write rate a one-shot grid reaches on this
GPU (tools/hbm_stream_probe.hip, DESIGN.md "HBM-bound kernels").  The kernel is output-bound: bytes = B * heads * n * ldp * 4.
The output buffers rotate over more than the 256 MB Infinity Cache, so the stores go to HBM.  Information only; gates nothing."""
import argparse, importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module("vl-bert_amd.ops")
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=str, nargs="+", default=["8,512", "64,101"], help="B,S pairs (n = S, 12 heads)")
ap.add_argument("--p", type=float, nargs="+", default=[0.0, 0.1])
ap.add_argument("--iters", type=int, default=40)
a = ap.parse_args()
d = "cuda:0"
ONE_SHOT_WRITE_GBS = 6610.0      # one-shot grid fill, 16 B per lane (DESIGN.md "HBM-bound kernels", profiles/r04_hbm_stream_probe.txt)


def run(B, S, P):
    H, nh, n = 768, 12, S
    ldp = (n + 31) // 32 * 32
    qkv = torch.randn((B * S, 3 * H), device=d).to(ops.BF16)
    mask = torch.ones((B, S), device=d)
    ctx = torch.zeros((B * S, H), dtype=ops.BF16, device=d)
    lse = torch.zeros((B, nh, S), device=d)
    seed = torch.tensor([123], dtype=torch.int32, device=d)
    ops.attention_fwd(qkv, mask, ctx, lse, B, S, H, nh)
    nbytes = B * nh * n * ldp * 4
    outs = [torch.empty((B, nh, n, ldp), dtype=torch.float32, device=d) for _ in range(max(2, -(-(768 << 20) // nbytes)))]
    k = [0]

    def fn():
        ops.attention_probs(qkv, mask, lse, B, S, H, nh, n=n, drop_p=P, seed=seed, tag=1, out=outs[k[0] % len(outs)])
        k[0] += 1
    for _ in range(len(outs)):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / a.iters * 1e3
    gbs = nbytes / us / 1e3
    print("attention_probs B=%d heads=%d S=n=%d ldp=%d p=%.2f: %.1f us per call (launch gaps included), %.1f MB written, %.0f GB/s = %.2f of the "
          "one-shot-grid write rate (%.0f GB/s); %d rotating buffers" % (B, nh, S, ldp, P, us, nbytes / 1e6, gbs, gbs / ONE_SHOT_WRITE_GBS,
                                                                        ONE_SHOT_WRITE_GBS, len(outs)))


for s in a.shapes:
    B_, S_ = [int(x) for x in s.split(",")]
    for P_ in a.p:
        run(B_, S_, P_)
