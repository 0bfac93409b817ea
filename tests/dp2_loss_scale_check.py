"""Dynamic loss scaling under data parallelism (test infrastructure; launched by tests/test_loss_scale_dp_gpu.py, never imported by the
package).  Two engine ranks share the one GPU over gloo.  An inf is put into rank 1's LOCAL gradient only, before the exchange:

  * the decision comes from the reduced gradient (all-reduce mode) or the all-reduced squared norm (sharded mode), so BOTH ranks must
    skip -- no extra communication --, with masters bit-unchanged and the same scaler state on both;
  * sharded mode, first step skipped: the compact 16-bit image a rank hands to the weight all-gather must still be the cast of its
    (unchanged) master slices -- nothing else has filled it before the first step that is really taken;
  * the next, real step updates the weights, gathers correct 16-bit copies, and leaves masters and scaler state identical across ranks.

Launch: python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P
        tests/dp2_loss_scale_check.py [--mode sharded|allreduce]"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import loss_scale_ref as R      # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def bits(t):
    return t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t.view(torch.int32)


def main():
    mode = arg("--mode", "sharded")
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    DEV = "cuda:0"
    torch.cuda.set_device(DEV)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    E = importlib.import_module("vl-bert_amd.engine")
    L = importlib.import_module("vl-bert_amd.loss_scale")
    syn = importlib.import_module("vl-bert_amd.synthetic")
    ops = importlib.import_module("vl-bert_amd.ops")
    B, T, Rg, S0 = 2, 16, 6, 1024.0
    eng = E.PretrainEngine(E.ModelConfig(num_hidden_layers=1), B, T, Rg, device=DEV, train=False, lr=1e-3, weight_decay=1e-2,
                           max_grad_norm=1.0, dp_mode=mode, loss_scale=L.DynamicLossScale(init_scale=S0, growth_interval=1000))
    bk = eng.buckets
    assert bk is not None and bk.world == world and bk.sharded == (mode == "sharded")
    print("rank %d: %s exchange, wire %s, collectives %s" % (rank, mode, "16-bit" if bk.wire_dtype is not None else "fp32",
                                                            "emulated" if bk.emulate else "native"), flush=True)
    eng.init_random(seed=3)
    eng.broadcast_parameters(src=0)
    eng.sync_weights()
    gemm = eng._gemm_weight_names()
    exp = np.array(eng.scaler.spec.initial_values(), dtype=np.float32)

    def check_w16(sd, when):
        eng.forward(False)                                  # (sharded: the weight gather lands under this forward)
        torch.cuda.synchronize()
        w16 = eng.P.named(eng.P.w16)
        for n in gemm:
            assert torch.equal(bits(w16[n]), bits(sd[n].to(ops.BF16))), "%s: 16-bit copy of %s is not the cast of the master" % (when, n)

    # ---- step 1: rank 1's local gradient carries one inf; both ranks must skip ------------------------------------------
    eng.set_batch(*[t.to(DEV) for t in syn.make_batch(B, T, Rg, seed=100 + rank, ragged=True)])
    eng.zero_grad()
    eng.forward(False)
    eng.backward(False)                                     # no exchange hooks: the gradient is still local
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.P.grad).all())
    if rank == 1:
        eng.P.grad[eng.P.offsets["vlbert.encoder.layer.0.output.dense.weight"] + 5] = float("inf")
    for k, _, _ in bk.buckets:
        bk.on_done(k)
    bk.wait()
    before = eng.P.master.clone()
    eng.optimizer_step()
    torch.cuda.synchronize()
    exp = R.update(exp, True)
    assert torch.equal(bits(eng.P.master), bits(before)), "rank %d: a skipped step moved the master weights" % rank
    assert float(eng.adam[5]) == 0.0 and not bool(eng.P.m.any()) and not bool(eng.P.v.any())
    assert eng.scaler.values() == exp.tolist(), (rank, eng.scaler_state())
    print("rank %d: step 1 skipped on an inf in rank 1's local gradient; scale %g" % (rank, eng.loss_scale), flush=True)
    sd = {n: t.clone() for n, t in eng.state_dict().items()}          # (sharded: gathers the master -- a collective)
    check_w16(sd, "after the skipped first step")

    # ---- step 2: a real step at the halved scale ----------------------------------------------------------------------------
    eng.zero_grad()
    eng.forward(False)
    eng.backward(False, on_layer_done=bk.on_done)
    bk.wait()
    eng.optimizer_step()
    torch.cuda.synchronize()
    exp = R.update(exp, False)
    assert eng.scaler.values() == exp.tolist() and float(eng.adam[5]) == 1.0
    sd2 = {n: t.clone() for n, t in eng.state_dict().items()}
    moved = max(float((sd2[n] - sd[n]).abs().max()) for n in gemm)
    assert bool(all(torch.isfinite(t).all() for t in sd2.values())) and moved > 0, moved
    check_w16(sd2, "after the first real step")

    # ---- replicas: masters and scaler state identical ----------------------------------------------------------------------
    flat = torch.cat([sd2[n].reshape(-1).float() for n in sorted(sd2)])
    other, sc_other = flat.clone(), eng.scaler.state.clone()
    dist.broadcast(other, src=0)
    dist.broadcast(sc_other, src=0)
    same = bool(torch.equal(bits(flat), bits(other))) and bool(torch.equal(sc_other, eng.scaler.state))
    print("rank %d: LOSS-SCALE DP OK=%s (%s, world %d): skipped 1, taken 1, scale %g, largest weight move %.3e" %
          (rank, same, mode, world, eng.loss_scale, moved), flush=True)
    assert same
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
