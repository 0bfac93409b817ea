"""Dynamic loss scaling on the fp16 build, with REAL overflow (-m gpu): nothing is injected.  One precision per process
(vl-bert_amd/_lib.py), so this file re-runs itself as a script in a child process with VLB_PRECISION=f16, like
tests/test_f16_build_gpu.py does with the engine suite.

The scale starts at 2^30.  The true-class d(logit) of the MLM loss is ~ -2^30 / n_labelled, far beyond fp16's 65504 for the few labelled
positions of a tiny batch; the 16-bit store is IEEE, so it becomes inf, reaches the decoder weight gradient and the squared norm.  The
first steps must therefore skip (weights bit-unchanged) while the scale halves, exactly, until the gradients fit; then training
proceeds.  The same sequence replayed through make_step_graph() must give the same scale history, step counts, schedule and scaler
state, bit for bit -- the skip decision, the scale and the schedule counter all live on the device -- and bit-unchanged weights through
its skipped steps.

Graph against eager, bit for bit: the engine's backward accumulates some gradients with float atomics (biases, LayerNorm parameters,
small embedding tables), so two eager runs of the SAME engine already differ in the last bits of those gradients, the clip
coefficient inherits the difference and every weight follows -- two whole trajectories cannot be compared bit for bit, whatever runs
them.  So every replay is checked against an eager SHADOW step from the same state: before a replay the engine's state (weights,
moments, Adam state, scaler, dropout seed) is copied into a second engine, which then runs zero_grad -> forward -> backward eagerly --
its d(logits) and every reproducible gradient must equal the replay's bit for bit --, takes the replay's gradient bits for the
rest, and runs optimizer_step() eagerly: weights, moments, 16-bit copies, Adam state (step count, lr), scaler state and dropout seed
must equal the replay's bit for bit, skipped steps and real ones alike.  The whole-trajectory distance to the independent eager run
is printed, not asserted."""
import importlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 32
INIT = 2.0 ** 30


def test_real_overflow_skips_halves_then_trains_eager_and_graph():
    env = dict(os.environ, VLB_PRECISION="f16")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "DYNAMIC LOSS SCALE ON THE FP16 BUILD OK" in r.stdout


def _child():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    E = importlib.import_module("vl-bert_amd.engine")
    L = importlib.import_module("vl-bert_amd.loss_scale")
    ops = importlib.import_module("vl-bert_amd.ops")
    syn = importlib.import_module("vl-bert_amd.synthetic")
    from tests import loss_scale_ref as R
    assert ops.BF16 == torch.float16, "the child must run the fp16 build"
    B, T, Rg = 2, 16, 6
    batch = [t.to("cuda:0") for t in syn.make_batch(B, T, Rg, seed=8, ragged=True)]

    def engine():
        eng = E.PretrainEngine(E.ModelConfig(num_hidden_layers=1), B, T, Rg, device="cuda:0", train=True, lr=1e-4, weight_decay=1e-2,
                               max_grad_norm=1.0, seed=5, lr_schedule="triangle", warmup_steps=4, t_total=100,
                               loss_scale=L.DynamicLossScale(init_scale=INIT, max_scale=INIT, growth_interval=1000))
        eng.init_random(seed=3)
        eng.set_batch(*batch)
        return eng

    def bits(t):
        return t.view(torch.int32)

    # ---- eager ----------------------------------------------------------------------------------------------------------
    eng = engine()
    w0 = eng.P.master.clone()
    hist, taken = [], []
    for i in range(STEPS):
        eng.train_step()
        torch.cuda.synchronize()
        st = eng.scaler_state()
        hist.append(st["scale"])
        taken.append(int(float(eng.adam[5])))
        if taken[-1] == 0:
            assert torch.equal(bits(eng.P.master), bits(w0)), "step %d was skipped but the weights moved" % (i + 1)
    skips = taken.count(0)
    print("eager: scale history %s" % ["2^%g" % np.log2(s) for s in hist])
    print("eager: %d skipped steps, then %d taken" % (skips, taken[-1]))
    assert skips >= 1 and taken[-1] >= 1, "expected real overflow at 2^30 and a recovery within %d steps" % STEPS
    # a run of exact halvings: the skipped steps form a prefix, each halves the scale, and the scale then stays (interval 1000)
    state = R.initial(init_scale=INIT, max_scale=INIT, growth_interval=1000)
    want = [float(s[0]) for s in R.run(state, [True] * skips + [False] * (STEPS - skips))]
    assert hist == want and want[skips - 1] == INIT / 2.0 ** skips, (hist, want)
    assert taken == [0] * skips + list(range(1, STEPS - skips + 1))
    assert st["skipped_total"] == skips and st["skipped_in_a_row"] == 0 and st["unskipped"] == STEPS - skips
    lv = eng.loss_values()
    assert all(np.isfinite(v) for v in lv.values()), lv
    assert bool(torch.isfinite(eng.P.master).all()) and not torch.equal(bits(eng.P.master), bits(w0))
    # the schedule counted the skipped steps, the bias correction did not
    k = STEPS                                                 # scheduler step of the last optimizer step = taken + skipped
    lr = float(np.float32(1e-4) * R.lr_lambda(2, k, 4, 100))
    assert abs(float(eng.adam[0]) - lr) <= 1e-6 * 1e-4, (float(eng.adam[0]), lr)
    print("eager: loss %.4f after %d real steps at scale 2^%g" % (lv["loss"], taken[-1], np.log2(hist[-1])))

    # ---- the same sequence through the replayed step graph, every replay against an eager shadow step ------------------------
    eng2, shadow = engine(), engine()
    eng2.train_step()                                         # (make_step_graph wants one eager step first)
    torch.cuda.synchronize()
    hist2 = [eng2.scaler_state()["scale"]]
    step = eng2.make_step_graph()
    # reproducible gradients: the Linear weights of the encoder layers and the heads.  The two Linear weights of the front end are not:
    # the tied word-embedding table also takes the embedding backward's atomic scatter, and the obj_downsample weight gradient is
    # computed from d(obj_reps), which that backward sums with atomics (it rarely differs: a 16-bit rounding has to flip)
    exact = set(eng2._gemm_weight_names()) - {"vlbert.word_embeddings.weight", "image_feature_extractor.obj_downsample.1.weight"}

    def bits16(t):
        return t.view(torch.int16)

    def carried(e):
        return [e.P.master, e.P.m, e.P.v, e.adam, e.scaler.state, e.seed]

    for i in range(1, STEPS):
        for dst, src in zip(carried(shadow), carried(eng2)):
            dst.copy_(src)
        shadow._weights_dirty = True
        step()
        shadow.zero_grad(); shadow.forward(True); shadow.backward(True)
        torch.cuda.synchronize()
        for a, b in ((eng2.mlm_logits, shadow.mlm_logits), (eng2.mvrc_logits, shadow.mvrc_logits)):
            assert torch.equal(bits16(a), bits16(b)), "replay %d: d(logits) differ from the eager step's" % i
        for (n, a), b in zip(eng2.g32.items(), shadow.g32.values()):
            if n in exact:
                assert torch.equal(bits(a), bits(b)), "replay %d: gradient of %s differs from the eager step's" % (i, n)
        shadow.P.grad.copy_(eng2.P.grad)                      # the atomically accumulated tensors: the replay's bits
        shadow.optimizer_step()
        torch.cuda.synchronize()
        for name, a, b in zip(("master", "m", "v", "adam", "scaler", "seed"), carried(eng2), carried(shadow)):
            assert torch.equal(a, b) and (a.dtype != torch.float32 or torch.equal(bits(a), bits(b))), "replay %d: %s differs" % (i, name)
        assert torch.equal(bits16(eng2.P.w16), bits16(shadow.P.w16)), "replay %d: the 16-bit weights differ" % i
        hist2.append(eng2.scaler_state()["scale"])
        if float(eng2.adam[5]) == 0.0:
            assert torch.equal(bits(eng2.P.master), bits(w0)), "replay %d was skipped but the weights moved" % i
    print("graph: %d graph segment(s), %d host call(s); scale history equal: %s" % (step.n_graphs, step.n_calls, hist2 == hist))
    assert step.n_graphs == 1 and step.n_calls == 0          # one rank: a single graph, no new host call
    # against the independent eager run: everything that does not depend on the gradient's last bits
    assert hist2 == hist, (hist2, hist)
    assert eng2.scaler.values() == eng.scaler.values() and torch.equal(eng2.adam, eng.adam) and torch.equal(eng2.seed, eng.seed)
    diff = float((eng2.P.master - eng.P.master).abs().max())
    ratio = float((eng2.P.master.double() - eng.P.master.double()).norm() / (eng.P.master.double() - w0.double()).norm())
    print("graph vs the independent eager run after %d real steps (not asserted): max |diff| %.3e, |diff| / |moved| %.3e" % (taken[-1], diff, ratio))
    print("DYNAMIC LOSS SCALE ON THE FP16 BUILD OK: %d skipped, %d taken, every replay equals its eager shadow step" % (skips, taken[-1]))


if __name__ == "__main__":
    _child()
