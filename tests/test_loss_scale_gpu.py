"""Dynamic loss scaling on the device (-m gpu, default build): the scaler forms of the optimizer kernels, the device-scale forms of the
loss kernels, the engine's skipped / halved / grown steps against a twin static engine, and the fused optimizers.

Scales are powers of two throughout, so "the dynamic step at scale S" and "the static step given the host product" are the SAME
arithmetic: every comparison between the two is bit for bit, except where the engine itself is not reproducible from one run to the
next (sums accumulated with float atomics: a loss value, the small gradient tensors) -- those carry their reordering bound."""
import numpy as np
import pytest
import torch

from oracle import vlbert_oracle as O
from tests import loss_scale_ref as R
from tests.gpu_util import dev, pkg

pytestmark = pytest.mark.gpu
S0 = 1024.0      # 2^10


def make_scaler(**kw):
    L = pkg("loss_scale")
    kw.setdefault("init_scale", S0)
    return L.LossScaler(L.DynamicLossScale(**kw), dev())


def ref_state(s):
    return np.array(s.spec.initial_values(), dtype=np.float32)


def same_bits(a, b):
    if a.dtype in (torch.bfloat16, torch.float16):
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def adam_state(step=3.0, max_norm=1.0):
    return torch.tensor([1e-3, 0.9, 0.999, 1e-6, 1e-2, step, max_norm, 0.0], dtype=torch.float32, device=dev())


def rand_pgmv(n, seed, gdtype):
    g0 = torch.Generator().manual_seed(seed)
    p, g, m = (torch.randn(n, generator=g0) for _ in range(3))
    v = torch.rand(n, generator=g0) * 0.1
    g = (g * 3).to(gdtype)
    gs = (g.float() * S0).to(gdtype)      # the loss-scaled gradient: exact in either type
    assert torch.equal(gs.float(), g.float() * S0)
    return [t.to(dev()) for t in (p, gs, m, v)]


# ------------------------------------------------------------------------------------------------ 1. optimizer kernels
@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("n", [1, 2047, 2051, 4099])
def test_flat_adamw_with_scaler(n, g16):
    ops = pkg("ops")
    gdtype = ops.BF16 if g16 else torch.float32
    ws = torch.zeros(2048, device=dev())
    gscale = 0.5
    for max_norm in (1.0, 0.0):
        p, g, m, v = rand_pgmv(n, 100 + n, gdtype)
        # finite gradient: the bits of the existing entry point given grad_scale / 2^10
        pa, ma, va, sa = p.clone(), m.clone(), v.clone(), adam_state(max_norm=max_norm)
        p16a = torch.zeros(n, dtype=ops.BF16, device=dev())
        ops.sumsq_det(g, ws, sa[7:8])
        ops.adamw_step(pa, g, ma, va, p16a, sa, grad_scale=gscale / S0)
        pb, mb, vb, sb = p.clone(), m.clone(), v.clone(), adam_state(max_norm=max_norm)
        p16b = torch.zeros(n, dtype=ops.BF16, device=dev())
        sc = make_scaler(growth_interval=2)
        ops.sumsq_det(g, ws, sb[7:8])
        ops.adamw_step(pb, g, mb, vb, p16b, sb, grad_scale=gscale, scaler=sc.state)
        torch.cuda.synchronize()
        assert not same_bits(pa, p)
        assert same_bits(pa, pb) and same_bits(ma, mb) and same_bits(va, vb) and same_bits(p16a, p16b)
        assert float(sa[5]) == 4.0 and float(sb[5]) == 4.0 and float(sb[7]) == 0.0
        exp = R.update(ref_state(sc), False)
        assert sc.values() == exp.tolist()
        # a second clean step reaches the interval: the scale grows
        ops.sumsq_det(g, ws, sb[7:8])
        ops.adamw_step(pb, g, mb, vb, p16b, sb, grad_scale=gscale, scaler=sc.state)
        exp = R.update(exp, False)
        assert sc.values() == exp.tolist() and exp[0] == 2 * S0 and float(sb[5]) == 5.0
    # one inf / NaN anywhere (tail elements included): nothing moves, the scale halves
    for bad in (float("inf"), float("nan")):
        for pos in sorted({0, n // 2, n - 1}):
            p, g, m, v = rand_pgmv(n, 200 + n, gdtype)
            g[pos] = bad
            st, sc = adam_state(), make_scaler()
            p16 = torch.full((n,), 7.0, dtype=ops.BF16, device=dev())
            keep = [t.clone() for t in (p, m, v, p16)]
            ops.sumsq_det(g, ws, st[7:8])
            ops.adamw_step(p, g, m, v, p16, st, grad_scale=gscale, scaler=sc.state)
            torch.cuda.synchronize()
            for t, k in zip((p, m, v, p16), keep):
                assert same_bits(t, k), (bad, pos)
            assert float(st[5]) == 3.0 and float(st[7]) == 0.0
            exp = R.update(ref_state(sc), True)
            assert sc.values() == exp.tolist() and sc.read()["scale"] == S0 / 2 and sc.read()["skipped_in_a_row"] == 1


def test_a_finite_gradient_whose_squared_norm_overflows_is_skipped_too():
    ops = pkg("ops")
    n = 2051
    p, g, m, v = rand_pgmv(n, 7, torch.float32)
    g[5] = 2.0e19 * 1.0                                     # finite, its square is not (fp32)
    st, sc = adam_state(), make_scaler()
    keep = p.clone()
    ops.sumsq_det(g, torch.zeros(2048, device=dev()), st[7:8])
    ops.adamw_step(p, g, m, v, None, st, scaler=sc.state)
    assert same_bits(p, keep) and sc.read()["skipped_total"] == 1


@pytest.mark.parametrize("g16", [False, True])
def test_ranges_adamw_with_scaler(g16):
    """The sharded optimizer's kernel over a table whose last range is ragged; on a skipped step the compact 16-bit image is still
    written, as the cast of the unchanged master."""
    ops = pkg("ops")
    gdtype = ops.BF16 if g16 else torch.float32
    rows = [(64, 0, 5000), (8000, 5000, 1028), (12000, 6028, 1027)]
    N, NC = 13100, 7055
    tbl = ops.ShardRanges(rows, dev())
    assert tbl.total_blocks > len(rows)                     # more than one block per range somewhere
    ws = torch.zeros(2048, device=dev())
    owned = torch.zeros(N, dtype=torch.bool)
    for p0, g0, ln in rows:
        owned[p0:p0 + ln] = True

    def fresh(seed):
        p, _, m, v = rand_pgmv(N, seed, torch.float32)
        _, g, _, _ = rand_pgmv(NC, seed + 1, gdtype)
        return p, g, m, v

    p, g, m, v = fresh(31)
    pa, ma, va, sa = p.clone(), m.clone(), v.clone(), adam_state()
    ca = torch.zeros(NC, dtype=ops.BF16, device=dev())
    tbl.sumsq(g, ws, sa[7:8])
    tbl.adamw(pa, g, ma, va, ca, sa, grad_scale=0.5 / S0)
    pb, mb, vb, sb, sc = p.clone(), m.clone(), v.clone(), adam_state(), make_scaler()
    cb = torch.zeros(NC, dtype=ops.BF16, device=dev())
    tbl.sumsq(g, ws, sb[7:8])
    tbl.adamw(pb, g, mb, vb, cb, sb, grad_scale=0.5, scaler=sc.state)
    torch.cuda.synchronize()
    assert same_bits(pa, pb) and same_bits(ma, mb) and same_bits(va, vb) and same_bits(ca, cb) and float(sb[5]) == 4.0
    assert same_bits(pb.cpu()[~owned], p.cpu()[~owned]) and not same_bits(pb, p)
    assert sc.values() == R.update(ref_state(sc), False).tolist()
    for bad, pos in ((float("inf"), 0), (float("nan"), NC - 1), (float("inf"), 5003)):
        p, g, m, v = fresh(41)
        g[pos] = bad
        st, sc = adam_state(), make_scaler()
        c = torch.full((NC,), 7.0, dtype=ops.BF16, device=dev())
        keep = [t.clone() for t in (p, m, v)]
        tbl.sumsq(g, ws, st[7:8])
        tbl.adamw(p, g, m, v, c, st, grad_scale=0.5, scaler=sc.state)
        torch.cuda.synchronize()
        for t, k in zip((p, m, v), keep):
            assert same_bits(t, k), (bad, pos)
        for p0, g0, ln in rows:                             # the compact image = cast of the (unchanged) master
            assert same_bits(c[g0:g0 + ln], p[p0:p0 + ln].to(ops.BF16)), (bad, pos, p0)
        assert float(st[5]) == 3.0 and float(st[7]) == 0.0
        assert sc.values() == R.update(ref_state(sc), True).tolist() and sc.read()["scale"] == S0 / 2


@pytest.mark.parametrize("n", [1, 2051, 4099])
def test_sgd_momentum_with_scaler(n):
    ops = pkg("ops")
    p, g, buf, _ = rand_pgmv(n, 300 + n, torch.float32)
    ss = torch.zeros(1, device=dev())
    ops.sumsq(g, ss)
    pa, ba = p.clone(), buf.clone()
    p16a, p16b = (torch.zeros(n, dtype=ops.BF16, device=dev()) for _ in range(2))
    ops.sgd_momentum_step(pa, g, ba, 0.05, 0.9, 1e-2, p16=p16a, sumsq=ss, max_norm=1.0, grad_scale=0.5 / S0)
    pb, bb, sc = p.clone(), buf.clone(), make_scaler()
    ops.sgd_momentum_step(pb, g, bb, 0.05, 0.9, 1e-2, p16=p16b, sumsq=ss, max_norm=1.0, grad_scale=0.5, scaler=sc.state)
    torch.cuda.synchronize()
    assert same_bits(pa, pb) and same_bits(ba, bb) and same_bits(p16a, p16b) and not same_bits(pb, p)
    assert sc.values() == R.update(ref_state(sc), False).tolist()
    g[n - 1] = float("nan")
    ss.zero_()
    ops.sumsq(g, ss)
    keep = [pb.clone(), bb.clone(), p16b.clone()]
    ops.sgd_momentum_step(pb, g, bb, 0.05, 0.9, 1e-2, p16=p16b, sumsq=ss, max_norm=0.0, grad_scale=0.5, scaler=sc.state)
    torch.cuda.synchronize()
    assert all(same_bits(t, k) for t, k in zip((pb, bb, p16b), keep))
    assert sc.values() == R.update(R.update(ref_state(sc), False), True).tolist()
    with pytest.raises(RuntimeError, match="squared gradient norm is required"):
        ops.sgd_momentum_step(pb, g, bb, 0.05, scaler=sc.state)


def test_lr_schedule_counts_the_skipped_steps():
    ops = pkg("ops")
    st, sc = adam_state(step=2.0), make_scaler()
    sc.state[5] = 3.0                                       # skipped_total
    for kind, warm, total in ((ops.LR_WARMUP_LINEAR, 8, 20), (ops.LR_WARMUP_LINEAR, 3, 20), (ops.LR_WARMUP_CONSTANT, 8, 0), (ops.LR_CONSTANT, 0, 0)):
        ops.lr_schedule_step(st, kind, 2e-4, warm, total, scaler=sc.state)
        want = np.float32(2e-4) * R.lr_lambda(kind, 2 + 3 + 1, warm, total)
        assert abs(float(st[0]) - float(want)) <= 1e-6 * 2e-4, (kind, float(st[0]), want)
        ops.lr_schedule_step(st, kind, 2e-4, warm, total)   # the plain form: steps taken only
        assert abs(float(st[0]) - float(np.float32(2e-4) * R.lr_lambda(kind, 3, warm, total))) <= 1e-6 * 2e-4


# ------------------------------------------------------------------------------------------------ 2. loss kernels
@pytest.mark.parametrize("k", [0, 10, 16])
def test_loss_kernels_device_scale_equals_host_product(k):
    ops = pkg("ops")
    ds = torch.tensor([2.0 ** k], device=dev())
    gen = torch.Generator().manual_seed(70 + k)

    def logits(rows, V, ld, fill):
        buf = torch.full((rows, ld), fill, dtype=ops.BF16, device=dev())
        buf[:, :V] = (torch.randn(rows, V, generator=gen) * 2).to(ops.BF16).to(dev())
        return buf

    def both(run):
        """run(gscale, dscale) -> (d(logits), loss values...); the host product against the device product.  d(logits) bit for bit.
        The loss VALUE does not depend on the scale at all and is an atomicAdd over the rows' blocks, in whatever order they finish:
        two launches of the same form already differ in its last bits, so it is held to the reordering bound of a sum of `rows`
        non-negative fp32 terms, (rows - 1) * 2^-24 relative."""
        a = run(0.5 * 2.0 ** k, None)
        b = run(0.5, ds)
        torch.cuda.synchronize()
        assert same_bits(a[0], b[0])
        rows = a[0].shape[0]
        for x, y in zip(a[1:], b[1:]):
            assert abs(float(x) - float(y)) <= (rows - 1) * 2.0 ** -24 * abs(float(x)), (float(x), float(y))
        return a

    # hard-label CE: the smallest shape of tests/test_ops_gpu.py, and V not a multiple of the 8-wide vectors
    for rows, V, ld in ((9, 300, 304), (9, 301, 304)):
        x = logits(rows, V, ld, 7.0)
        labels = torch.randint(0, V, (rows,), generator=gen)
        labels[torch.rand(rows, generator=gen) < 0.4] = -1
        labels[0] = V - 1
        labels = labels.to(dev())

        def ce(gs, d):
            buf, counts, lo = x.clone(), torch.zeros(1, device=dev()), torch.zeros(1, device=dev())
            ops.ce_fwd_bwd(buf, V, labels, counts, lo, gscale=gs, dscale=d)
            return buf, lo
        out = both(ce)
        assert float(out[0].float().abs().max()) > 0

        lab_c = torch.cat((torch.randint(0, V, (6,), generator=gen), torch.full((rows - 6,), -1, dtype=torch.int64))).to(dev())
        c0, c1 = torch.tensor([4.0], device=dev()), torch.tensor([2.0], device=dev())

        def cec(gs, d):
            buf, l0, l1 = x.clone(), torch.zeros(1, device=dev()), torch.zeros(1, device=dev())
            ops.ce_fwd_bwd_compact(buf, V, lab_c, c0, c1, l0, l1, gscale=gs, dscale=d)
            return buf, l0, l1
        both(cec)
    # soft-label CE (C = 1601 is odd) and BCE-with-logits (A = 37): the shapes of tests/test_ops_gpu.py
    rows, C, ld = 29, 1601, 1664
    x = logits(rows, C, ld, 3.0)
    t = torch.softmax(torch.randn(rows, C, generator=gen), -1)
    t[torch.rand(rows, generator=gen) < 0.4] = 0
    t = t.to(dev())

    def soft(gs, d):
        buf, counts, lo, tsum = x.clone(), torch.zeros(1, device=dev()), torch.zeros(1, device=dev()), torch.zeros(rows, device=dev())
        ops.soft_ce_fwd_bwd(buf, C, t, tsum, counts, lo, gscale=gs, dscale=d)
        return buf, lo
    assert float(both(soft)[0].float().abs().max()) > 0
    B, A, Ap = 5, 37, 64
    x = logits(B, A, Ap, 9.0)
    y = ((torch.rand(B, A, generator=gen) < 0.2).float() * torch.rand(B, A, generator=gen)).to(dev())

    def bce(gs, d):
        buf, lo = x.clone(), torch.zeros(1, device=dev())
        ops.bce_logits_fwd_bwd(buf, A, y, lo, gscale=gs, dscale=d, pos_weight=1.5)
        return buf, lo
    assert float(both(bce)[0].float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3. engine
def forward_state(eng):
    """Everything the next forward reads that an optimizer step writes (the dropout seed aside: it advances on every step)."""
    return [eng.P.master, eng.P.m, eng.P.v, eng.P.w16, eng.adam[5:6]] + [eng.wT[k] for k in sorted(eng.wT)]


def test_engine_skips_halves_grows_and_matches_a_static_twin():
    """zero_grad -> forward -> backward, one inf poked into the flat gradient, optimizer_step: nothing the next forward reads may move
    and the schedule advances; every following clean step against a twin STATIC engine at the same scale, bit for bit.

    What "bit for bit" can cover: the engine's backward accumulates the gradients of the biases, LayerNorm parameters and small
    embedding tables with float atomics, so the SAME static engine run twice on the same state already gives different bits there
    (measured on MI355X, this configuration: 7-9 of the tensors differ, by up to 1.2e-4 on a tensor whose largest entry is 1.8e3 =
    one ulp; every GEMM weight gradient is reproducible).  Two separate backward passes can therefore not be compared bit for bit on
    those tensors (nor on the two Linear weights of the front end, which sit behind them), whatever the loss scale.  So the twin's
    d(logits) and its reproducible gradients (every Linear weight of the encoder and the heads) are compared bit for bit with the dynamic engine's, the atomically accumulated ones to their reordering noise, and the optimizer step -- the
    arithmetic this feature adds -- runs on the SAME gradient bits in both engines and is compared bit for bit on everything it writes."""
    E, L, syn = pkg("engine"), pkg("loss_scale"), pkg("synthetic")
    B, T, Rg = 2, 16, 6                                     # the smallest engine of tests/test_engine_gpu.py: one base layer, batch 2
    base, warm, total = 1e-3, 3, 10
    kw = dict(device="cuda:0", train=True, lr=base, weight_decay=1e-2, max_grad_norm=1.0, seed=5)
    dyn = E.PretrainEngine(E.ModelConfig(num_hidden_layers=1), B, T, Rg, lr_schedule="triangle", warmup_steps=warm, t_total=total,
                           loss_scale=L.DynamicLossScale(init_scale=S0, growth_interval=3), **kw)
    twin = E.PretrainEngine(E.ModelConfig(num_hidden_layers=1), B, T, Rg, loss_scale=S0 / 2, **kw)
    dyn.init_random(seed=3)
    batch = [t.to(dev()) for t in syn.make_batch(B, T, Rg, seed=8, ragged=True)]
    dyn.set_batch(*batch)
    twin.set_batch(*batch)
    assert twin.scaler is None and twin.scaler_state() is None and isinstance(twin.loss_scale, float) and dyn.loss_scale == S0
    exp = ref_state(dyn.scaler)

    def lr_at(k):
        return float(np.float32(base) * R.lr_lambda(2, k, warm, total))

    # step 1: one inf in the gradient -> skipped
    dyn.zero_grad(); dyn.forward(True); dyn.backward(True)
    torch.cuda.synchronize()
    assert np.isfinite(dyn.grad_norm()) and dyn.grad_norm() > 0
    dyn.P.grad[dyn.P.numel // 2] = float("inf")
    keep = [t.clone() for t in forward_state(dyn)]
    seed0 = int(dyn.seed)
    dyn.optimizer_step()
    torch.cuda.synchronize()
    for t, k in zip(forward_state(dyn), keep):
        assert same_bits(t, k)
    exp = R.update(exp, True)
    assert dyn.scaler.values() == exp.tolist() and dyn.loss_scale == S0 / 2
    assert dyn.scaler_state() == R.as_dict(exp) and dyn.scaler_state()["skipped_total"] == 1
    assert float(dyn.adam[5]) == 0.0 and float(dyn.adam[7]) == 0.0 and int(dyn.seed) != seed0      # the dropout seed advanced
    assert abs(float(dyn.adam[0]) - lr_at(1)) <= 1e-6 * base

    # clean steps: each against the twin at the same scale, from the same state; the fourth runs at twice the scale
    for i, scale in enumerate((S0 / 2, S0 / 2, S0 / 2, S0), 1):
        assert dyn.loss_scale == scale
        for dst, src in ((twin.P.master, dyn.P.master), (twin.P.m, dyn.P.m), (twin.P.v, dyn.P.v), (twin.adam, dyn.adam), (twin.seed, dyn.seed)):
            dst.copy_(src)
        twin._weights_dirty = True
        twin.loss_scale = scale
        for eng in (dyn, twin):
            eng.zero_grad(); eng.forward(True); eng.backward(True)
        torch.cuda.synchronize()
        for a, b in ((dyn.mlm_logits, twin.mlm_logits), (dyn.mvrc_logits, twin.mvrc_logits)):      # d(logits): device scale == host product
            assert same_bits(a, b) and float(a.float().abs().max()) > 0
        # (the front end's two Linear weights sit behind the embedding backward's atomics: the tied word-embedding table receives its
        # scatter, the obj_downsample weight gradient is computed from the d(obj_reps) it sums -- rarely different, but not reproducible)
        exact = set(dyn._gemm_weight_names()) - {"vlbert.word_embeddings.weight", "image_feature_extractor.obj_downsample.1.weight"}
        rows = dyn.M
        for (n, a), b in zip(dyn.g32.items(), twin.g32.values()):
            if n in exact:
                assert same_bits(a, b), n
            else:      # Float atomics: reordering noise.  The bound is an ASSUMPTION, not a derivation: at most `rows` addends per
                # element, none larger than the tensor's largest sum.  It only keeps these tensors from going unlooked-at; nothing
                # this change adds is judged by it (the optimizer below runs on shared gradient bits).
                assert float((a - b).abs().max()) <= rows * (rows - 1) * 2.0 ** -24 * max(float(b.abs().max()), 1e-30), n
        assert float(dyn.P.grad.abs().max()) > 0
        twin.P.grad.copy_(dyn.P.grad)                       # the same gradient bits into both optimizer steps
        assert dyn.grad_norm() == twin.grad_norm()
        dyn.optimizer_step()
        twin.optimizer_step(lr=float(dyn.adam[0]))          # (the twin has no device schedule: hand it the lr the step ran with)
        torch.cuda.synchronize()
        assert abs(float(dyn.adam[0]) - lr_at(i + 1)) <= 1e-6 * base, i      # schedule step = taken + skipped + 1
        for a, b in zip(forward_state(dyn), forward_state(twin)):
            assert same_bits(a, b), i
        assert not same_bits(dyn.P.master, keep[0])
        exp = R.update(exp, False)
        assert dyn.scaler.values() == exp.tolist() and float(dyn.adam[5]) == float(i)
    assert dyn.loss_scale == S0 and dyn.scaler_state()["unskipped"] == 1
    lv = dyn.loss_values()
    assert np.isfinite(lv["loss"])


def test_engine_host_check_raises_when_the_scale_cannot_help():
    E, L, syn = pkg("engine"), pkg("loss_scale"), pkg("synthetic")
    eng = E.PretrainEngine(E.ModelConfig(num_hidden_layers=1), 2, 16, 6, device="cuda:0", train=False, loss_scale="dynamic")
    assert eng.scaler.spec == L.DynamicLossScale() and eng.loss_scale == 2.0 ** 16
    eng.scaler.state[6] = float(L.MAX_SKIPPED_IN_A_ROW)
    eng._opt_steps = 63
    eng._check_mlm_overflow_now_and_then()                  # 32 skips, but the scale is still above its floor: still recovering
    eng.scaler.state[0] = eng.scaler.spec.min_scale
    eng.scaler.state[6] = float(L.MAX_SKIPPED_IN_A_ROW - 1)
    eng._opt_steps = 63
    eng._check_mlm_overflow_now_and_then()                  # at the floor, one skip short
    eng.scaler.state[6] = float(L.MAX_SKIPPED_IN_A_ROW)
    eng._opt_steps = 63
    with pytest.raises(FloatingPointError, match="in a row"):
        eng._check_mlm_overflow_now_and_then()
    with pytest.raises(ValueError):
        E.PretrainEngine(E.ModelConfig(num_hidden_layers=1), 2, 16, 6, device="cuda:0", core=True, loss_scale="dynamic")


def test_engine_checkpoint_carries_the_scaler(tmp_path):
    E, L, C = pkg("engine"), pkg("loss_scale"), pkg("common.checkpoint")
    mk = lambda ls: E.PretrainEngine(E.ModelConfig(num_hidden_layers=1), 2, 16, 6, device="cuda:0", train=False, loss_scale=ls)
    eng = mk(L.DynamicLossScale(init_scale=S0, growth_interval=7))
    eng.init_random(seed=1)
    eng.scaler.load_values(R.run(ref_state(eng.scaler), [True, False, False])[-1].tolist())
    path = C.save_checkpoint(eng, str(tmp_path / "dyn"), 0)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert list(ck)[:2] == ["state_dict", "optimizer"] and ck[L.CHECKPOINT_KEY]["scale"] == S0 / 2 and ck[L.CHECKPOINT_KEY]["unskipped"] == 2
    eng2 = mk(L.DynamicLossScale(init_scale=S0, growth_interval=7))
    C.load_checkpoint(eng2, path)
    assert eng2.scaler.values() == eng.scaler.values() and same_bits(eng2.P.master, eng.P.master)
    static = mk(None)
    path2 = C.save_checkpoint(static, str(tmp_path / "static"), 0)
    assert L.CHECKPOINT_KEY not in torch.load(path2, map_location="cpu", weights_only=False)
    C.load_checkpoint(eng2, path2)                          # no key: back to the initial state
    assert eng2.scaler.values() == eng2.scaler.spec.initial_values()


# ------------------------------------------------------------------------------------------------ 4. fused optimizers
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_fused_optimizers_with_a_loss_scaler(kind):
    """One skipped and two real steps against the torch statement of tests/test_vcr_gpu.py (clip, then the optimizer), its tolerance."""
    OPT = pkg("optim")
    g0 = torch.Generator().manual_seed(11)
    shapes = [(300, 64), (64,), (1000,), (17, 5)]
    flat = torch.zeros(sum(int(np.prod(sh)) for sh in shapes) + 64, device=dev())
    gflat = torch.zeros_like(flat)
    ps, off = [], 0
    for i, sh in enumerate(shapes):
        n = int(np.prod(sh))
        if i == 2:
            off += 64                                       # a gap: two flat runs, one scaler update
        q = torch.nn.Parameter(flat[off:off + n].view(sh))
        q.data.copy_(torch.randn(sh, generator=g0))
        q.grad = gflat[off:off + n].view(sh)
        ps.append(q)
        off += n
    ref = [torch.nn.Parameter(q.detach().cpu().clone()) for q in ps]
    sc = make_scaler(growth_interval=2)
    if kind == "sgd":
        opt = OPT.FusedSGD(ps, lr=0.05, momentum=0.9, weight_decay=1e-2, loss_scaler=sc)
        ropt = torch.optim.SGD(ref, lr=0.05, momentum=0.9, weight_decay=1e-2)
    else:
        opt = OPT.FusedAdamW(ps, lr=1e-2, eps=1e-6, weight_decay=1e-2, loss_scaler=sc)
        m = [torch.zeros_like(r) for r in ref]
        v = [torch.zeros_like(r) for r in ref]
    exp, taken, max_norm = ref_state(sc), 0, 1.0
    for step, mag, poke, clip in ((1, 3.0, True, True), (2, 3.0, False, True), (3, 0.01, False, False)):
        scale = float(exp[0])
        grads = [torch.randn(sh, generator=g0) * mag for sh in shapes]
        for q, g in zip(ps, grads):
            q.grad.copy_(g * scale)
        if poke:
            ps[3].grad.view(-1)[-1] = float("inf")          # the last element of the second run
        before = [q.detach().clone() for q in ps]
        if clip:
            total = OPT.clip_grad_norm_(ps, max_norm, opt)
        opt.step()                                          # (without a clip call it takes the norm itself)
        torch.cuda.synchronize()
        exp = R.update(exp, poke)
        assert sc.values() == exp.tolist(), step
        if poke:
            assert all(same_bits(q.detach(), b) for q, b in zip(ps, before)) and not np.isfinite(float(total))
            continue
        taken += 1
        for r, g in zip(ref, grads):
            r.grad = g.clone()
        if clip:
            tnorm = torch.nn.utils.clip_grad_norm_(ref, max_norm)
            assert abs(float(total) - float(tnorm)) <= 1e-5 * float(tnorm)      # returned unscaled by the device scale
        if kind == "sgd":
            ropt.step()
        else:
            for r, mm, vv in zip(ref, m, v):
                O.adamw_step(r.data, r.grad, mm, vv, taken, 1e-2, eps=1e-6, weight_decay=1e-2)      # bias correction: steps TAKEN
        err = max(float((q.detach().cpu() - r.detach()).abs().max()) for q, r in zip(ps, ref))
        print("fused %s with a loss scaler, step %d (scale %g): max |p - torch| %.3e" % (kind, step, scale, err))
        assert err < 5e-6
    assert sc.read()["scale"] == S0 and sc.read()["skipped_total"] == 1      # halved once, grown once (interval 2)
    if kind == "adamw":
        assert all(opt.state[q]["step"] == 3 for q in ps)   # the host-side count: steps attempted
