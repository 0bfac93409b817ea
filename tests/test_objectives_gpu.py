"""The pre-training objective switches on the GPU (-m gpu): the per-sample weight kernel and the row-weighted losses of csrc/loss.hip
against tests/objectives_ref.py, then the engine's objective variants (ends_16.Heads16) at the dimensions of
tests/golden/objectives/objectives_small.npz against the same restatement and against what the real reference recorded.

Bars: the kernel tests take those of tests/test_ops_gpu.py::test_ce_fwd_bwd / test_soft_ce_fwd_bwd (loss 1e-4 + 1e-3 |ref|, d(logits)
1e-5 + bar16(1e-2) max |ref|) -- the only new arithmetic is one fp32 multiply per row; the engine tests those of
tests/test_engine_gpu.py::check_against_oracle (losses and gradient norm 1e-2, per-parameter gradients 5e-2 relative Frobenius).

Some cases need a process of their own (one precision per process; an initialised process group): this file re-runs itself as a
script, the way tests/test_loss_scale_f16_gpu.py does."""
import importlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from tests import objectives_ref as R  # noqa: E402
from tests.gpu_util import EngineDropoutMasks, act_dtype, bar16, bf, dev, device_seed, pkg, report  # noqa: E402
from tests.test_objectives_cpu import case, fixture, ref_result  # noqa: E402

pytestmark = pytest.mark.gpu
COMBOS = [(ds, acc, cp) for ds in (False, True) for acc in (False, True) for cp in (False, True)]      # dscale, acc, logits_copy


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def hard_labels(pattern, B, T, V, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, V, (B, T), generator=g)
    lab[torch.rand(B, T, generator=g) < 0.4] = -1
    lab[0, 0], lab[-1, -1] = V - 1, 0          # (every sample keeps a label before the pattern takes some away)
    if pattern == "one_sample_unlabelled":
        lab[1] = -1
    elif pattern == "all_unlabelled":
        lab[:] = -1
    elif pattern == "one_sample_carries_every_label":
        lab[1:] = -1
        lab[0] = torch.randint(0, V, (T,), generator=g)
    return lab.view(-1)


def padded(x, ld, fill=7.0):
    buf = torch.full((x.shape[0], ld), fill, dtype=act_dtype(), device=dev())
    buf[:, :x.shape[1]] = x.to(act_dtype()).to(dev())
    return buf


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["one_sample_unlabelled", "all_unlabelled", "one_sample_carries_every_label"])
@pytest.mark.parametrize("B,T,V", [(3, 5, 37), (2, 3, 30522)])
def test_weighted_ce_against_the_restatement(B, T, V, pattern):
    """vlb_sample_norm_weights + vlb_ce_rowweight_fwd_bwd on full rows (V = 37: padding columns inside the last 8-wide load; 30522: 15
    chunks per thread row), with / without dscale, counters and a kept copy; then the forward-only twin."""
    ops = pkg("ops")
    ld = (V + 7) // 8 * 8
    x = bf(torch.randn(B * T, V, generator=torch.Generator().manual_seed(7)) * 2.0)
    lab = hard_labels(pattern, B, T, V, 8)
    gs = 0.5
    l0, _, dref = R.weighted_ce(x, lab, B, T, gscale=gs * 4.0)
    n_lab = int((lab >= 0).sum())
    labg = lab.to(dev())
    # the unweighted kernel's counters on the same input: what the weighted forms must count
    acc_ref, c_ref, lo_ref = torch.zeros(2, dtype=torch.int64, device=dev()), torch.zeros(1, device=dev()), torch.zeros(1, device=dev())
    ops.ce_fwd_bwd(padded(x, ld), V, labg, c_ref, lo_ref, acc=acc_ref)
    first = None
    for ds, with_acc, with_copy in COMBOS:
        buf = padded(x, ld)
        w, counts, lo = torch.full((B,), 9.0, device=dev()), torch.full((2,), 9.0, device=dev()), torch.zeros(2, device=dev())
        acc = torch.zeros(2, dtype=torch.int64, device=dev()) if with_acc else None
        cp = torch.zeros((B * T, ld), dtype=act_dtype(), device=dev()) if with_copy else None
        scale = torch.full((1,), 4.0, device=dev())
        ops.sample_norm_weights(w, T, labels=labg, V=V, count0=counts[0:1])
        ops.ce_rowweight_fwd_bwd(buf, V, labg, w, T, lo[0:1], gscale=gs if ds else gs * 4.0, logits_copy=cp, dscale=scale if ds else None,
                                 acc=acc)
        tag = "weighted ce %dx%dx%d %s ds=%d acc=%d copy=%d" % (B, T, V, pattern, ds, with_acc, with_copy)
        report(tag + " loss", lo[0:1], torch.tensor([l0]), 1e-4, 1e-3)
        report(tag + " dlogits", buf[:, :V], dref, 1e-5, bar16(1e-2))
        assert float(buf[:, V:].float().abs().max() if ld > V else 0.0) == 0.0, "pad columns must be zeroed"
        assert float(counts[0]) == n_lab and float(counts[1]) == 9.0 and float(lo[1]) == 0.0
        if n_lab == 0:
            assert float(lo[0]) == 0.0 and not bool(buf.float().abs().max() > 0) and not bool(torch.isnan(w).any())
        if with_copy:
            report(tag + " copy", cp[:, :V], x, 0, 0)
        if with_acc:
            assert torch.equal(acc, acc_ref), (acc, acc_ref)
        # every form leaves the same gradient bits (the device scale times gscale is the product the static form was given)
        if first is None:
            first = bits(buf).clone()
        assert torch.equal(bits(buf), first), tag
    # forward only: the same loss up to the order of the rows' atomic adds (n terms: n 2^-24 sum |term|), the logits untouched
    buf = padded(x, ld)
    before = bits(buf).clone()
    lo2, acc2 = torch.zeros(1, device=dev()), torch.zeros(2, dtype=torch.int64, device=dev())
    ops.ce_rowweight_eval(buf, V, labg, w, T, lo2, acc2)
    assert abs(float(lo2) - float(lo[0])) <= max(n_lab, 1) * 2.0 ** -24 * abs(float(lo[0]))
    assert torch.equal(bits(buf), before) and torch.equal(acc2, acc_ref)


def test_weighted_ce_on_compacted_rows_with_the_caption_aux_split():
    """The rows mlm_compact lists (caption samples 0-1, then the text-only sample 2), through sel_pos: loss slots 0 and 2 each right,
    the gradient rows those of the full-row restatement, the padding rows behind the list zero."""
    ops = pkg("ops")
    B, T, V, split, cap = 3, 5, 37, 2, 16
    ld = 40
    x = bf(torch.randn(B * T, V, generator=torch.Generator().manual_seed(11)) * 2.0)
    lab = hard_labels("plain", B, T, V, 12)
    l0, l1, dref = R.weighted_ce(x, lab, B, T, B_split=split)
    assert l0 > 0 and l1 > 0
    labg = lab.to(dev())
    sel_pos, sel_src = (torch.zeros(cap, dtype=torch.int32, device=dev()) for _ in range(2))
    labels_c = torch.zeros(cap, dtype=torch.int64, device=dev())
    counts, over = torch.zeros(4, device=dev()), torch.zeros(1, dtype=torch.int32, device=dev())
    ops.mlm_compact(labg, torch.arange(B * T, dtype=torch.int32, device=dev()), split * T, V, sel_pos, sel_src, labels_c, counts[0:1],
                    counts[2:3], over)
    n = int((lab >= 0).sum())
    pos = sel_pos.cpu().long()
    assert int(over) == 0 and pos[:n].tolist() == [i for i in range(B * T) if lab[i] >= 0] and (pos[n:] == -1).all()
    xc = torch.zeros(cap, V)
    xc[:n] = x[pos[:n]]
    for ds, with_acc, with_copy in COMBOS:
        buf = padded(xc, ld)
        cp = torch.zeros((cap, ld), dtype=act_dtype(), device=dev()) if with_copy else None
        w, losses = torch.zeros(B, device=dev()), torch.zeros(4, device=dev())
        acc = torch.zeros((2, 2), dtype=torch.int64, device=dev())
        ops.sample_norm_weights(w, T, labels=labg, V=V, B_split=split)
        ops.ce_rowweight_fwd_bwd(buf, V, labels_c, w, T, losses[0:1], B_split=split, loss_out1=losses[2:3], sel_pos=sel_pos,
                                 gscale=0.25 if ds else 1.0, dscale=torch.full((1,), 4.0, device=dev()) if ds else None, logits_copy=cp,
                                 **(dict(acc=acc[0], acc1=acc[1]) if with_acc else {}))
        if with_copy:      # (the engine keeps no copy of compacted rows; the entry point allows one)
            report("compacted weighted ce: kept copy", cp[:n, :V], xc[:n], 0, 0)
        report("compacted weighted ce: caption loss (slot 0)", losses[0:1], torch.tensor([l0]), 1e-4, 1e-3)
        report("compacted weighted ce: text-only loss (slot 2)", losses[2:3], torch.tensor([l1]), 1e-4, 1e-3)
        assert float(losses[1]) == 0.0 and float(losses[3]) == 0.0
        report("compacted weighted ce: dlogits", buf[:n, :V], dref[pos[:n]], 1e-5, bar16(1e-2))
        assert float(buf[n:].float().abs().max()) == 0.0 and float(buf[:, V:].float().abs().max()) == 0.0
        if with_acc:
            assert acc[:, 1].tolist() == [int((lab[:split * T] >= 0).sum()), int((lab[split * T:] >= 0).sum())]
            hits = (xc[:n].argmax(1) == lab[pos[:n]])
            assert acc[:, 0].tolist() == [int(hits[pos[:n] < split * T].sum()), int(hits[pos[:n] >= split * T].sum())]
    # forward-only twin over the same list
    buf = padded(xc, ld)
    before, lo = bits(buf).clone(), torch.zeros(4, device=dev())
    acc2 = torch.zeros((2, 2), dtype=torch.int64, device=dev())
    ops.ce_rowweight_eval(buf, V, labels_c, w, T, lo[0:1], acc2[0], B_split=split, loss_out1=lo[2:3], acc1=acc2[1], sel_pos=sel_pos)
    assert torch.equal(bits(buf), before) and torch.equal(acc2, acc)
    for k in (0, 2):
        assert abs(float(lo[k]) - float(losses[k])) <= n * 2.0 ** -24 * abs(float(losses[k]))


@pytest.mark.parametrize("B,Rg,C", [(3, 4, 5), (2, 3, 1601)])
def test_weighted_soft_ce_against_the_restatement(B, Rg, C):
    """vlb_soft_ce_rowweight_fwd_bwd with one sample of only invalid rows (and an invalid row inside a valid sample)."""
    ops = pkg("ops")
    ld = (C + 7) // 8 * 8
    g = torch.Generator().manual_seed(21)
    x = bf(torch.randn(B * Rg, C, generator=g) * 2.0)
    t = torch.softmax(torch.randn(B * Rg, C, generator=g), -1)
    t[0] = t[0] * 1.05                  # still valid: |sum - 1| < 0.1
    t[1] = 0                            # an invalid row of a valid sample
    t[(B - 1) * Rg:] = 0                # the last sample: no valid region
    valid = ((t.sum(1) - 1).abs() < 0.1)
    lref, dref = R.weighted_soft_ce(x, t, B, Rg, gscale=2.0)
    tg = t.to(dev())
    acc_ref, c_ref, lo_ref = torch.zeros(2, dtype=torch.int64, device=dev()), torch.zeros(1, device=dev()), torch.zeros(1, device=dev())
    ops.soft_ce_fwd_bwd(padded(x, ld, 3.0), C, tg, torch.zeros(B * Rg, device=dev()), c_ref, lo_ref, acc=acc_ref)
    first = None
    for ds, with_acc, with_copy in COMBOS:
        buf = padded(x, ld, 3.0)
        tsum, w, counts, lo = (torch.full((n,), 9.0, device=dev()) for n in (B * Rg, B, 1, 1))
        lo.zero_()
        acc = torch.zeros(2, dtype=torch.int64, device=dev()) if with_acc else None
        cp = torch.zeros((B * Rg, ld), dtype=act_dtype(), device=dev()) if with_copy else None
        ops.soft_ce_rowweight_fwd_bwd(buf, C, tg, tsum, w, Rg, counts, lo, gscale=0.5 if ds else 2.0, logits_copy=cp,
                                      dscale=torch.full((1,), 4.0, device=dev()) if ds else None, acc=acc)
        tag = "weighted soft ce %dx%dx%d ds=%d acc=%d copy=%d" % (B, Rg, C, ds, with_acc, with_copy)
        report(tag + " loss", lo, torch.tensor([lref]), 1e-4, 1e-3)
        report(tag + " dlogits", buf[:, :C], dref, 1e-5, bar16(1e-2))
        assert float(buf[:, C:].float().abs().max() if ld > C else 0.0) == 0.0
        assert float(counts) == float(valid.sum()) == float(c_ref) and float(w[B - 1]) == 0.0
        assert not bool(buf[~valid.to(dev())].float().abs().max() > 0)
        if with_copy:
            report(tag + " copy", cp[:, :C], x, 0, 0)
        if with_acc:
            assert torch.equal(acc, acc_ref), (acc, acc_ref)
        if first is None:
            first = bits(buf).clone()
        assert torch.equal(bits(buf), first), tag
    buf = padded(x, ld, 3.0)
    before, lo2, acc2 = bits(buf).clone(), torch.zeros(1, device=dev()), torch.zeros(2, dtype=torch.int64, device=dev())
    ops.soft_ce_rowweight_eval(buf, C, tg, tsum, w, Rg, counts, lo2, acc2)
    assert abs(float(lo2) - float(lo)) <= B * Rg * 2.0 ** -24 * abs(float(lo))
    assert torch.equal(bits(buf), before) and torch.equal(acc2, acc_ref)
    # no valid row at all: loss 0, gradient 0, nothing NaN
    buf, lo3 = padded(x, ld, 3.0), torch.zeros(1, device=dev())
    ops.soft_ce_rowweight_fwd_bwd(buf, C, torch.zeros_like(tg), tsum, w, Rg, counts, lo3)
    assert float(lo3) == 0.0 and float(counts) == 0.0 and not bool(buf.float().abs().max() > 0) and not bool(w.abs().max() > 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------------------
def model_config(cfg, sw, **kw):
    E = pkg("engine")
    return E.ModelConfig(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                         intermediate_size=cfg.intermediate_size, vocab_size=cfg.vocab_size, max_position_embeddings=cfg.max_position_embeddings,
                         visual_region_classes=cfg.visual_region_classes, hidden_dropout_prob=cfg.hidden_dropout_prob,
                         attention_probs_dropout_prob=cfg.attention_probs_dropout_prob, obj_downsample_dropout=cfg.obj_downsample_dropout,
                         multitask=cfg.multitask, **dict(sw.engine_kw(), **kw))


def fixture_engine(name, multitask, train=False, **kw):
    """(engine with the case's parameters and batch loaded, cfg, switches, params, batch)."""
    E = pkg("engine")
    tag, cfg, sw, batch = case(name, multitask)
    params = R.init_params(cfg, int(fixture()["pseed"]), sw)
    B, T, Rg = batch[2].shape[0], batch[2].shape[1], batch[0].shape[1]
    Ba, Tm = (batch[7].shape[0], max(T, batch[7].shape[1])) if multitask else (0, T)
    eng = E.PretrainEngine(model_config(cfg, sw), B, Tm, Rg, device="cuda:0", train=train, B_aux=Ba, **dict(dict(keep_logits=True), **kw))
    eng.load_state_dict({k: v.to(dev()) for k, v in params.items()})
    eng.set_batch(*[t.to(dev()) for t in batch])
    return eng, cfg, sw, params, batch


def rel_fro(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / max(b.norm(), 1e-12))


RAN = [(n, m) for m in (False, True) for n in ("mlm_only", "mvrc_only", "both_norm", "mlm_only_norm", "mvrc_only_norm", "both")
       if not (m and n.startswith("mvrc_only"))]


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name,multitask", RAN)
def test_engine_objective_variants_vs_restatement_and_reference(name, multitask, train):
    """The fixture cases (the reference's multitask wrapper cannot run MVRC-only: not a case): losses, gradient norm and every parameter
    gradient against tests/objectives_ref.py -- in train mode under the masks the engine regenerates --, the absent head's slot and
    parameters, and in eval mode losses and gradient norm against the REAL reference's recorded values."""
    z = fixture()
    eng, cfg, sw, params, batch = fixture_engine(name, multitask, train=train)
    tag = "%s/%s/" % ("multitask" if multitask else "plain", name)
    seed = device_seed(eng)
    eng.zero_grad()
    eng.forward(train=train)
    eng.backward(train=train)
    torch.cuda.synchronize()
    if train:
        hook = EngineDropoutMasks(seed, eng.S, eng.R, eng.cfg.num_attention_heads)
        outputs, loss, grads, norm = R.loss_and_grads(params, cfg, batch, sw, train=True, drop_hook=hook)
    else:
        outputs, loss, grads, norm = ref_result(name, multitask)
    lv = eng.loss_values()
    keys = ("mlm_loss_wvc", "mlm_loss_aux", "mvrc_loss") if multitask else ("mlm_loss", "mvrc_loss")
    for k in keys:
        ref = float(outputs[k])
        print("%s%s %s: hip %.6f restatement %.6f" % (tag, "train" if train else "eval", k, lv[k], ref))
        assert abs(lv[k] - ref) <= 1e-2 * max(1.0, abs(ref)), (k, lv[k], ref)
    # an absent head: its key stays, its slot is exactly zero, its parameters are not there
    assert lv["relationship_loss"] == 0.0
    if not sw.with_mlm_loss:
        assert lv["mlm_loss"] == 0.0 and float(eng.losses[2]) == 0.0 and float(eng.counts[0]) == 0.0 and not hasattr(eng, "mlm_logits")
    if not sw.with_mvrc_loss:
        assert lv["mvrc_loss"] == 0.0 and float(eng.counts[1]) == 0.0 and not hasattr(eng, "mvrc_logits")
    got = eng.grads()
    assert set(got) == set(params) and not [n for n in got if R.absent(n, sw)]
    sd = eng.state_dict()
    assert ("vlbert.mlm_head.predictions.decoder.weight" in sd) == sw.with_mlm_loss and set(sd) - {"vlbert.mlm_head.predictions.decoder.weight"} == set(params)
    gn = eng.grad_norm()
    print("%s grad_norm: hip %.6f restatement %.6f" % (tag, gn, norm))
    assert abs(gn - norm) <= 1e-2 * norm
    worst = sorted(((rel_fro(g, grads[n]), n) for n, g in got.items() if float(grads[n].norm()) >= 1e-6 * norm), reverse=True)
    for e, n in worst[:5]:
        print("   rel-fro grad err %.3e  %s" % (e, n))
    assert worst[0][0] <= 5e-2, worst[:5]
    # the gradient of object_mask_visual_embedding (next to the one-row linguistic table in the flat buffer) is among them
    if not train:
        for k in keys + ("loss",):
            assert abs(lv[k] - float(z[tag + k])) <= 1e-2 * max(1.0, abs(float(z[tag + k]))), (k, lv[k], float(z[tag + k]))
        assert abs(gn - float(z[tag + "grad_norm"])) <= 1e-2 * float(z[tag + "grad_norm"])


@pytest.mark.parametrize("name", ["mlm_only", "mvrc_only"])
def test_rows_that_reach_no_loss_get_exactly_zero_gradient(name):
    """d X[L] as the heads leave it: with one head absent, the rows only it would have fed -- the text rows without MLM, the object rows
    without MVRC -- are exactly zero, and the other kind is not."""
    eng, cfg, sw, params, batch = fixture_engine(name, False)
    eng.zero_grad()
    eng.forward(train=False)
    dx = eng.back.heads_bwd().clone()
    eng._join_side()
    torch.cuda.synchronize()
    # rows of the packed sequence: a sample's objects follow its last token, so the slots of its padded text positions hold objects --
    # the rows of the real tokens and of the real boxes are what the two heads feed
    trow = eng.lay["text_rows"].view(-1).long()[eng.text_mask.view(-1).bool()]
    orow = eng.lay["obj_rows"].view(-1).long()[eng.box_mask.view(-1).bool()]
    assert trow.numel() and orow.numel() and not set(trow.tolist()) & set(orow.tolist())
    dead, live = (trow, orow) if name == "mvrc_only" else (orow, trow)
    assert not bool(dx[dead].float().abs().max() > 0) and bool(dx[live].float().abs().max() > 0)
    other = torch.ones(dx.shape[0], dtype=torch.bool, device=dev())
    other[torch.cat((trow, orow))] = False
    assert not bool(dx[other].float().abs().max() > 0)            # END and padding rows feed no head


def test_compacted_mlm_rows_equal_the_full_rows_under_the_norm_switch(monkeypatch):
    """B x T = 288 positions > the 256-row capacity floor: the MLM head runs on the labelled rows, weighted through sel_pos; losses and
    gradients equal the full-row path's (as test_engine_fp32_full_compacted_mlm_rows_match_the_full_path for the unweighted loss)."""
    E, syn = pkg("engine"), pkg("synthetic")
    res = []
    for compact in ("1", "0"):
        monkeypatch.setenv("VLB_MLM_COMPACT", compact)
        mc = E.ModelConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=1, vocab_size=1000,
                           visual_region_classes=40, multitask=True, mlm_norm_in_batch_first=True, mvrc_norm_in_batch_first=True)
        eng = E.PretrainEngine(mc, 4, 48, 4, device="cuda:0", train=False, seed=5, B_aux=2)
        assert (eng.mlm_cap is not None) == (compact == "1")
        eng.init_random(seed=3, visual_ln_init=1.0)
        batch = list(syn.make_batch(4, 48, 4, vocab_size=1000, region_classes=40, seed=10, ragged=True))
        batch[4][1] = -1
        aux = syn.make_aux_text(2, 48, vocab_size=1000, seed=10)
        eng.set_batch(*[t.to(dev()) for t in batch], aux_text=aux[0].to(dev()), aux_mlm_labels=aux[1].to(dev()))
        eng.zero_grad()
        eng.forward(train=False)
        eng.backward(train=False)
        torch.cuda.synchronize()
        res.append((eng.loss_values(), eng.grads(), eng.counts.cpu()))
    a, b = res
    for k in ("mlm_loss_wvc", "mlm_loss_aux", "mvrc_loss"):
        assert a[0][k] > 0 and abs(a[0][k] - b[0][k]) <= 1e-5 * b[0][k], (k, a[0][k], b[0][k])
    assert torch.equal(a[2], b[2])
    norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in b[1].values())))
    worst = sorted(((rel_fro(a[1][n], g), n) for n, g in b[1].items() if float(g.norm()) >= 1e-6 * norm), reverse=True)
    print("compacted vs full rows under the norm switch: worst rel-fro %.3e (%s)" % worst[0])
    # The two paths run the same rows through GEMMs of another height, so fp32 sums form in another order and a 16-bit store may round
    # the other way: one element then moves by 2^-8 relative, and a quarter of a tensor's elements doing so is 2^-8 sqrt(1/4) = 2e-3
    assert worst[0][0] <= 2e-3, worst[:4]


def test_graph_replay_of_the_weighted_step_equals_the_eager_step():
    """Two train_step()s replayed from make_step_graph() against eager shadow steps from the same state (the pattern of
    tests/test_long_sequence_engine_gpu.py): d(logits) and the reproducible gradients bit for bit, then weights and optimizer state."""
    E, syn = pkg("engine"), pkg("synthetic")
    B, T, Rg = 3, 16, 6
    batch = list(syn.make_batch(B, T, Rg, vocab_size=1000, region_classes=40, seed=47, ragged=True))
    batch[4][2] = -1
    batch = [t.to(dev()) for t in batch]

    def engine():
        mc = E.ModelConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, vocab_size=1000,
                           visual_region_classes=40, with_mvrc_loss=False, mlm_norm_in_batch_first=True)
        eng = E.PretrainEngine(mc, B, T, Rg, device="cuda:0", train=True, lr=1e-4, weight_decay=1e-2, max_grad_norm=1.0, seed=5)
        eng.init_random(seed=3)
        eng.set_batch(*batch)
        return eng

    def carried(e):
        return [e.P.master, e.P.m, e.P.v, e.adam, e.seed]

    eng, shadow = engine(), engine()
    eng.train_step()
    torch.cuda.synchronize()
    step = eng.make_step_graph()
    exact = set(eng._gemm_weight_names()) - {"vlbert.word_embeddings.weight", "image_feature_extractor.obj_downsample.1.weight"}
    assert exact
    for i in range(2):
        for dst, src in zip(carried(shadow), carried(eng)):
            dst.copy_(src)
        shadow._weights_dirty = True
        step()
        shadow.zero_grad(); shadow.forward(True); shadow.backward(True)
        torch.cuda.synchronize()
        a, b = float(eng.losses[0]), float(shadow.losses[0])
        assert b > 0 and abs(a - b) <= eng.BT * 2.0 ** -24 * abs(b) and float(eng.losses[1]) == 0.0
        assert torch.equal(bits(eng.mlm_logits), bits(shadow.mlm_logits)), "replay %d: d(logits) differ" % i
        assert torch.equal(eng.back.mlm_w, shadow.back.mlm_w)
        for (n, ga), gb in zip(eng.g32.items(), shadow.g32.values()):
            if n in exact:
                assert torch.equal(bits(ga), bits(gb)), "replay %d: gradient of %s differs" % (i, n)
        shadow.P.grad.copy_(eng.P.grad)
        shadow.optimizer_step()
        torch.cuda.synchronize()
        for nme, a, b in zip(("master", "m", "v", "adam", "seed"), carried(eng), carried(shadow)):
            assert torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b), (i, nme)
    assert step.n_graphs == 1 and step.n_calls == 0


def test_eval_step_of_an_mvrc_only_engine_leaves_the_mlm_rows_alone():
    eng, cfg, sw, params, batch = fixture_engine("mvrc_only", False, keep_logits=False)
    ref = ref_result("mvrc_only", False)[0]
    eng.reset_metrics()
    eng.eval_step()
    torch.cuda.synchronize()
    m, lv = eng.metric_counts(), eng.loss_values()
    valid = int(((batch[6].sum(-1) - 1).abs() < 0.1).sum())
    assert m["mlm"] == (0, 0) and m["mlm_aux"] == (0, 0) and m["relationship"] == (0, 0) and m["mvrc"][1] == valid > 0
    assert lv["mlm_loss"] == 0.0 and abs(lv["mvrc_loss"] - float(ref["mvrc_loss"])) <= 1e-2 * max(1.0, float(ref["mvrc_loss"]))
    # the weighted forward-only path: both norm switches, same batch
    eng2 = fixture_engine("both_norm", False, keep_logits=False)[0]
    ref2 = ref_result("both_norm", False)[0]
    eng2.reset_metrics()
    eng2.eval_step()
    torch.cuda.synchronize()
    m2, lv2 = eng2.metric_counts(), eng2.loss_values()
    assert m2["mvrc"][1] == valid and m2["mlm"][1] == int((batch[4] >= 0).sum())
    for k in ("mlm_loss", "mvrc_loss"):
        assert abs(lv2[k] - float(ref2[k])) <= 1e-2 * max(1.0, float(ref2[k])), k


def test_train_metrics_count_the_rows_the_unweighted_losses_count():
    """train_metrics=True under both norm switches: [hits, counted rows] per head as eval_step counts them on the same weights."""
    eng = fixture_engine("both_norm", True, train_metrics=True)[0]
    eng.zero_grad()
    eng.forward(train=False)
    eng.backward(train=False)
    eng.reset_metrics()
    eng.eval_step()
    torch.cuda.synchronize()
    assert eng.train_metric_counts() == eng.metric_counts() and eng.metric_counts()["mlm_aux"][1] > 0


def test_module_mirror_without_the_mvrc_loss():
    """ResNetVLBERTForPretraining with WITH_MVRC_LOSS: false: the outputs dict carries None for the absent head, loss.backward() fills
    .grad of exactly the present parameters, and losses / gradients are the restatement's."""
    from tests.test_engine_gpu import _module_config
    M = pkg("pretrain.modules.resnet_vlbert_for_pretraining")
    tag, cfg, sw, batch = case("mlm_only_norm", False)
    params = R.init_params(cfg, int(fixture()["pseed"]), sw)
    mcfg = _module_config(cfg)
    mcfg["NETWORK"].update(WITH_MVRC_LOSS=False, MLM_LOSS_NORM_IN_BATCH_FIRST=True, MVRC_LOSS_NORM_IN_BATCH_FIRST=True)
    net = M.ResNetVLBERTForPretraining(mcfg)
    names = [n for n, _ in net.named_parameters()]
    assert set(names) == set(params)
    assert set(net.state_dict()) == set(params) | {"vlbert.mlm_head.predictions.decoder.weight"}
    net.load_state_dict({k: v.to(dev()) for k, v in params.items()})
    net.eval()
    outputs, loss = net(None, *[t.to(dev()) for t in batch])
    assert outputs["mvrc_logits"] is None and outputs["mvrc_label"] is None and outputs["relationship_logits"] is None
    assert tuple(outputs["mlm_logits"].shape) == (3, batch[2].shape[1], cfg.vocab_size) and float(outputs["mvrc_loss"]) == 0.0
    loss.backward()
    torch.cuda.synchronize()
    ref_out, ref_loss, grads, norm = ref_result("mlm_only_norm", False)
    assert abs(float(loss) - float(ref_loss)) <= 1e-2 * float(ref_loss)
    got = {n: p.grad for n, p in net.named_parameters()}
    assert all(g is not None for g in got.values())
    worst = sorted(((rel_fro(g, grads[n]), n) for n, g in got.items() if float(grads[n].norm()) >= 1e-6 * norm), reverse=True)
    assert worst[0][0] <= 5e-2, worst[:4]
    # against the REAL reference's record: the gradient norm a per-sample mean gives (the batch mean's is 11 % smaller on this batch)
    z, gn = fixture(), float(torch.sqrt(sum((g.double() ** 2).sum() for g in got.values())))
    assert abs(gn - float(z["plain/mlm_only_norm/grad_norm"])) <= 1e-2 * float(z["plain/mlm_only_norm/grad_norm"])
    assert abs(gn - float(z["plain/mlm_only/grad_norm"])) > 5e-2 * float(z["plain/mlm_only/grad_norm"])
    with pytest.raises(NotImplementedError, match="multitask wrapper without WITH_MLM_LOSS"):
        mcfg["NETWORK"].update(WITH_MVRC_LOSS=True, WITH_MLM_LOSS=False)
        M.ResNetVLBERTForPretrainingMultitask(mcfg)


def test_e2e_engine_mlm_only_step():
    """The e2e configuration shares the front end and the heads: one MLM-only step under the norm switch at the image size of
    tests/test_vision_gpu.py -- finite loss, MVRC slot zero, the linguistic table's one-row gradient finite."""
    from tests.test_vision_gpu import _vision_fixture
    E, syn = pkg("engine"), pkg("synthetic")
    z, nl, P = _vision_fixture()
    img, boxes4 = torch.from_numpy(z["img"]), torch.from_numpy(z["boxes"]).clone()
    B, Rg, T = boxes4.shape[0], boxes4.shape[1], 12
    batch = list(syn.make_batch(B, T, Rg, seed=22, ragged=False))
    batch[0] = torch.cat((boxes4, torch.zeros(B, Rg, 2048)), -1)
    batch[1] = torch.from_numpy(z["im_info"])
    pad = boxes4[:, :, 0] <= -1.5
    batch[5][pad] = 0
    batch[6][pad] = 0
    mc = E.ModelConfig(num_hidden_layers=1, e2e=True, image_num_layers=nl, with_mvrc_loss=False, mlm_norm_in_batch_first=True)
    eng = E.PretrainEngine(mc, B, T, Rg, device="cuda:0", train=True, lr=1e-4, image_size=tuple(img.shape[2:]))
    eng.init_random(seed=3, visual_ln_init=1.0)
    eng.set_batch(*[t.to(dev()) for t in batch], image=img.to(dev()))
    eng.train_step()
    torch.cuda.synchronize()
    lv = eng.loss_values()
    assert np.isfinite(lv["loss"]) and lv["mlm_loss"] > 0 and lv["mvrc_loss"] == 0.0
    assert "object_mask_word_embedding.weight" not in eng.g32 and bool(torch.isfinite(eng.P.grad).all()) and bool(torch.isfinite(eng.P.master).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# cases that need a process of their own
# ---------------------------------------------------------------------------------------------------------------------------------
def _child(mode, env_extra):
    env = dict(os.environ, **env_extra)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and ("OBJECTIVES CHILD OK: " + mode) in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_dynamic_loss_scale_on_the_fp16_build_with_the_weighted_losses():
    _child("f16_dynamic", {"VLB_PRECISION": "f16"})


def test_forced_exchange_in_a_world_of_one_with_an_absent_head():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    _child("dp_world1", {"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "OMP_NUM_THREADS": "4"})


def _small_engine(E, batch, B, T, Rg, **kw):
    mc = E.ModelConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, vocab_size=1000,
                       visual_region_classes=40, **kw.pop("model"))
    eng = E.PretrainEngine(mc, B, T, Rg, device="cuda:0", train=True, lr=1e-4, weight_decay=1e-2, max_grad_norm=1.0, seed=5, **kw)
    eng.init_random(seed=3, visual_ln_init=1.0)
    eng.set_batch(*batch)
    return eng


def _child_f16_dynamic():
    """Two steps with the dynamic loss scale on the fp16 build, both norm switches on: the device scale reaches the weighted kernels
    (d(logits) = the static engine's at the same scale, bit for bit), the steps are taken and everything stays finite."""
    E, L, ops, syn = (importlib.import_module("vl-bert_amd." + n) for n in ("engine", "loss_scale", "ops", "synthetic"))
    assert ops.BF16 == torch.float16, "the child must run the fp16 build"
    B, T, Rg = 3, 16, 6
    batch = list(syn.make_batch(B, T, Rg, vocab_size=1000, region_classes=40, seed=8, ragged=True))
    batch[4][0] = -1
    batch = [t.to("cuda:0") for t in batch]
    model = dict(mlm_norm_in_batch_first=True, mvrc_norm_in_batch_first=True)
    dyn = _small_engine(E, batch, B, T, Rg, model=dict(model), loss_scale=L.DynamicLossScale(init_scale=1024.0, growth_interval=1000))
    sta = _small_engine(E, batch, B, T, Rg, model=dict(model), loss_scale=1024.0)
    for eng in (dyn, sta):
        eng.zero_grad(); eng.forward(True)
    torch.cuda.synchronize()
    for a, b in ((dyn.mlm_logits, sta.mlm_logits), (dyn.mvrc_logits, sta.mvrc_logits)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and bool(a.float().abs().max() > 0)
    w0 = dyn.P.master.clone()
    for _ in range(2):
        dyn.train_step()
    torch.cuda.synchronize()
    st, lv = dyn.scaler_state(), dyn.loss_values()
    assert int(float(dyn.adam[5])) == 2 and st["skipped_total"] == 0 and st["scale"] == 1024.0, st
    assert all(np.isfinite(v) for v in lv.values()) and lv["mlm_loss"] > 0 and lv["mvrc_loss"] > 0, lv
    assert bool(torch.isfinite(dyn.P.master).all()) and not torch.equal(dyn.P.master, w0)
    print("OBJECTIVES CHILD OK: f16_dynamic")


def _child_dp_world1():
    """An MLM-only engine through the data-parallel exchange in a world of one (every collective the identity; both modes): no bucket
    needs the absent head, the step is finite and its gradient the no-exchange step's."""
    import torch.distributed as dist
    E, syn = (importlib.import_module("vl-bert_amd." + n) for n in ("engine", "synthetic"))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    B, T, Rg = 3, 16, 6
    batch = [t.to("cuda:0") for t in syn.make_batch(B, T, Rg, vocab_size=1000, region_classes=40, seed=8, ragged=True)]
    model = dict(with_mvrc_loss=False, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, obj_downsample_dropout=0.0)
    os.environ["VLB_DP_FORCE_EXCHANGE"] = "0"
    plain = _small_engine(E, batch, B, T, Rg, model=dict(model))
    assert plain.buckets is None
    plain.zero_grad(); plain.forward(True); plain.backward(True)
    torch.cuda.synchronize()
    os.environ["VLB_DP_FORCE_EXCHANGE"] = "1"
    for mode in ("allreduce", "sharded"):
        eng = _small_engine(E, batch, B, T, Rg, model=dict(model), dp_mode=mode)
        assert eng.buckets is not None and eng.buckets.sharded == (mode == "sharded")
        assert "vlbert.mvrc_head.transform.dense.weight" not in eng.P.offsets
        eng.train_step()
        torch.cuda.synchronize()
        lv = eng.loss_values()
        assert np.isfinite(lv["loss"]) and lv["mlm_loss"] > 0 and lv["mvrc_loss"] == 0.0, lv
        assert abs(lv["mlm_loss"] - plain.loss_values()["mlm_loss"]) <= 1e-5 * lv["mlm_loss"]
        n = plain.P.numel
        err = float((eng.P.grad[:n].double() - plain.P.grad.double()).norm() / plain.P.grad.double().norm())
        print("dp world 1 (%s): loss %.5f, local gradient vs the no-exchange step: rel %.3e" % (mode, lv["loss"], err))
        assert err <= 1e-3 and bool(torch.isfinite(eng.P.master).all())      # (float atomics: not bit for bit run to run)
        eng.train_step()
        torch.cuda.synchronize()
        assert np.isfinite(eng.loss_values()["loss"])
    dist.destroy_process_group()
    print("OBJECTIVES CHILD OK: dp_world1")


if __name__ == "__main__":
    {"f16_dynamic": _child_f16_dynamic, "dp_world1": _child_dp_world1}[sys.argv[1]]()
