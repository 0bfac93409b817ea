"""Validation on the device (-m gpu): the forward-only loss + accuracy kernels (vl-bert_amd/csrc/metrics.hip) against their numpy
restatement (tests/metrics_ref.py, itself pinned to the reference's metric classes by tests/test_metrics_cpu.py) on the same 16-bit
logits, their loss values against the fused forward+backward kernels of csrc/loss.hip, PretrainEngine.eval_step() against its own
logits, forward(train=False) and the fp32 oracle, its non-interference with the training state, and the entry point's validation
lines."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import vlbert_oracle as O
from tests import metrics_ref as MR
from tests.gpu_util import act_dtype, dev, pkg

pytestmark = pytest.mark.gpu

# Largest relative difference between the loss of an eval kernel and of the fused forward+backward kernel on the same logits.  Both
# take the row's log-sum-exp in fp32 with __expf / __logf but merge the (max, sum) pairs in a different order, and the mean is one
# division of an atomic sum here, a sum of divided rows there.  Measured on MI355X (bf16 build) over every comparison of this file
# (53 of them): 1.53e-7, one fp32 ulp of a loss around 6; asserted with the 4x margin for reduction-order differences.
LOSS_REL_MEASURED = 1.53e-7
LOSS_REL_TOL = 4 * LOSS_REL_MEASURED


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def check_loss(tag, got, ref):
    print("%s: eval %.9g fused %.9g rel diff %.3e (bar %.1e)" % (tag, got, ref, rel(got, ref), LOSS_REL_TOL))
    assert rel(got, ref) <= LOSS_REL_TOL, (tag, got, ref)


def to16(x):
    return torch.from_numpy(x).to(act_dtype()).to(dev())


def plant_ties(x, labels, V):
    """Row maximum (8.0, above the rest of the row) twice in one row.  Rows 0 / 1: columns 7 | 8, the last of thread 0's and the first
    of thread 1's 8-column range (label on the second occurrence = a miss, on the first = a hit).  V > 512, rows 2 / 3: columns
    511 | 512, the last of wave 0's and the first of wave 1's; rows 4 / 5: columns 5 | 2053, one thread's first and second chunk."""
    pairs = [(7, 8)] if V > 8 else [(0, 1)]
    if V > 512:
        pairs.append((511, 512))
    if V > 2053:
        pairs.append((5, 2053))
    want = []
    for k, (a, b) in enumerate(pairs):
        for j, lab in enumerate((b, a)):
            r = 2 * k + j
            x[r, :V] = np.minimum(x[r, :V], 7.875)
            x[r, a] = x[r, b] = 8.0
            labels[r] = lab
            want.append((r, a, lab == a))
    return want


CE_CASES = [(2, 64), (37, 40), (1601, 1664), (30522, 30528)]      # (V, ld): one element per wave and below; odd, under one block; the MVRC
#                                                                  width; the MLM vocabulary with the engine's padded ld (V rounded up to 64)


@pytest.mark.parametrize("negative", [False, True], ids=["grid", "all_negative_zero_padding"])
@pytest.mark.parametrize("V,ld", CE_CASES)
def test_ce_eval_matches_the_restatement_and_the_fused_loss(V, ld, negative):
    ops = pkg("ops")
    rng = np.random.RandomState(V + negative)
    rows = 12
    x = MR.grid_logits(rng, (rows, ld), -8.0, -0.125) if negative else MR.grid_logits(rng, (rows, ld))
    x[:, V:] = 0.0 if negative else 8.0                     # padding that would win the max if it were read
    labels = rng.randint(0, V, rows).astype(np.int64)
    ties = [] if negative else plant_ties(x, labels, V)
    labels[[6, 9]] = -1                                     # interleaved unlabelled rows
    ref = MR.ce_eval_ref(x, V, labels)
    for r, col, hit in ties:
        assert ref["pred"][r] == col and (ref["pred"][r] == labels[r]) == hit
    logits = to16(x)
    assert np.array_equal(logits.float().cpu().numpy(), x)  # the grid is exact in the 16-bit type
    before = logits.clone()
    lab = torch.from_numpy(labels).to(dev())
    # ---- one group, the kernel counts the labelled rows itself ----
    loss = torch.full((1,), 0.5, dtype=torch.float32, device=dev())
    acc = torch.tensor([10, 20], dtype=torch.int64, device=dev())
    pred = torch.full((rows,), -7, dtype=torch.int32, device=dev())
    ops.ce_eval(logits, V, lab, loss, acc, pred=pred)
    torch.cuda.synchronize()
    assert torch.equal(logits.view(torch.int16), before.view(torch.int16))
    assert acc.tolist() == [10 + ref["hits"], 20 + ref["n"]] and np.array_equal(pred.cpu().numpy(), ref["pred"])
    assert abs(float(loss) - 0.5 - ref["loss"]) <= 1e-5 * ref["loss"]
    fused = torch.zeros(1, dtype=torch.float32, device=dev())
    ops.ce_fwd_bwd(before.clone(), V, lab, torch.zeros(1, dtype=torch.float32, device=dev()), fused)
    one = torch.zeros(1, dtype=torch.float32, device=dev())
    ops.ce_eval(logits, V, lab, one, acc)
    torch.cuda.synchronize()
    assert acc.tolist() == [10 + 2 * ref["hits"], 20 + 2 * ref["n"]]          # accumulated
    check_loss("ce_eval V=%d one group" % V, float(one), float(fused))
    # ---- two groups over compacted rows: n0 rows of group 0, n1 of group 1, unlabelled rows behind them ----
    order = np.concatenate((np.flatnonzero(labels >= 0), np.flatnonzero(labels < 0)))
    xc, lc = x[order], labels[order]
    n0, n1 = 4, int((labels >= 0).sum()) - 4
    r0, r1 = MR.ce_eval_ref(xc[:n0], V, lc[:n0]), MR.ce_eval_ref(xc[n0:], V, lc[n0:])
    lg, lb = to16(xc), torch.from_numpy(lc).to(dev())
    counts = torch.tensor([n0, n1], dtype=torch.float32, device=dev())
    l2 = torch.zeros(2, dtype=torch.float32, device=dev())
    a2 = torch.zeros((2, 2), dtype=torch.int64, device=dev())
    p2 = torch.zeros(rows, dtype=torch.int32, device=dev())
    ops.ce_eval(lg, V, lb, l2[0:1], a2[0], count0=counts[0:1], count1=counts[1:2], loss_out1=l2[1:2], acc1=a2[1], pred=p2)
    f2 = torch.zeros(2, dtype=torch.float32, device=dev())
    ops.ce_fwd_bwd_compact(lg.clone(), V, lb, counts[0:1], counts[1:2], f2[0:1], f2[1:2])
    torch.cuda.synchronize()
    assert torch.equal(lg.view(torch.int16), to16(xc).view(torch.int16))
    assert a2.tolist() == [[r0["hits"], r0["n"]], [r1["hits"], r1["n"]]] and [r0["n"], r1["n"]] == [n0, n1]
    assert np.array_equal(p2.cpu().numpy(), np.concatenate((r0["pred"], r1["pred"])))
    check_loss("ce_eval V=%d group 0" % V, float(l2[0]), float(f2[0]))
    check_loss("ce_eval V=%d group 1" % V, float(l2[1]), float(f2[1]))


def test_ce_eval_without_a_labelled_row_touches_nothing():
    ops = pkg("ops")
    V, ld, rows = 37, 40, 8
    logits = to16(MR.grid_logits(np.random.RandomState(1), (rows, ld)))
    lab = torch.full((rows,), -1, dtype=torch.int64, device=dev())
    loss = torch.full((2,), 3.25, dtype=torch.float32, device=dev())
    acc = torch.tensor([[5, 7], [1, 2]], dtype=torch.int64, device=dev())
    pred = torch.zeros(rows, dtype=torch.int32, device=dev())
    ops.ce_eval(logits, V, lab, loss[0:1], acc[0], pred=pred)
    zero = torch.zeros(2, dtype=torch.float32, device=dev())
    ops.ce_eval(logits, V, lab, loss[0:1], acc[0], count0=zero[0:1], count1=zero[1:2], loss_out1=loss[1:2], acc1=acc[1])
    target = torch.zeros((rows, 11), dtype=torch.float32, device=dev())
    ops.soft_ce_eval(logits, 11, target, loss[1:2], acc[1])
    torch.cuda.synchronize()
    assert loss.tolist() == [3.25, 3.25] and acc.tolist() == [[5, 7], [1, 2]] and pred.tolist() == [-1] * rows


@pytest.mark.parametrize("C,ld", [(50, 64), (1601, 1664)])
def test_soft_ce_eval_matches_the_restatement_and_the_fused_loss(C, ld):
    ops = pkg("ops")
    rng = np.random.RandomState(C)
    rows = 12
    x = MR.grid_logits(rng, (rows, ld))
    x[:, C:] = 8.0
    t = rng.dirichlet(np.ones(C) * 0.2, rows).astype(np.float32)
    t[3] = 0.0                                               # invalid: sum 0
    t[4] *= 1.2                                              # invalid: sum 1.2
    t[5] = 0.0
    t[5, [9, 30]] = 0.5                                      # tie in the target: argmax 9 ...
    x[5, :C] = np.minimum(x[5, :C], 7.875)
    x[5, [9, 40]] = 8.0                                      # ... and in the logits: argmax 9 -> a hit
    # ties of the row maximum across two threads of different waves (63 | 64) and across one thread's two columns (3 | 259)
    pairs = [(6, 0, 1)] + ([(7, 63, 64), (8, 3, 259)] if C > 259 else [])
    for r, a, b in pairs:
        x[r, :C] = np.minimum(x[r, :C], 7.875)
        x[r, a] = x[r, b] = 8.0
        t[r] = 0.0
        t[r, b] = 1.0                                        # target on the second occurrence: a miss
    ref = MR.soft_ce_eval_ref(x, C, t)
    assert ref["n"] == rows - 2 and not ref["valid"][3] and not ref["valid"][4]
    assert (x[5, :C].argmax(), t[5].argmax()) == (9, 9) and all(x[r, :C].argmax() == a for r, a, b in pairs)
    logits, target = to16(x), torch.from_numpy(t).to(dev())
    before = logits.clone()
    loss = torch.zeros(1, dtype=torch.float32, device=dev())
    acc = torch.tensor([3, 4], dtype=torch.int64, device=dev())
    ops.soft_ce_eval(logits, C, target, loss, acc)
    fused = torch.zeros(1, dtype=torch.float32, device=dev())
    ops.soft_ce_fwd_bwd(before.clone(), C, target, torch.zeros(rows, dtype=torch.float32, device=dev()),
                        torch.zeros(1, dtype=torch.float32, device=dev()), fused)
    torch.cuda.synchronize()
    assert torch.equal(logits.view(torch.int16), before.view(torch.int16))
    assert acc.tolist() == [3 + ref["hits"], 4 + ref["n"]]
    assert abs(float(loss) - ref["loss"]) <= 1e-5 * ref["loss"]
    check_loss("soft_ce_eval C=%d" % C, float(loss), float(fused))


# ---- eval_step on the small model ---------------------------------------------------------------------------------------------
def small_case(name):
    """Small-fixture dimensions (tests/golden/multitask_small.npz / full_rel.npz: hidden 128, 2-3 layers, V = 512, C = 50 / 40) on
    synthetic ragged batches with enough labelled rows for the margin statistics below.  aux: multitask with text-only rows,
    B*T <= 256 so the MLM head runs on every row; compact: B*T = 640, the head runs on the compacted labelled rows; rel: pooler +
    relationship head.  Seeds chosen on the CPU (oracle alone, bf16-rounded weights as the stand-in for the engine): at most
    22 % of a head's rows have a top-1 / top-2 margin within four times that stand-in's logits error."""
    syn = pkg("synthetic")
    if name == "rel":
        cfg = O.VLBertConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=384, vocab_size=512,
                             max_position_embeddings=64, visual_region_classes=40, with_pooler=True, with_rel_loss=True)
        B, T, R, Ba, pseed, bseed = 4, 32, 6, 0, 44, 54
    else:
        cfg = O.VLBertConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=512,
                             max_position_embeddings=64 if name == "aux" else 128, visual_region_classes=50, multitask=True)
        B, T, R, Ba, pseed, bseed = (4, 32, 6, 3, 41, 51) if name == "aux" else (6, 64, 12, 4, 44, 54)
    for k in ("hidden_dropout_prob", "attention_probs_dropout_prob", "obj_downsample_dropout"):
        assert getattr(cfg, k) > 0                           # eval_step must switch them off itself
    params = O.init_params(cfg, seed=pseed)
    batch = tuple(syn.make_batch(B, T, R, vocab_size=512, region_classes=cfg.visual_region_classes, seed=bseed, ragged=True))
    if Ba:
        batch += tuple(syn.make_aux_text(Ba, T, vocab_size=512, seed=bseed + 1))
    return cfg, params, batch, (B, T, R, Ba)


def small_engine(name, train=True):
    cfg, params, batch, (B, T, R, Ba) = small_case(name)
    E = pkg("engine")
    mc = E.ModelConfig(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                       intermediate_size=cfg.intermediate_size, vocab_size=cfg.vocab_size, max_position_embeddings=cfg.max_position_embeddings,
                       visual_region_classes=cfg.visual_region_classes, hidden_dropout_prob=cfg.hidden_dropout_prob,
                       attention_probs_dropout_prob=cfg.attention_probs_dropout_prob, obj_downsample_dropout=cfg.obj_downsample_dropout,
                       multitask=cfg.multitask, with_pooler=cfg.with_pooler, with_rel_loss=cfg.with_rel_loss)
    eng = E.PretrainEngine(mc, B, T, R, device="cuda:0", train=train, B_aux=Ba)
    assert (eng.mlm_cap is not None) == (name == "compact")
    eng.load_state_dict({k: v.to(dev()) for k, v in params.items()})
    eng.set_batch(*[t.to(dev()) for t in batch])
    return eng, cfg, params, batch


def engine_heads(eng, cfg):
    """{head: (logits [rows, V] fp32 numpy as the kernels read them, labels / soft targets, source position of every row)} read back
    from the engine's own buffers after eval_step()."""
    V, C, nw = cfg.vocab_size, cfg.visual_region_classes, eng.B * eng.T
    out = {}
    if eng._mlm_compact_now:
        pos = eng.sel_pos.cpu().numpy()
        lab = eng.labels_c.cpu().numpy()
        lg = eng.mlm_logits[:eng.mlm_cap].float().cpu().numpy()
        n0 = int(eng.counts[0])
        rows = np.arange(len(pos))
        g0, g1 = (rows < n0) & (lab >= 0), (rows >= n0) & (lab >= 0)
        out["mlm"] = (lg[g0], lab[g0], pos[g0])
        out["mlm_aux"] = (lg[g1], lab[g1], pos[g1] - nw)
    else:
        lab = eng.in_mlm_labels.view(-1).cpu().numpy()
        lg = eng.mlm_logits[:eng.BT].float().cpu().numpy()
        out["mlm"] = (lg[:nw], lab[:nw], np.arange(nw))
        if eng.Ba:
            out["mlm_aux"] = (lg[nw:], lab[nw:], np.arange(eng.BT - nw))
    out["mvrc"] = (eng.mvrc_logits.float().cpu().numpy(), eng.in_mvrc_labels.view(eng.BR, C).cpu().numpy(), np.arange(eng.BR))
    if cfg.with_rel_loss:
        out["relationship"] = (eng.rel_logits.float().cpu().numpy(), eng.in_rel_label.cpu().numpy(), np.arange(eng.B))
    return out


@pytest.mark.parametrize("name", ["aux", "compact", "rel"])
def test_eval_step_counters_losses_and_predictions(name):
    eng, cfg, params, batch = small_engine(name)
    V, C = cfg.vocab_size, cfg.visual_region_classes
    eng.eval_step()
    torch.cuda.synchronize()
    counts, lv = eng.metric_counts(), eng.loss_values()
    heads = engine_heads(eng, cfg)
    # (1) counters == the restatement on the engine's own logits, exactly
    refs = {}
    for k, (lg, lab, pos) in heads.items():
        refs[k] = MR.soft_ce_eval_ref(lg, C, lab) if k == "mvrc" else MR.ce_eval_ref(lg, 2 if k == "relationship" else V, lab)
        print("%s %s: device [hits, n] %s, restatement [%d, %d]" % (name, k, list(counts[k]), refs[k]["hits"], refs[k]["n"]))
        assert counts[k] == (refs[k]["hits"], refs[k]["n"]), k
        assert refs[k]["n"] > 0
    for k in set(counts) - set(heads):
        assert counts[k] == (0, 0), k
    # (2) losses == forward(train=False) on the same batch
    eng.forward(train=False)
    torch.cuda.synchronize()
    fw = eng.loss_values()
    for k in sorted(fw):
        if fw[k] != 0.0 or lv[k] != 0.0:
            check_loss("%s eval_step %s vs forward(train=False)" % (name, k), lv[k], fw[k])
    assert eng.metric_counts() == counts                     # a forward leaves the counters alone
    # (3) predictions vs the fp32 oracle wherever its top-1 / top-2 margin exceeds twice the logits error of this run
    outputs = O.loss_and_grads(params, cfg, batch, train=False)[0]
    B, T = eng.B, eng.T
    oracle = {}
    if cfg.multitask:
        oracle["mlm"] = outputs["mlm_logits_wvc"].detach()
        oracle["mlm_aux"] = outputs["mlm_logits_aux"].detach()
    else:
        oracle["mlm"] = outputs["mlm_logits"].detach()
    full = {}
    for k, x in oracle.items():                              # the oracle trims to the longest text: back to the engine's T columns
        pad = torch.zeros((x.shape[0], T, V))
        pad[:, :x.shape[1]] = x
        full[k] = pad.reshape(-1, V).numpy()
    mv = outputs["mvrc_logits"].detach()
    pad = torch.zeros((B, eng.R, C))
    pad[:, :mv.shape[1]] = mv
    full["mvrc"] = pad.reshape(-1, C).numpy()
    if cfg.with_rel_loss:
        full["relationship"] = outputs["relationship_logits"].detach().numpy()
    for k, (lg, lab, pos) in heads.items():
        width = C if k == "mvrc" else (2 if k == "relationship" else V)
        keep = refs[k]["valid"] if k == "mvrc" else ((lab >= 0) & (lab < width))
        got, ref = lg[keep][:, :width], full[k][pos[keep]]
        e = float(np.abs(got - ref).max())
        bound = 2e-3 + 1e-2 * float(np.abs(ref).max())       # what the small-model logits tests assert (tests/test_engine_gpu.py)
        top2 = np.sort(ref, axis=1)[:, -2:]
        margin = top2[:, 1] - top2[:, 0]
        sure = margin > 2 * e
        agree = got.argmax(1)[sure] == ref.argmax(1)[sure]
        print("%s %s: %d rows, logits error e %.3e (bound %.3e), %d rows with an oracle margin <= 2e left out, %d / %d predictions agree"
              % (name, k, len(margin), e, bound, int((~sure).sum()), int(agree.sum()), int(sure.sum())))
        assert e <= bound, (k, e, bound)
        assert (~sure).sum() <= len(margin) / 4, (k, int((~sure).sum()), len(margin))
        assert agree.all(), k


def test_eval_step_leaves_the_training_state_alone_and_accumulates():
    eng, cfg, params, batch = small_engine("compact")
    eng.train_step()                                          # non-trivial gradients, moments, step counter and an advanced seed
    torch.cuda.synchronize()
    state = lambda: [t.clone() for t in (eng.seed, eng.P.grad, eng.P.master, eng.P.m, eng.P.v, eng.adam, eng.P.w16)]
    snap = state()
    eng.eval_step()
    torch.cuda.synchronize()
    once, loss_once = eng.metric_acc.clone(), eng.losses.clone()
    eng.eval_step()
    torch.cuda.synchronize()
    for a, b, what in zip(snap, state(), ("seed", "grad", "master", "m", "v", "adam (lr, step counter, norm)", "w16")):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), what
    assert int(once.sum()) > 0 and torch.equal(eng.metric_acc, 2 * once)
    assert torch.allclose(eng.losses, loss_once, rtol=LOSS_REL_TOL, atol=0)       # the slots are written, not accumulated
    eng.reset_metrics()
    assert eng.metric_counts() == {k: (0, 0) for k in eng.METRIC_ROWS}


def test_train_end2end_validates_at_every_epoch_end(capsys):
    """--val-steps on synthetic batches.  tests/fixtures/pretrain_small.yaml accumulates 2 micro-batches per optimizer step, so
    --steps-per-epoch 2 is ONE optimizer step per epoch and --steps 4 ends four epochs: four validation lines (the two the issue
    names, and two more).  The --data variant is left out: the cc_tiny configuration names no validation set."""
    tr = pkg("pretrain.train_end2end")
    cfg = os.path.join(os.path.dirname(__file__), "fixtures", "pretrain_small.yaml")
    eng = tr.main(["--cfg", cfg, "--steps", "4", "--steps-per-epoch", "2", "--val-steps", "2", "--text-len", "32", "--regions", "10"])
    torch.cuda.synchronize()
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Epoch[")]
    assert len(lines) == 4 and len(lines) >= 2, out
    for k, l in enumerate(lines):
        m = re.fullmatch(r"Epoch\[%d\] \tVal-((?:\w+=[-\w.]+,\t)+)" % k, l)
        assert m, l
        pairs = [p.split("=") for p in m.group(1).split(",\t") if p]
        assert [p[0] for p in pairs] == ["MLMAcc", "MVRCAccuracy", "RelLoss", "MLMLoss", "MVRCLoss"], l
        vals = dict((a, float(b)) for a, b in pairs)
        assert 0.0 <= vals["MLMAcc"] <= 1.0 and 0.0 <= vals["MVRCAccuracy"] <= 1.0 and vals["MLMLoss"] > 0 and vals["MVRCLoss"] > 0
        assert vals["RelLoss"] == 0.0
    best = [l for l in out.splitlines() if l.startswith("Best Val MLMAcc: ")]
    assert len(best) == 4
    mon = eng.validation_monitor
    assert math.isfinite(mon.best_val) and 0.0 <= mon.best_val <= 1.0 and 0 <= mon.best_epoch <= 3
    assert best[-1] == "Best Val MLMAcc: {}, Epoch: {}".format(mon.best_val, mon.best_epoch)
    assert float(eng.adam[5]) == 4.0                         # four optimizer steps: validation did not move the step counter
