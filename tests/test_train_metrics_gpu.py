"""Training-time metrics on the device (-m gpu): the ACC forms of the fused forward+backward loss kernels (csrc/loss.hip,
csrc/f32_pretrain.hip) against the plain entry points on the same input (gradient, kept copy and loss) and against the restatement
of tests/metrics_ref.py and the validation kernels (counters); PretrainEngine(train_metrics=True) against a host restatement on
logits cloned before the losses overwrite them (tests/train_metrics_ref.py); the metric classes over train_metrics_source; the entry
point's Train- line.

Inputs lie on metrics_ref.grid_logits (multiples of 1/8 in [-8, 8]: exact in bf16 and fp16), soft-target rows sum to exactly 0, 0.5
or 1, pad columns hold +64 (they would win every argmax if they were read).  Tests whose name holds `kernel` are the ones the fp16
child of test_fp16_build_runs_the_kernel_tests runs again on the other build."""
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import torch

from tests import metrics_ref as MR
from tests import train_metrics_ref as TR
from tests.gpu_util import REPORT, act_dtype, dev, pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64.0
FORMS = ["16", "f32"]          # 16-bit logits (loss.hip) | fp32 logits (f32_pretrain.hip)


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def lg(form, x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    t = t.to(act_dtype()) if form == "16" else t
    assert np.array_equal(t.float().numpy(), x)              # the grid (and the pad value) is exact in the type under test
    return t.to(dev())


def zf(n, v=0.0):
    return torch.full((n,), v, dtype=torch.float32, device=dev())


def counters(a=7, b=11):
    return torch.tensor([a, b], dtype=torch.int64, device=dev())


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def ld_of(form, V):
    return (V + 7) // 8 * 8 if form == "16" else (V + 3) // 4 * 4


def grid(rng, rows, V, ld):
    x = MR.grid_logits(rng, (rows, ld))
    x[:, V:] = PAD
    return x


def check_loss(form, got, ref, tag):
    """16-bit losses are float atomic sums (the same up to summation order: 1e-6 relative); the fp32 ones have a fixed order."""
    got, ref = float(got), float(ref)
    print("%s: loss %.9g, plain entry point %.9g" % (tag, got, ref))
    if form == "16":
        assert abs(got - ref) <= 1e-6 * abs(ref), (tag, got, ref)
    else:
        assert got == ref, (tag, got, ref)


def run_ce(form, x, V, labels, gscale=0.5, acc=None, dscale=None, copy=True):
    ops = pkg("ops")
    logits, lab = lg(form, x), torch.from_numpy(labels).to(dev())
    counts, loss = zf(1), zf(1)
    cp = torch.zeros_like(logits) if copy else None
    kw = dict(kv for kv in (("acc", acc), ("dscale", dscale)) if kv[1] is not None)
    (ops.ce_fwd_bwd if form == "16" else ops.ce_f32_fwd_bwd)(logits, V, lab, counts, loss, gscale=gscale, logits_copy=cp, **kw)
    torch.cuda.synchronize()
    return logits, cp, loss, counts


def run_compact(form, x, V, labels_c, n0, n1, gscale=0.5, acc=None, dscale=None):
    ops = pkg("ops")
    logits, lab = lg(form, x), torch.from_numpy(labels_c).to(dev())
    counts = torch.tensor([n0, n1], dtype=torch.float32, device=dev())
    loss = zf(2)
    kw = dict(acc=acc[0], acc1=acc[1]) if acc is not None else {}
    if dscale is not None:
        kw["dscale"] = dscale
    (ops.ce_fwd_bwd_compact if form == "16" else ops.ce_f32_fwd_bwd_compact)(logits, V, lab, counts[0:1], counts[1:2], loss[0:1], loss[1:2],
                                                                             gscale=gscale, **kw)
    torch.cuda.synchronize()
    return logits, loss


def run_soft(form, x, C, t, gscale=0.5, acc=None, dscale=None):
    ops = pkg("ops")
    logits, target = lg(form, x), torch.from_numpy(t).to(dev())
    tsum, counts, loss = zf(x.shape[0]), zf(1), zf(1)
    cp = torch.zeros_like(logits)
    kw = dict(kv for kv in (("acc", acc), ("dscale", dscale)) if kv[1] is not None)
    (ops.soft_ce_fwd_bwd if form == "16" else ops.soft_ce_f32_fwd_bwd)(logits, C, target, tsum, counts, loss, gscale=gscale, logits_copy=cp, **kw)
    torch.cuda.synchronize()
    return logits, cp, loss, counts


def mixed_labels(rng, rows, V):
    """Valid labels with -1, other negative and >= V ones in between (rows >= 5); one valid row at rows == 1."""
    lab = rng.randint(0, V, rows).astype(np.int64)
    if rows >= 5:
        lab[1], lab[2] = -1, V + 3
    if rows >= 70:
        lab[rng.choice(np.arange(5, rows), 25, replace=False)] = -1
        lab[[8, 33]] = V, -100
        lab[0] = -1                                            # block 0's own row is unlabelled
    return lab


# ---- hard labels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("V", [2, 37, 30522])
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_kernel_hard_ce_counts_and_leaves_the_fused_loss_alone(rows, V, form):
    ops = pkg("ops")
    ld = ld_of(form, V)
    assert form != "16" or ld == {2: 8, 37: 40, 30522: 30528}[V]
    rng = np.random.RandomState(rows * 1000 + V % 997)
    x, labels = grid(rng, rows, V, ld), mixed_labels(rng, rows, V)
    ref = MR.ce_eval_ref(x, V, labels)
    g0, c0, l0, n0 = run_ce(form, x, V, labels)
    acc = counters()
    g1, c1, l1, n1 = run_ce(form, x, V, labels, acc=acc)
    assert same_bits(g1, g0) and same_bits(c1, c0) and same_bits(n1, n0)
    assert float(g1[:, V:].abs().max()) == 0.0                # pad columns zeroed
    check_loss(form, l1, l0, "hard CE %s rows %d V %d" % (form, rows, V))
    print("acc %s, restatement [%d, %d]" % (acc.tolist(), ref["hits"], ref["n"]))
    assert acc.tolist() == [7 + ref["hits"], 11 + ref["n"]]
    if form == "16":                                           # ... and exactly what the validation kernel counts on the same logits
        ev = counters()
        ops.ce_eval(lg(form, x), V, torch.from_numpy(labels).to(dev()), zf(1), ev)
        torch.cuda.synchronize()
        assert ev.tolist() == acc.tolist()
    run_ce(form, x, V, labels, acc=acc)                        # a second call accumulates
    assert acc.tolist() == [7 + 2 * ref["hits"], 11 + 2 * ref["n"]]


def tie_rows(form, V):
    """[(columns holding the row maximum, label, hit?)]: the maximum twice at j < k with the label on j (a hit) and on k (a miss) --
    far apart, inside one vector of a thread, in neighbouring threads, in two waves, in two loop iterations of one thread -- and the
    maximum alone in the last, partial vector (column V - 1)."""
    w = 8 if form == "16" else 4                               # columns per thread and iteration; a wave covers 64 w, the block 256 w
    pairs = [(1, 30), (2 * w, 2 * w + 3), (3 * w, 4 * w), (100, 200), (5 * w, 5 * w + 64 * w), (5, 5 + 256 * w)]
    assert 5 + 256 * w == (2053 if form == "16" else 1029) and 5 * w + 64 * w == (552 if form == "16" else 276)
    out = []
    for j, k in pairs:
        if k < V:
            out += [((j, k), j, True), ((j, k), k, False)]
    assert V % w != 0
    out.append(((V - 1,), V - 1, True))
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("V", [37, 30522])
def test_kernel_hard_ce_ties_go_to_the_lowest_column_and_pads_are_ignored(V, form):
    ld = ld_of(form, V)
    cases = tie_rows(form, V)
    assert len(cases) == (13 if V == 30522 else 7)
    rng = np.random.RandomState(V)
    x = np.minimum(grid(rng, len(cases), V, ld), 7.875)
    x[:, V:] = PAD
    labels = np.zeros(len(cases), dtype=np.int64)
    for r, (cols, lab, hit) in enumerate(cases):
        x[r, list(cols)] = 8.0
        labels[r] = lab
    ref = MR.ce_eval_ref(x, V, labels)
    assert [int(p) for p in ref["pred"]] == [c[0][0] for c in cases] and ref["hits"] == sum(c[2] for c in cases)
    g0, c0, l0, _ = run_ce(form, x, V, labels)
    # row by row, so that a wrong tie rule names its row
    for r, (cols, lab, hit) in enumerate(cases):
        acc = counters(0, 0)
        run_ce(form, x[r:r + 1], V, labels[r:r + 1], acc=acc, copy=False)
        assert acc.tolist() == [int(hit), 1], (form, V, cols, lab, acc.tolist())
    acc = counters(0, 0)
    g1, c1, l1, _ = run_ce(form, x, V, labels, acc=acc)
    assert acc.tolist() == [ref["hits"], len(cases)] and same_bits(g1, g0) and same_bits(c1, c0)
    check_loss(form, l1, l0, "tie rows %s V %d" % (form, V))


@pytest.mark.parametrize("form", FORMS)
def test_kernel_hard_ce_unlabelled_first_row_and_no_labelled_row(form):
    V, rows = 37, 6
    ld = ld_of(form, V)
    x = grid(np.random.RandomState(3), rows, V, ld)
    labels = np.array([-1, 4, 9, -1, 36, V], dtype=np.int64)   # block 0's row is unlabelled, three rows count
    ref = MR.ce_eval_ref(x, V, labels)
    acc = counters()
    run_ce(form, x, V, labels, acc=acc)
    assert ref["n"] == 3 and acc.tolist() == [7 + ref["hits"], 11 + 3]
    g0, _, l0, _ = run_ce(form, x, V, np.full(rows, -1, dtype=np.int64))
    g1, _, l1, _ = run_ce(form, x, V, np.full(rows, -1, dtype=np.int64), acc=acc)
    assert acc.tolist() == [7 + ref["hits"], 11 + 3] and float(l1) == 0.0 == float(l0) and same_bits(g1, g0) and float(g1.abs().max()) == 0.0
    # two-group form with both groups empty: block 0's row is unlabelled padding
    a2 = torch.tensor([[1, 2], [3, 4]], dtype=torch.int64, device=dev())
    g2, l2 = run_compact(form, x, V, np.full(rows, -1, dtype=np.int64), 0, 0, acc=a2)
    assert a2.tolist() == [[1, 2], [3, 4]] and l2.tolist() == [0.0, 0.0] and float(g2.abs().max()) == 0.0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows,V", [(70, 37), (5, 30522)])
@pytest.mark.parametrize("n0,n1", [(0, 3), (3, 0), (2, 2)])
def test_kernel_two_group_form_counts_each_group(n0, n1, rows, V, form):
    ops = pkg("ops")
    ld = ld_of(form, V)
    rng = np.random.RandomState(V + 10 * n0 + n1)
    x = np.minimum(grid(rng, rows, V, ld), 7.875)
    x[:, V:] = PAD
    labels = np.full(rows, -1, dtype=np.int64)                 # compacted rows: group 0, group 1, unlabelled padding behind them
    labels[:n0 + n1] = rng.randint(0, V, n0 + n1)
    x[0, labels[0]] = 8.0                                      # at least one hit, in whichever group row 0 belongs to ...
    other = (labels[n0 + n1 - 1] + 1) % V
    x[n0 + n1 - 1, other] = 8.0                                # ... and a miss in the last labelled row
    r0, r1 = MR.ce_eval_ref(x[:n0], V, labels[:n0]), MR.ce_eval_ref(x[n0:], V, labels[n0:])
    assert (r0["n"], r1["n"]) == (n0, n1) and r0["hits"] + r1["hits"] >= 1
    g0, l0 = run_compact(form, x, V, labels, n0, n1)
    acc = torch.tensor([[5, 6], [7, 8]], dtype=torch.int64, device=dev())
    g1, l1 = run_compact(form, x, V, labels, n0, n1, acc=acc)
    assert same_bits(g1, g0) and float(g1[:, V:].abs().max()) == 0.0
    for k in (0, 1):
        check_loss(form, l1[k], l0[k], "two-group %s (%d, %d) rows %d V %d group %d" % (form, n0, n1, rows, V, k))
    assert acc.tolist() == [[5 + r0["hits"], 6 + n0], [7 + r1["hits"], 8 + n1]]
    if form == "16":
        ev = torch.tensor([[5, 6], [7, 8]], dtype=torch.int64, device=dev())
        counts = torch.tensor([n0, n1], dtype=torch.float32, device=dev())
        ops.ce_eval(lg(form, x), V, torch.from_numpy(labels).to(dev()), zf(1), ev[0], count0=counts[0:1], count1=counts[1:2], loss_out1=zf(1), acc1=ev[1])
        torch.cuda.synchronize()
        assert ev.tolist() == acc.tolist()


# ---- soft labels ----------------------------------------------------------------------------------------------------------------
def soft_case(rng, rows, C, ld):
    """rows == 7: row 0 invalid (sum 0: block 0's own row), 1 a one-hot hit, 2 invalid (sum 0.5), 3 a 0.5 / 0.5 target tie whose lower
    column is the logits' argmax (hit), 4 / 5 a logits tie with the target on the upper (miss) / lower (hit) column, 6 a 0.25 / 0.75
    target on random columns.  rows == 1: the target tie alone."""
    x = np.minimum(MR.grid_logits(rng, (rows, ld)), 7.875)
    x[:, C:] = PAD
    t = np.zeros((rows, C), dtype=np.float32)
    a, b = (3, 259) if C > 259 else (1, 3)                    # one thread's first and second column at C = 1601
    c, d = (63, 64) if C > 64 else (2, 4)                      # two waves at C = 1601
    if rows == 1:
        t[0, [a, b]] = 0.5
        x[0, a] = 8.0
        return x, t
    x[1, 2], t[1, 2] = 8.0, 1.0
    t[2, 0] = 0.5
    t[3, [a, b]] = 0.5
    x[3, a] = 8.0
    x[4, [c, d]], t[4, d] = 8.0, 1.0
    x[5, [a, b]], t[5, a] = 8.0, 1.0
    p, q = rng.choice(C, 2, replace=False)
    t[6, p], t[6, q] = 0.25, 0.75
    return x, t


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C", [5, 1601])
@pytest.mark.parametrize("rows", [1, 7])
def test_kernel_soft_ce_counts_and_leaves_the_fused_loss_alone(rows, C, form):
    ops = pkg("ops")
    ld = ld_of(form, C)
    x, t = soft_case(np.random.RandomState(C + rows), rows, C, ld)
    ref = MR.soft_ce_eval_ref(x, C, t)
    if rows == 7:
        assert ref["n"] == 5 and not ref["valid"][0] and not ref["valid"][2]
        hits = [bool(x[r, :C].argmax() == t[r].argmax()) for r in (1, 3, 4, 5)]
        assert hits == [True, True, False, True]
    else:
        assert (ref["hits"], ref["n"]) == (1, 1)
    g0, c0, l0, n0 = run_soft(form, x, C, t)
    acc = counters()
    g1, c1, l1, n1 = run_soft(form, x, C, t, acc=acc)
    assert same_bits(g1, g0) and same_bits(c1, c0) and same_bits(n1, n0)
    assert float(g1[:, C:].abs().max()) == 0.0 and float(g1[~torch.from_numpy(ref["valid"]).to(dev())].abs().sum()) == 0.0
    check_loss(form, l1, l0, "soft CE %s rows %d C %d" % (form, rows, C))
    print("acc %s, restatement [%d, %d]" % (acc.tolist(), ref["hits"], ref["n"]))
    assert acc.tolist() == [7 + ref["hits"], 11 + ref["n"]]
    if form == "16":
        ev = counters()
        ops.soft_ce_eval(lg(form, x), C, torch.from_numpy(t).to(dev()), zf(1), ev)
        torch.cuda.synchronize()
        assert ev.tolist() == acc.tolist()
    run_soft(form, x, C, t, acc=acc)
    assert acc.tolist() == [7 + 2 * ref["hits"], 11 + 2 * ref["n"]]


# ---- logits off the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_kernel_bits_of_the_plain_form_on_logits_off_the_grid(form):
    """Beyond the grid batteries: normal logits rounded to the type under test, enough rows that a row sum-exp differing in its last
    bit from the plain kernel's shows as a flipped 16-bit gradient (the build contracts a * b + c * d into one fused multiply-add
    and chooses the product per inlined copy: csrc/loss.hip, block_online_reduce_as_plain).  Gradients and counts bit for bit
    against the plain entry points, counters against the restatement on the same rounded logits."""
    rng = np.random.RandomState(77)
    rnd = lambda a: (torch.from_numpy(a.astype(np.float32)).to(act_dtype()).float().numpy() if form == "16" else a.astype(np.float32))
    V, rows = 30522, 48
    x = rnd(rng.randn(rows, ld_of(form, V)) * 3.0)
    x[:, V:] = PAD
    labels = rng.randint(0, V, rows).astype(np.int64)
    labels[::5] = x[::5, :V].argmax(1)                         # some hits
    labels[3] = -1
    ref = MR.ce_eval_ref(x, V, labels)
    g0, _, l0, _ = run_ce(form, x, V, labels, copy=False)
    acc = counters(0, 0)
    g1, _, l1, _ = run_ce(form, x, V, labels, acc=acc, copy=False)
    assert same_bits(g1, g0) and acc.tolist() == [ref["hits"], ref["n"]] and ref["hits"] >= 9
    check_loss(form, l1, l0, "off-grid hard CE %s" % form)
    lc = np.concatenate((labels[labels >= 0], labels[labels < 0]))
    xc = np.concatenate((x[labels >= 0], x[labels < 0]))
    n0 = 20
    g0, l0 = run_compact(form, xc, V, lc, n0, ref["n"] - n0)
    a2 = torch.zeros((2, 2), dtype=torch.int64, device=dev())
    g1, l1 = run_compact(form, xc, V, lc, n0, ref["n"] - n0, acc=a2)
    r0, r1 = MR.ce_eval_ref(xc[:n0], V, lc[:n0]), MR.ce_eval_ref(xc[n0:], V, lc[n0:])
    assert same_bits(g1, g0) and a2.tolist() == [[r0["hits"], n0], [r1["hits"], ref["n"] - n0]]
    C, rows = 1601, 256
    xs = rnd(rng.randn(rows, ld_of(form, C)) * 3.0)
    xs[:, C:] = PAD
    t = np.zeros((rows, C), dtype=np.float32)
    for r in range(rows):                                      # 0.25 + 0.75: row sums of exactly 1; every fourth row agrees with the logits
        p, q = rng.choice(C, 2, replace=False)
        q = int(xs[r, :C].argmax()) if r % 4 == 0 else q
        p = p if p != q else (q + 1) % C
        t[r, p], t[r, q] = 0.25, 0.75
    t[5] = 0.0
    rs = MR.soft_ce_eval_ref(xs, C, t)
    g0, _, l0, _ = run_soft(form, xs, C, t)
    acc = counters(0, 0)
    g1, _, l1, _ = run_soft(form, xs, C, t, acc=acc)
    assert same_bits(g1, g0) and acc.tolist() == [rs["hits"], rs["n"]] and rs["n"] == rows - 1 and rs["hits"] >= 60
    check_loss(form, l1, l0, "off-grid soft CE %s" % form)


# ---- the device scale -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_kernel_dscale_form_is_the_host_product(form):
    """gscale * *dscale is rounded once to fp32 on the device: the bits of the call given that product from the host, the counters of
    the static call.  (0.37 x 1.3: the fp32 product is not exact, so a second rounding would show.)"""
    gs, dsv = 0.37, 1.3
    prod = float(np.float32(gs) * np.float32(dsv))
    assert prod != float(np.float32(gs)) * float(np.float32(dsv))
    ds = zf(1, dsv)
    rng = np.random.RandomState(12)
    V, rows = 37, 9
    x, labels = grid(rng, rows, V, ld_of(form, V)), mixed_labels(rng, rows, V)
    a_s, a_d = counters(), counters()
    gs_, _, ls_, _ = run_ce(form, x, V, labels, gscale=prod, acc=a_s)
    gd_, _, ld_, _ = run_ce(form, x, V, labels, gscale=gs, acc=a_d, dscale=ds)
    assert same_bits(gd_, gs_) and a_d.tolist() == a_s.tolist() and a_s.tolist() != [7, 11]
    check_loss(form, ld_, ls_, "dscale hard CE %s" % form)
    if form == "16":                                           # and the bits of the existing dynamic entry point
        assert same_bits(gd_, run_ce(form, x, V, labels, gscale=gs, dscale=ds)[0])
    lc = np.full(rows, -1, dtype=np.int64)
    lc[:5] = rng.randint(0, V, 5)
    a_s, a_d = torch.zeros((2, 2), dtype=torch.int64, device=dev()), torch.zeros((2, 2), dtype=torch.int64, device=dev())
    gs_, _ = run_compact(form, x, V, lc, 2, 3, gscale=prod, acc=a_s)
    gd_, _ = run_compact(form, x, V, lc, 2, 3, gscale=gs, acc=a_d, dscale=ds)
    assert same_bits(gd_, gs_) and a_d.tolist() == a_s.tolist() and a_s[:, 1].tolist() == [2, 3]
    C = 50
    xs, t = soft_case(rng, 7, C, ld_of(form, C))
    a_s, a_d = counters(), counters()
    gs_, _, _, _ = run_soft(form, xs, C, t, gscale=prod, acc=a_s)
    gd_, _, _, _ = run_soft(form, xs, C, t, gscale=gs, acc=a_d, dscale=ds)
    assert same_bits(gd_, gs_) and a_d.tolist() == a_s.tolist() and a_s.tolist() != [7, 11]


# ---- the reference's own numbers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", ["plain", "multi"])
def test_kernel_counters_reproduce_the_reference_metric_classes(case, form):
    """tests/golden/metrics/pretrain_metrics_small.npz: logits and labels fed to the reference's metric classes, and the hits and
    counts those classes recorded per batch."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "metrics", "pretrain_metrics_small.npz"), allow_pickle=False))
    V, C = int(g["V"]), int(g["C"])

    def padded(a, width):
        a = a.reshape(-1, a.shape[-1])
        out = np.full((a.shape[0], ld_of(form, width) + 8), PAD, dtype=np.float32)
        out[:, :width] = a
        return out

    for b in range(3):
        pre = "%s_b%d_" % (case, b)
        acc = torch.zeros((4, 2), dtype=torch.int64, device=dev())
        for row, sfx in (((0, "_wvc"), (1, "_aux")) if case == "multi" else ((0, ""),)):
            run_ce(form, padded(g[pre + "mlm_logits" + sfx], V), V, g[pre + "mlm_label" + sfx].reshape(-1), acc=acc[row], copy=False)
        run_soft(form, padded(g[pre + "mvrc_logits"], C), C, np.ascontiguousarray(g[pre + "mvrc_label"].reshape(-1, C)), acc=acc[2])
        if case == "plain":
            run_ce(form, padded(g[pre + "relationship_logits"], 2), 2, g[pre + "relationship_label"], acc=acc[3], copy=False)
        print("%s batch %d: device %s, reference %s" % (case, b, acc.tolist(), g[case + "_counts"][b].tolist()))
        assert acc.tolist() == g[case + "_counts"][b].tolist()


# ---- the fp16 build ---------------------------------------------------------------------------------------------------------------
KERNEL_TESTS = 52          # `pytest tests/test_train_metrics_gpu.py --collect-only -q -m gpu -k "kernel and not fp16_build"`


def test_fp16_build_runs_the_kernel_tests():
    """The kernel tests above once more in ONE child with VLB_PRECISION=f16 (one precision per process), with the rules of
    tests/test_f16_kernels_gpu.py: return code 0, the hard-coded number passed, nothing skipped; a signal, an abort or the time limit
    fails the test and nothing else is started; fails if the parent already runs the fp16 build."""
    if os.environ.get("VLB_PRECISION", "bf16").lower() in ("f16", "fp16"):
        pytest.fail("the parent process already runs with VLB_PRECISION=f16")
    env = dict(os.environ, VLB_PRECISION="f16", PYTHONUNBUFFERED="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_train_metrics_gpu.py"), "-m", "gpu", "-q", "-k",
           "kernel and not fp16_build"]
    t0 = time.time()
    with tempfile.TemporaryFile("w+") as outf, tempfile.TemporaryFile("w+") as errf:
        try:
            rc = subprocess.run(cmd, env=env, cwd=ROOT, stdout=outf, stderr=errf, timeout=180).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        outf.seek(0)
        errf.seek(0)
        out, err = outf.read(), errf.read()
    print(out[-4000:])
    print(err[-1500:])
    print("fp16 child: return code %d, %.1f s" % (rc, time.time() - t0))
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(os.path.join(os.path.dirname(REPORT), "f16_kernels_test_train_metrics_gpu.log"), "w") as f:
            f.write(out + "\n---- stderr ----\n" + err + "\n---- return code %d ----\n" % rc)
    except OSError:
        pass
    if rc < 0 or rc in (124, 134, 137, 139):
        pytest.fail("the fp16 child ended with return code %d (signal, abort or time limit)" % rc)
    assert rc == 0, out[-3000:]
    summary = out.strip().splitlines()[-1] if out.strip() else ""
    m = re.search(r"(\d+) passed", summary)
    assert m and int(m.group(1)) == KERNEL_TESTS, "expected %d passed: %s" % (KERNEL_TESTS, summary)
    assert "failed" not in summary and "skipped" not in summary and "error" not in summary, summary


# ---- the engine -------------------------------------------------------------------------------------------------------------------
# Model of the engine tests: 2 base-width layers, T = 32, R = 10, ragged synthetic batches, dropout on.  B = 3 (96 text positions) runs
# the MLM head on every row; labelled-row compaction needs more positions than its smallest capacity (256), so those cases use B = 9.
def make_engine(B=3, T=32, R=10, Ba=0, cfg_kw=None, batch_seed=9, **kw):
    E = pkg("engine")
    mc = E.ModelConfig(**dict(dict(num_hidden_layers=2), **(cfg_kw or {})))
    assert mc.hidden_dropout_prob > 0 and mc.attention_probs_dropout_prob > 0
    eng = E.PretrainEngine(mc, B, T, R, device="cuda:0", train=True, seed=5, B_aux=Ba, **kw)
    eng.init_random(seed=1, visual_ln_init=1.0)
    put_batch(eng, batch_seed)
    return eng


def put_batch(eng, seed):
    syn = pkg("synthetic")
    c = eng.cfg
    batch = list(syn.make_batch(eng.B, eng.T, eng.R, vocab_size=c.vocab_size, region_classes=c.visual_region_classes, seed=seed, ragged=True))
    if eng.Ba:
        batch += list(syn.make_aux_text(eng.Ba, eng.T, vocab_size=c.vocab_size, seed=seed + 1))
    eng.set_batch(*[t.to(dev()) for t in batch])


def forward_once(eng):
    """_forward_to_logits, clone the logits, _losses_fwd_bwd(keep=True) with forward()'s scale -> the restatement's counters."""
    eng._forward_to_logits(True)
    clones = (eng.mlm_logits.clone(), eng.mvrc_logits.clone(), eng.rel_logits.clone() if eng.cfg.with_rel_loss else None)
    eng._losses_fwd_bwd(1.0 if eng.scaler is not None else eng.loss_scale, True)
    torch.cuda.synchronize()
    eng.loss_values()                                          # (raises on an MLM compaction overflow)
    return TR.counts_ref(TR.engine_heads(eng, *clones), eng.cfg.vocab_size, eng.cfg.visual_region_classes)


def add_counts(a, b):
    return {k: (a[k][0] + b[k][0], a[k][1] + b[k][1]) for k in a}


@pytest.mark.parametrize("B", [9, 3], ids=["compact", "every_row"])
def test_engine_counters_equal_the_host_restatement_and_nothing_else_changes(B):
    on, off = make_engine(B=B, train_metrics=True), make_engine(B=B)
    assert (on.mlm_cap is not None) == (B == 9) and off.train_metric_acc is None
    want = forward_once(on)
    forward_once(off)
    got = on.train_metric_counts()
    print("B %d: device %s, restatement %s" % (B, got, want))
    assert got == want and want["mlm"][1] > 0 and want["mvrc"][1] > 0 and want["mlm_aux"] == (0, 0) == want["relationship"]
    # the same gradients and losses as an engine built without the option; the validation counters stay untouched
    assert same_bits(on.mlm_logits, off.mlm_logits) and same_bits(on.mvrc_logits, off.mvrc_logits)
    for a, b in zip(on.losses.tolist(), off.losses.tolist()):
        assert abs(a - b) <= 1e-6 * abs(b), (on.losses.tolist(), off.losses.tolist())
    assert int(on.metric_acc.abs().sum()) == 0
    with pytest.raises(ValueError, match="train_metrics=True"):
        off.train_metric_counts()
    on.reset_train_metrics()
    assert on.train_metric_counts() == {k: (0, 0) for k in on.METRIC_ROWS}


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "every_row"])
def test_engine_multitask_counts_caption_and_text_only_rows_apart(compact):
    """The configuration of tests/golden/multitask_small.npz (hidden 128, 2 layers, V = 512, C = 50, multitask).  every_row: its own
    batch (B = 3, B_aux = 2, 14 text positions).  compact: that batch has too few positions for the compaction, so a synthetic one
    of B = 6, B_aux = 4, T = 64 (640 positions, capacity 256) stands in."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "multitask_small.npz"), allow_pickle=False)
    kw = {str(k): (bool(v) if str(k) == "multitask" else int(v)) for k, v in zip(z["cfg_keys"], z["cfg_vals"])}
    if compact:
        kw["max_position_embeddings"] = 128
        eng = make_engine(B=6, T=64, R=12, Ba=4, cfg_kw=kw, batch_seed=54, train_metrics=True)
    else:
        Ba, Ta = [int(v) for v in z["aux_shape"]]
        E = pkg("engine")
        eng = E.PretrainEngine(E.ModelConfig(**kw), int(z["B"]), max(int(z["T"]), Ta), int(z["R"]), device="cuda:0", train=True, seed=5, B_aux=Ba,
                               train_metrics=True)
        eng.init_random(seed=1, visual_ln_init=1.0)
        eng.set_batch(*[torch.from_numpy(z["in_" + k]).to(dev()) for k in
                        ("boxes", "im_info", "text", "relationship_label", "mlm_labels", "mvrc_ops", "mvrc_labels", "aux_text", "aux_mlm_labels")])
    assert (eng.mlm_cap is not None) == compact
    want = forward_once(eng)
    got = eng.train_metric_counts()
    print("multitask %s: device %s, restatement %s" % ("compact" if compact else "every row", got, want))
    assert got == want and want["mlm"][1] > 0 and want["mlm_aux"][1] > 0 and want["relationship"] == (0, 0)


def test_engine_relationship_head_counts_into_row_3():
    z = np.load(os.path.join(ROOT, "tests", "golden", "full_rel.npz"), allow_pickle=False)
    kw = {str(k): (bool(v) if str(k) in ("with_pooler", "with_rel_loss") else int(v)) for k, v in zip(z["cfg_keys"], z["cfg_vals"])}
    assert kw["with_rel_loss"] and kw["with_pooler"]
    eng = make_engine(B=4, T=32, R=6, cfg_kw=kw, batch_seed=54, train_metrics=True)
    want = forward_once(eng)
    got = eng.train_metric_counts()
    print("full_rel: device %s, restatement %s" % (got, want))
    assert got == want and want["relationship"][1] > 0 and want["mlm"][1] > 0


def test_engine_dynamic_loss_scale_counts_like_the_static_engine():
    dyn, sta = make_engine(train_metrics=True, loss_scale="dynamic"), make_engine(train_metrics=True)
    assert dyn.scaler is not None and sta.scaler is None
    want = forward_once(dyn)
    forward_once(sta)
    assert dyn.train_metric_counts() == want == sta.train_metric_counts() and want["mlm"][1] > 0


@pytest.mark.parametrize("B", [9, 3], ids=["compact", "every_row"])
def test_engine_fp32_full_counts_from_its_fp32_logits(B):
    eng = make_engine(B=B, encoder_fp32=True, fp32_full=True, train_metrics=True)
    assert eng.mlm_logits.dtype == torch.float32 and (eng.mlm_cap is not None) == (B == 9)
    want = forward_once(eng)
    got = eng.train_metric_counts()
    print("fp32_full B %d: device %s, restatement %s" % (B, got, want))
    assert got == want and want["mlm"][1] > 0 and want["mvrc"][1] > 0


def test_engine_counters_accumulate_and_only_the_training_forward_moves_them():
    eng = make_engine(train_metrics=True, keep_logits=True)   # (kept copies: what the keep=False re-run restores the logits from)
    first = forward_once(eng)
    put_batch(eng, 10)
    both = add_counts(first, forward_once(eng))
    assert eng.train_metric_counts() == both and both != first
    eng._losses_fwd_bwd(eng.loss_scale, False)                 # the mirrors' re-run with another upstream scale: nothing counted twice
    torch.cuda.synchronize()
    assert eng.train_metric_counts() == both
    eng.eval_step()                                            # validation counts into its own table
    torch.cuda.synchronize()
    assert eng.train_metric_counts() == both and int(eng.metric_acc[:, 1].sum()) > 0
    eng.forward(True)                                          # and forward() is the path that counts
    torch.cuda.synchronize()
    assert eng.train_metric_counts()["mlm"][1] == both["mlm"][1] + (both["mlm"][1] - first["mlm"][1])


def test_engine_graph_replays_count_every_batch():
    """Exact form: the counters of three replays equal the sum, over the three batches, of the restatement on logits cloned in an
    eager twin stepped in lockstep.  Both engines run with lr = 0 (and the same weights, batches and dropout seed), so the optimizer
    leaves the weights as they are and every forward is a function of (weights, batch, seed) alone -- the twin's logits are the
    replayed step's logits although the gradients of a step are not reproducible bit for bit."""
    kw = dict(train_metrics=True, lr=0.0)
    eng, twin = make_engine(**kw), make_engine(**kw)
    eng.train_step()                                           # steady state before the capture
    twin.train_step()
    torch.cuda.synchronize()
    step = eng.make_step_graph()
    eng.reset_train_metrics()
    want = {k: (0, 0) for k in eng.METRIC_ROWS}
    for seed in (21, 22, 23):
        put_batch(eng, seed)
        step()
        put_batch(twin, seed)
        twin.zero_grad()
        want = add_counts(want, forward_once(twin))
        twin.backward(True)
        twin.optimizer_step()
    torch.cuda.synchronize()
    got = eng.train_metric_counts()
    print("three replays: device %s, eager twin's restatement %s" % (got, want))
    assert got == want and want["mlm"][1] > 0 and want["mvrc"][1] > 0


def test_engine_metric_classes_read_the_training_counters():
    met = pkg("common.metrics")
    eng = make_engine(train_metrics=True)
    metrics = met.pretrain_metrics()
    total, losses = {k: (0, 0) for k in eng.METRIC_ROWS}, []
    for seed in (9, 10):
        put_batch(eng, seed)
        total = add_counts(total, forward_once(eng))
        losses.append(eng.loss_values())
        metrics.update(eng.train_metrics_source)
        assert eng.train_metric_counts() == {k: (0, 0) for k in eng.METRIC_ROWS}      # moved into the metrics
    v = dict(zip(*metrics.get()))
    f32 = lambda a, b: (torch.tensor(a, dtype=torch.float32) / torch.tensor(b, dtype=torch.float32)).item()
    assert v["MLMAcc"] == f32(*total["mlm"]) and v["MVRCAccuracy"] == f32(*total["mvrc"])
    for name, key in (("MLMLoss", "mlm_loss"), ("MVRCLoss", "mvrc_loss")):
        mean = (losses[0][key] + losses[1][key]) / 2
        assert abs(v[name] - mean) <= 1e-6 * mean and mean > 0
    assert int(eng.metric_acc.abs().sum()) == 0


def test_train_end2end_prints_the_train_line(capsys):
    tr = pkg("pretrain.train_end2end")
    cfg = os.path.join(ROOT, "tests", "fixtures", "pretrain_small.yaml")
    eng = tr.main(["--cfg", cfg, "--steps", "4", "--train-metrics"])
    torch.cuda.synchronize()
    out = capsys.readouterr().out
    pat = re.compile(r"^Epoch\[0\] Batch \[\d+\]\tSpeed: [\d.]+ samples/s\tTrain-MLMAcc=[\d.]+,\tTrain-MVRCAccuracy=[\d.]+,"
                     r"\tTrain-MLMLoss=[\d.]+,\tTrain-MVRCLoss=[\d.]+,\t")
    lines = out.splitlines()
    train = [l for l in lines if pat.match(l)]
    steps = [l for l in lines if re.match(r"^step \d+  lr ", l)]
    assert len(train) == 2 and len(steps) == 2, out         # LOG_FREQUENT 2: after steps 2 and 4
    assert [lines.index(t) for t in train] == [lines.index(s) + 1 for s in steps]
    assert [int(re.search(r"Batch \[(\d+)\]", l).group(1)) for l in train] == [4, 8]      # two micro-batches per optimizer step
    assert eng.train_metrics and eng.train_metrics_monitor is not None
