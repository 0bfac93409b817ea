"""Fine-tuning evaluation on the device (-m gpu): the kernels of vl-bert_amd/csrc/finetune_metrics.hip against their numpy
restatement (tests/finetune_metrics_ref.py, itself pinned to the reference's metric classes by tests/test_finetune_metrics_cpu.py),
exactly; the metric classes of common/{vqa,vcr,refcoco}_metrics.py on the fixture's `outputs` dicts without a host synchronisation
in update(); do_validation / predict / the writers through the three module mirrors at the small fixture configurations; the entry
point's --val-steps lines and checkpoints; and the whole file once more on the fp16 build."""
import importlib
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import finetune_metrics_ref as FR
from tests.gpu_util import dev, pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "metrics")
U = 2.0 ** -24

# Largest |probs - float64 numpy softmax| of vlb_argmax_eval over every case of test_argmax_eval_*: fp32 accumulation in another order
# and __expf against exp.  Measured on MI355X: 4.641e-08 (at C = 4; the same in the bf16 and the fp16 build, the kernel reads fp32 only;
# 6.2e-10 at C = 3129); asserted with the 4x margin
# tests/test_metrics_gpu.py uses for __expf and reduction-order differences.
PROBS_ABS_MEASURED = 4.641e-8
PROBS_ABS_TOL = 4 * PROBS_ABS_MEASURED
_probs_seen = [0.0]

WAVE_MAX_C = 256                    # C <= 256: one wave per row; above: one 256-thread block per row (csrc/finetune_metrics.hip)
SHAPES = [(3, 1, 1), (7, 4, 4), (5, 20, 24), (4, 64, 64), (4, 65, 72), (3, 256, 256), (3, 257, 264), (5, 3129, 3136)]
TIE, TOP, PAD = 7.75, 7.5, 8.0      # planted row maximum | ceiling of every other real column | columns C..ld-1: would win if read


def g(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(dev())


def tie_pairs(C):
    """(a, b), a < b: both hold the row maximum, a must win.  Adjacent columns = two neighbouring threads (lanes); 63 | 64 = the last
    thread of wave 0 and the first of wave 1 in the block-per-row layout (two chunks of lane 63 / lane 0 in the wave layout);
    c | c + stride = one thread's first and second chunk (stride 64 in the wave-per-row layout, 256 in the block-per-row layout)."""
    pairs = []
    if C >= 2:
        pairs.append((C // 2 - 1, C // 2) if C < 9 else (7, 8))
    if C > 64:
        pairs.append((63, 64))
    stride = 64 if C <= WAVE_MAX_C else 256
    if C > stride:
        pairs.append((0, stride) if C < stride + 4 else (3, stride + 3))
    return pairs


def make_logits(rows, C, ld, variant, seed):
    """fp32 [rows, ld]: real columns <= TOP, padding PAD.  variant "ties": row k holds pair k of tie_pairs (cycled).  "special": row 0
    two NaNs (the first wins), row 1 all -inf (column 0), the other rows a tie pair."""
    rng = np.random.RandomState(seed)
    x = (rng.randint(-64, int(TOP * 8) + 1, size=(rows, ld)) / 8.0).astype(np.float32)
    x[:, C:] = PAD
    pairs = tie_pairs(C)
    want = {}
    for r in range(rows):
        if variant == "special" and r == 0:
            cols = sorted({C // 3, C - 1})
            x[r, cols] = np.nan
            want[r] = cols[0]
        elif variant == "special" and r == 1:
            x[r, :C] = -np.inf
            want[r] = 0
        elif pairs:
            a, b = pairs[r % len(pairs)]
            x[r, [a, b]] = TIE
            want[r] = a
    return x, want


def check_probs(probs, x, C, ldp):
    got = probs.cpu().numpy()
    ref = FR.softmax_ref(x, C)
    assert (got[:, C:] == -3.0).all()                                     # columns >= C of probs are not written
    nan_rows = np.isnan(ref).any(axis=1)
    assert np.isnan(got[nan_rows][:, :C]).all() and not np.isnan(got[~nan_rows][:, :C]).any()
    if (~nan_rows).any():
        d = float(np.abs(got[~nan_rows][:, :C].astype(np.float64) - ref[~nan_rows]).max())
        _probs_seen[0] = max(_probs_seen[0], d)
        print("probs C=%d: max |kernel - float64 softmax| %.3e (largest so far %.3e, bar %.1e)" % (C, d, _probs_seen[0], PROBS_ABS_TOL))
        assert d <= PROBS_ABS_TOL, (C, d)


@pytest.mark.parametrize("variant", ["ties", "special"])
@pytest.mark.parametrize("rows,C,ld", SHAPES)
def test_argmax_eval_matches_the_restatement_in_every_mode(rows, C, ld, variant):
    ops = pkg("ops")
    x, want = make_logits(rows, C, ld, variant, seed=rows * 1000 + C)
    pred_ref = FR.argmax_ref(x, C)
    for r, col in want.items():
        assert pred_ref[r] == col, (r, col, pred_ref[r])                  # the plants are what the restatement sees
    logits = g(x)
    before = logits.clone()
    rng = np.random.RandomState(C)
    # ---- mode 0: predictions and the softmax ----
    pred = torch.full((rows,), -7, dtype=torch.int32, device=dev())
    ldp = C + 1
    probs = torch.full((rows, ldp), -3.0, dtype=torch.float32, device=dev())
    ops.argmax_eval(logits[:, :C], ops.ARGMAX_PREDICT, pred=pred, probs=probs[:, :C])
    torch.cuda.synchronize()
    assert np.array_equal(pred.cpu().numpy(), pred_ref)
    check_probs(probs, x, C, ldp)
    # ---- mode 1: hard labels, -1 interleaved, one label >= C, hits on the even rows ----
    lab = rng.randint(0, C, rows).astype(np.int64)
    lab[0::2] = pred_ref[0::2]
    lab[1::2] = -1
    lab[rows - 1] = C + 1
    ref = FR.argmax_eval_ref(x, C, FR.HARD, lab, 10, 20)
    assert ref["count"] == 20 + rows - len(lab[1::2]) + (1 if (rows - 1) % 2 else 0)
    pred.fill_(-7)
    score = torch.full((rows,), -7.0, dtype=torch.float32, device=dev())
    acc = torch.tensor([10, 20], dtype=torch.int64, device=dev())
    ops.argmax_eval(logits[:, :C], ops.ARGMAX_HARD, label=g(lab), pred=pred, score=score, sum=acc[0], count=acc[1])
    torch.cuda.synchronize()
    assert np.array_equal(pred.cpu().numpy(), pred_ref) and np.array_equal(score.cpu().numpy(), ref["score"])
    assert acc.tolist() == [ref["sum"], ref["count"]]
    ops.argmax_eval(logits[:, :C], ops.ARGMAX_HARD, label=g(lab), sum=acc[0], count=acc[1])         # no optional output; accumulated
    torch.cuda.synchronize()
    assert acc.tolist() == [2 * ref["sum"] - 10, 2 * ref["count"] - 20]
    # ---- mode 2: soft scores from {0, 0.3, 0.6, 0.9, 1}, label stride > C; the double is bit-equal to the sequential loop ----
    ldl = ld + 3
    soft = rng.choice(np.array([0.0, 0.3, 0.6, 0.9, 1.0], np.float32), size=(rows, ldl)).astype(np.float32)
    soft[np.arange(rows), pred_ref] = np.array([0.3, 0.6, 0.9, 1.0, 0.3, 0.9, 0.6], np.float32)[:rows]      # nonzero scores in every row
    soft[:, C:] = 55.0
    ref = FR.argmax_eval_ref(x, C, FR.GATHER, soft[:, :C], 0.25, 3)
    dsum = torch.tensor(0.25, dtype=torch.float64, device=dev())
    cnt = torch.tensor(3, dtype=torch.int64, device=dev())
    label = g(soft)
    score.fill_(-7.0)
    ops.argmax_eval(logits[:, :C], ops.ARGMAX_GATHER, label=label[:, :C], score=score, sum=dsum, count=cnt)
    torch.cuda.synchronize()
    assert np.array_equal(score.cpu().numpy(), ref["score"]) and int(cnt) == ref["count"]
    assert dsum.item() == ref["sum"], (dsum.item(), ref["sum"])
    ref2 = FR.argmax_eval_ref(x, C, FR.GATHER, soft[:, :C], ref["sum"], ref["count"])
    ops.argmax_eval(logits[:, :C], ops.ARGMAX_GATHER, label=label[:, :C], score=score, sum=dsum, count=cnt)
    torch.cuda.synchronize()
    assert dsum.item() == ref2["sum"] and int(cnt) == ref2["count"]
    # ---- mode 3: a gathered 0.5 is a miss (strict); a -1 padding column that wins the argmax is a miss ----
    hard = (rng.rand(rows, ldl) < 0.5).astype(np.float32)
    hard[:, C:] = 1.0
    hard[0, pred_ref[0]] = 0.5
    x3 = x.copy()
    if C > 1 and rows > 2 and variant == "ties":
        x3[2, C - 1] = PAD - 0.125                                        # above TIE: the last column wins row 2 ...
        hard[2, C - 1] = -1.0                                             # ... and it is padding of the label
    pred3 = FR.argmax_ref(x3, C)
    ref = FR.argmax_eval_ref(x3, C, FR.GATHER_GT, hard[:, :C], 10, 20)
    assert ref["score"][0] == 0.0 and (not (C > 1 and rows > 2 and variant == "ties") or (pred3[2] == C - 1 and ref["score"][2] == 0.0))
    acc = torch.tensor([10, 20], dtype=torch.int64, device=dev())
    pred.fill_(-7)
    score.fill_(-7.0)
    ops.argmax_eval(g(x3)[:, :C], ops.ARGMAX_GATHER_GT, label=g(hard)[:, :C], pred=pred, score=score, sum=acc[0], count=acc[1])
    torch.cuda.synchronize()
    assert np.array_equal(pred.cpu().numpy(), pred3) and np.array_equal(score.cpu().numpy(), ref["score"])
    assert acc.tolist() == [ref["sum"], ref["count"]] and ref["count"] == 20 + rows
    assert torch.equal(logits.view(torch.int32), before.view(torch.int32))                            # the logits are only read


def test_argmax_eval_rejects_what_it_cannot_run():
    ops = pkg("ops")
    x = torch.zeros((2, 4), dtype=torch.float32, device=dev())
    acc = torch.zeros(2, dtype=torch.int64, device=dev())
    with pytest.raises(RuntimeError, match="needs score"):
        ops.argmax_eval(x, ops.ARGMAX_GATHER, label=x, sum=torch.zeros((), dtype=torch.float64, device=dev()), count=acc[1])
    with pytest.raises(RuntimeError, match="ldl"):
        ops.argmax_eval(x, ops.ARGMAX_GATHER_GT, label=x[:, :3].contiguous(), sum=acc[0], count=acc[1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.argmax_eval(x.cpu(), ops.ARGMAX_PREDICT, pred=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="expected dtype"):
        ops.argmax_eval(x.half(), ops.ARGMAX_PREDICT)


@pytest.mark.parametrize("rows,N", [(1, 1), (3, 20), (5, 77)])
def test_binary_cls_eval_matches_the_restatement(rows, N):
    ops = pkg("ops")
    rng = np.random.RandomState(N)
    ld, ldl = N + 3, N + 5
    x = rng.choice(np.array([0.0, 1e-30, -1e-30, np.nan, 2.5, -2.5], np.float32), size=(rows, ld)).astype(np.float32)
    lab = rng.choice(np.array([-1.0, -0.5, 0.0, 0.7, 1.0, 1.0], np.float32), size=(rows, ldl)).astype(np.float32)
    x[:, N:], lab[:, N:] = PAD, 1.0                                       # would be counted as correct positives if read
    if N == 1:
        x[0, 0], lab[0, 0] = 1e-30, 1.0
    ref = FR.binary_cls_ref(x, lab, N)
    assert N == 1 or (ref[1] < rows * N and ref[3] > 0 and ref[0] < ref[1])
    acc = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device=dev())
    ops.binary_cls_eval(g(x)[:, :N], g(lab)[:, :N], acc)
    torch.cuda.synchronize()
    assert acc.tolist() == [1 + ref[0], 2 + ref[1], 3 + ref[2], 4 + ref[3]]


@pytest.mark.parametrize("rows", [1, 5, 130])
def test_joint_hits_matches_the_restatement(rows):
    ops = pkg("ops")
    rng = np.random.RandomState(rows)
    pa, pr = rng.randint(0, 4, rows).astype(np.int32), rng.randint(0, 4, rows).astype(np.int32)
    la, lr = pa.astype(np.int64), pr.astype(np.int64)
    la[1::3] = (la[1::3] + 1) % 4                                         # answer wrong
    lr[2::3] = -1                                                         # rationale label -1: not filtered, simply wrong
    ref = FR.joint_hits_ref(pa, la, pr, lr)
    assert ref == [len(range(0, rows, 3)), rows]
    acc = torch.tensor([7, 9], dtype=torch.int64, device=dev())
    ops.joint_hits(g(pa), g(la), g(pr), g(lr), acc)
    torch.cuda.synchronize()
    assert acc.tolist() == [7 + ref[0], 9 + ref[1]]


# ---- the metric classes on the reference's fixture ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "finetune_metrics_small.npz"), allow_pickle=False))


def fixture_metrics(case):
    if case == "vqa":
        m = pkg("common.vqa_metrics")
        return [m.SoftAccuracy(), m.LossLogger("ans_loss", display_name="AnsLoss")]
    if case == "vcr":
        m = pkg("common.vcr_metrics")
        return [m.Accuracy(), m.AnsLoss(), m.CNNRegLoss(), m.PositiveFraction(), m.LossLogger("ans_loss", display_name="AnsLossLog"),
                m.LossLogger("no_such_loss"), m.JointAccuracy()]
    m = pkg("common.refcoco_metrics")
    return [m.RefAccuracy(), m.ClsAccuracy(), m.ClsPosAccuracy(), m.ClsPosFraction(), m.LossLogger("cls_loss", display_name="ClsLoss")]


def no_sync(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("host synchronisation inside update()")
    for name in ("item", "cpu", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, boom)


@pytest.mark.parametrize("case", ["vqa", "vcr", "refcoco"])
def test_metric_classes_reproduce_the_reference_fixture_without_synchronising(case, gold, monkeypatch):
    M = pkg("common.metrics")
    metrics = fixture_metrics(case)
    comp = M.CompositeEvalMetric()
    for m in metrics:
        assert isinstance(m, M.EvalMetric)
        comp.add(m)
    names, values = comp.get()
    assert names == [str(n) for n in gold[case + "_names"]] and all(math.isnan(v) for v in values)      # nan before any update
    batches, soft_bound = [], 0.0
    for b in range(3):
        pre = "%s_b%d_" % (case, b)
        out = {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}
        if case == "vqa":
            sc = FR.argmax_eval_ref(out["label_logits"], out["label_logits"].shape[1], FR.GATHER, out["label"])["score"]
            soft_bound += len(sc) * U * float(sc.astype(np.float64).sum())
        batches.append({k: g(v) for k, v in out.items()})
    with monkeypatch.context() as mp:
        no_sync(mp)
        for out in batches:
            comp.update(out)
    torch.cuda.synchronize()
    ref_sum, ref_n = gold[case + "_sum_metric"][-1], gold[case + "_num_inst"][-1]
    names, values = comp.get()
    for k, m in enumerate(metrics):
        s, n = float(m.sum_metric), int(m.num_inst)
        assert n == ref_n[k], (m.name, n, ref_n[k])
        if m.sum_metric.dtype == torch.int64:
            assert s == ref_sum[k], (m.name, s, ref_sum[k])
            tol = 0.0
        elif m.name == "SoftAcc":
            assert m.sum_metric.dtype == torch.float64 and m.sum_metric.is_cuda
            tol = soft_bound                                              # n * 2^-24 * sum(score) per batch: the reference's fp32 sums
            print("SoftAcc: device %.17g reference %.17g bound %.3e" % (s, ref_sum[k], tol))
        else:
            tol = 3 * (3 + 1) * U * abs(ref_sum[k])                       # three batches: a mean of <= 3 fp32 values + one fp32 add each
        assert abs(s - ref_sum[k]) <= tol, (m.name, s, ref_sum[k], tol)
        ref_v = float(gold[case + "_values"][k])
        assert abs(values[k] - ref_v) <= 2.0 ** -23 * abs(ref_v) + tol / max(n, 1), (m.name, values[k], ref_v)
    comp.reset()
    assert all(math.isnan(v) for v in comp.get()[1])


def test_metric_classes_refuse_cpu_tensors_and_one_dimensional_vcr_logits(gold):
    for case in ("vqa", "vcr", "refcoco"):
        pre = case + "_b0_"
        out = {k[len(pre):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(pre)}
        for m in fixture_metrics(case):
            if m.name == "no_such_loss":
                m.update(out)                                             # nothing to read: the batch is counted
                assert int(m.num_inst) == 1
                continue
            with pytest.raises(RuntimeError, match="no CPU path"):
                m.update(out)
    acc = pkg("common.vcr_metrics").Accuracy()
    with pytest.raises(NotImplementedError):
        acc.update({"label_logits": torch.zeros(8, device=dev()), "label": torch.zeros(8, dtype=torch.int64, device=dev())})


# ---- through the module mirrors at the small fixture configurations -------------------------------------------------------------
TASKS = ["vqa", "vcr", "refcoco"]
_nets = {}


def small_net(task):
    """(net, config, two validation batches in the entry point's layout, label index) -- built once per task"""
    if task not in _nets:
        F = pkg("common.finetune_entry")
        syn = pkg("synthetic")
        config = F.load_config(task, os.path.join(ROOT, "tests", "fixtures", task + "_small.yaml"))
        torch.manual_seed(5)
        net = getattr(pkg("%s.modules.resnet_vlbert_for_%s" % (task, task)), config.MODULE)(config, device=dev())
        Hi, Wi = int(config.SCALES[0]), int(config.SCALES[1])

        def make(seed):
            if task == "vqa":
                return syn.make_vqa_batch(3, 10, 12, seed, dev(), answers=int(config.DATASET.ANSWER_VOCAB_SIZE))
            if task == "refcoco":
                return syn.make_refcoco_batch(3, 6, 8, Hi, Wi, seed, dev(), precomputed=bool(config.NETWORK.IMAGE_FEAT_PRECOMPUTED))
            return syn.make_vcr_batch(3, 4, 5, 8, 9, Hi, Wi, seed, dev())
        _nets[task] = (net, config, list(F._ValBatches(task, make, 2)), F.VAL_LABEL_INDEX[task])
    return _nets[task]


class Recorder:
    """the net as do_validation sees it, keeping a copy of every label_logits it returns"""

    def __init__(self, net):
        self.net, self.logits = net, []

    def eval(self):
        self.net.eval()
        return self

    def __call__(self, *datas):
        out = self.net(*datas)
        self.logits.append(out["label_logits"].detach().clone())
        return out


@pytest.mark.parametrize("task", TASKS)
def test_do_validation_through_the_mirror_counts_what_the_restatement_counts(task):
    net, config, batches, index = small_net(task)
    M, fe = pkg("common.metrics"), pkg("common.finetune_eval")
    TM = pkg("common.%s_metrics" % task)
    net.train()
    net.zero_grad()
    _, loss = net(*batches[0])                                            # (the validation layout IS train_forward's argument list)
    loss.backward()
    torch.cuda.synchronize()
    params = [(n, p.detach().clone(), None if p.grad is None else p.grad.detach().clone()) for n, p in net.named_parameters()]
    assert any(gr is not None and float(gr.abs().sum()) > 0 for _, _, gr in params)
    seed = net._seed.clone()
    metrics = M.CompositeEvalMetric()
    for m in ([TM.SoftAccuracy()] if task == "vqa" else [TM.Accuracy()] if task == "vcr" else
              [TM.RefAccuracy(), TM.ClsAccuracy(), TM.ClsPosAccuracy(), TM.ClsPosFraction()]):
        metrics.add(m)
    rec = Recorder(net)
    fe.do_validation(rec, batches, metrics, index)
    torch.cuda.synchronize()
    assert not net.training and len(rec.logits) == 2
    s, n, cls = 0, 0, [0, 0, 0, 0]
    for lg, b in zip(rec.logits, batches):
        x, lab = lg.cpu().numpy(), b[index].cpu().numpy()
        assert x.dtype == np.float32 and x.ndim == 2 and x.shape[0] == 3
        mode = {"vqa": FR.GATHER, "vcr": FR.HARD, "refcoco": FR.GATHER_GT}[task]
        r = FR.argmax_eval_ref(x, x.shape[1], mode, lab, s, n)
        s, n = r["sum"], r["count"]
        if task == "refcoco":
            cls = [a + c for a, c in zip(cls, FR.binary_cls_ref(x, lab, x.shape[1]))]
    host = metrics.get_metric(0)
    print("%s: device sum %r count %d, restatement %r %d" % (task, host.sum_metric.item(), int(host.num_inst), s, n))
    assert host.sum_metric.item() == s and int(host.num_inst) == n == 6
    if task == "refcoco":
        got = [(float(m.sum_metric), float(m.num_inst)) for m in metrics.metrics[1:]]
        assert got == [(cls[0], cls[1]), (cls[2], cls[3]), (cls[3], cls[1])] and cls[1] > 0
    # validation changed nothing the training step owns
    for (name, p0, g0), (_, p) in zip(params, net.named_parameters()):
        assert torch.equal(p0, p.detach()), name
        assert (g0 is None and p.grad is None) or torch.equal(g0, p.grad), name
    assert torch.equal(seed, net._seed)
    net.train()


@pytest.mark.parametrize("task", TASKS)
def test_predict_and_the_writers_round_trip(task, tmp_path):
    net, config, batches, index = small_net(task)
    fe = pkg("common.finetune_eval")
    loader = [[x for i, x in enumerate(b) if i != index] for b in batches]
    rec = Recorder(net)
    got = fe.predict(rec, loader, task)
    torch.cuda.synchronize()
    logits = torch.cat(rec.logits, 0).cpu().numpy()
    n = logits.shape[0]
    assert n == 6
    if task == "vqa":
        assert got.dtype == np.int64 and np.array_equal(got, FR.argmax_ref(logits, logits.shape[1]))
        vocab = ["answer %d" % i for i in range(logits.shape[1])]
        qids = list(range(100, 100 + n))
        with open(fe.write_vqa_result(str(tmp_path / "vqa.json"), qids, got, vocab)) as f:
            back = json.load(f)
        assert [r["question_id"] for r in back] == qids and [vocab.index(r["answer"]) for r in back] == got.tolist()
    elif task == "vcr":
        ref = FR.softmax_ref(logits, 4)
        # (other logits than the measured kernel cases: <= 8 fp32 roundoffs of a value <= 1 -- two __expf, a 4-term sum, a reciprocal, a product)
        assert got.dtype == np.float32 and got.shape == (n, 4) and float(np.abs(got - ref).max()) <= 8 * U
        ids = ["val-%d" % i for i in range(n)]
        c, p = str(tmp_path / "q2a.csv"), str(tmp_path / "q2a.npy")
        fe.write_vcr_result(c, p, ids, got, "Q2A")
        assert np.array_equal(np.load(p), got)
        with open(c) as f:
            lines = f.read().splitlines()
        assert lines[0] == "annot_id,answer_0,answer_1,answer_2,answer_3" and [l.split(",")[0] for l in lines[1:]] == ids
        back = np.array([[np.float32(v) for v in l.split(",")[1:]] for l in lines[1:]], dtype=np.float32)
        assert np.array_equal(back, got)                                  # the shortest text reads back to the same fp32
        c2 = str(tmp_path / "qa2r.csv")
        fe.write_vcr_result(c2, str(tmp_path / "qa2r.npy"), ids[::-1], np.tile(got[::-1], (1, 4)), "QA2R")
        with open(fe.merge_vcr_results(c, c2, str(tmp_path / "merged.csv"))) as f:
            merged = f.read().splitlines()
        assert len(merged) == n + 1 and len(merged[0].split(",")) == 21 and [l.split(",")[0] for l in merged[1:]] == ids
        assert all(l.split(",")[1:5] == l.split(",")[5:9] for l in merged[1:])
    else:
        assert got.dtype == np.float32 and got.shape == (n, 4) and np.isfinite(got).all()
        rids = list(range(7, 7 + n))
        with open(fe.write_refcoco_result(str(tmp_path / "ref.json"), rids, got)) as f:
            back = json.load(f)
        assert [r["ref_id"] for r in back] == rids and np.array_equal(np.array([r["box"] for r in back], dtype=np.float32), got)
        # every predicted box is one of the sample's own boxes scaled back by im_info's ratios: the accuracy against themselves is 1
        xywh = got.astype(np.float64).copy()
        xywh[:, 2:] -= xywh[:, :2]
        assert fe.refcoco_accuracy(got, xywh) == 1.0
    net.train()


@pytest.mark.parametrize("task", TASKS)
def test_entry_point_validates_and_checkpoints_at_every_epoch_end(task, tmp_path, capsys, monkeypatch):
    for k in ("VLB_ENCODER_FP32", "HSA_ENABLE_IPC_MODE_LEGACY"):          # main() sets them: put them back afterwards
        monkeypatch.setenv(k, os.environ.get(k, "0"))
    F = pkg("common.finetune_entry")
    mdir = str(tmp_path / "model")
    cfg = os.path.join(ROOT, "tests", "fixtures", task + "_small.yaml")
    net, opt, loss = F.main(task, ["--cfg", cfg, "--steps", "4", "--steps-per-epoch", "2", "--val-steps", "2", "--model-dir", mdir])
    torch.cuda.synchronize()
    out = capsys.readouterr().out
    name = {"vqa": "SoftAcc", "vcr": "Acc", "refcoco": "RefAcc"}[task]
    lines = [l for l in out.splitlines() if l.startswith("Epoch[")]
    assert len(lines) == 2, out
    vals = []
    for k, l in enumerate(lines):
        m = re.fullmatch(r"Epoch\[%d\] \tVal-%s=([-\w.]+),\t" % (k, name), l)
        assert m, l
        vals.append(float(m.group(1)))
        assert 0.0 <= vals[-1] <= 1.0
    assert net.training and math.isfinite(loss)
    prefix = "vl-bert_small_" + task
    files = sorted(os.listdir(mdir))
    assert files == [prefix + "-0000.model", prefix + "-0001.model", prefix + "-best.model"], files
    cks = [torch.load(os.path.join(mdir, f), map_location="cpu", weights_only=False) for f in files]
    M = pkg("common.metrics")
    for e, ck in enumerate(cks[:2]):
        mon = M.ValidationMonitor(None, None, None)
        mon.load_state_dict(ck["validation_monitor"])
        assert 0 <= mon.best_epoch <= e and abs(mon.best_val - max(vals[:e + 1])) <= 5e-7 and "optimizer" in ck      # (the lines print %f)
    best_epoch = cks[1]["validation_monitor"]["best_epoch"]
    assert cks[0]["validation_monitor"]["best_epoch"] == 0 and vals[best_epoch] >= vals[1 - best_epoch] - 1e-6
    best, same = cks[2], cks[best_epoch]
    assert best["validation_monitor"] == same["validation_monitor"] and list(best["state_dict"]) == list(same["state_dict"])
    assert all(torch.equal(best["state_dict"][k], same["state_dict"][k]) for k in same["state_dict"])
    assert out.count("Save new best model to %s." % os.path.join(mdir, prefix + "-best.model")) == 1 + best_epoch
    assert any(not torch.equal(cks[0]["state_dict"][k], cks[1]["state_dict"][k]) for k in cks[0]["state_dict"])      # two different epochs


def test_this_file_on_the_fp16_build():
    """One precision per process (vl-bert_amd/_lib.py): the file once more in a child with VLB_PRECISION=f16, as
    tests/test_f16_build_gpu.py runs the engine suite."""
    if os.environ.get("VLB_PRECISION", "bf16").lower() in ("f16", "fp16", "half", "float16"):
        return                                                            # (already the fp16 build: nothing to add)
    env = dict(os.environ, VLB_PRECISION="f16")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-k", "not fp16_build"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    print(r.stderr[-1500:])
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 35, r.stdout[-500:]
