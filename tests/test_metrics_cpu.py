"""CPU checks of the validation layer: vl-bert_amd/common/metrics.py fed device-counter-shaped CPU tensors reproduces what the
REFERENCE's metric classes produced (tests/golden/metrics/pretrain_metrics_small.npz, tools/make_pretrain_metrics_golden.py), the
validation monitor follows the reference's best-epoch rule, the all-reduce sums before it divides, and the numpy restatement of the
kernels (tests/metrics_ref.py) agrees with the reference's counts and losses on the fixture's logits."""
import importlib
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import metrics_ref as MR

HERE = os.path.dirname(os.path.abspath(__file__))
N_BATCH = 3


def M():
    return importlib.import_module("vl-bert_amd.common.metrics")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "metrics", "pretrain_metrics_small.npz"), allow_pickle=False))


class FakeEngine:
    """What metrics.update() reads of a PretrainEngine: metric_acc, losses, reset_metrics()."""

    def __init__(self):
        self.metric_acc = torch.zeros((4, 2), dtype=torch.int64)
        self.losses = torch.zeros(4, dtype=torch.float32)
        self.resets = 0

    def reset_metrics(self):
        self.metric_acc.zero_()
        self.resets += 1


def build(case, gold, **kw):
    m = M()
    multi = case == "multi"
    return m.pretrain_metrics(with_rel_loss=not multi, multitask=multi, loss_loggers=m.parse_loss_loggers([str(s) for s in gold[case + "_loggers"]]), **kw)


@pytest.mark.parametrize("case", ["plain", "multi"])
def test_host_metrics_reproduce_the_reference_values(case, gold):
    metrics = build(case, gold)
    eng = FakeEngine()
    for b in range(N_BATCH):
        eng.metric_acc += torch.from_numpy(gold[case + "_counts"][b])      # what eval_step() adds
        eng.losses.copy_(torch.from_numpy(gold[case + "_losses"][b]))
        metrics.update(eng)
        assert int(eng.metric_acc.abs().sum()) == 0                          # moved, not copied
    names, values = metrics.get()
    assert names == [str(n) for n in gold[case + "_names"]]
    for n, v, ref in zip(names, values, gold[case + "_values"]):
        assert (math.isnan(v) and math.isnan(ref)) or v == ref, (n, v, ref)
    if case == "multi":
        assert math.isnan(dict(zip(names, values))["MLMAccAUX"])             # no aux label in any batch: the empty metric
    metrics.reset()
    assert all(math.isnan(v) for v in metrics.get()[1])
    assert [n for n, _ in metrics.get_metric(0).get_name_value()] == names[:1]


def test_counters_accumulated_over_batches_on_the_source_give_the_same_accuracies(gold):
    """The accuracies do not depend on how often the counters are moved: one update after three eval steps == three updates."""
    a, b = build("plain", gold), build("plain", gold)
    eng = FakeEngine()
    for i in range(N_BATCH):
        eng.metric_acc += torch.from_numpy(gold["plain_counts"][i])
    a.update(eng)
    eng2 = FakeEngine()
    for i in range(N_BATCH):
        eng2.metric_acc += torch.from_numpy(gold["plain_counts"][i])
        b.update(eng2)
    assert a.get()[1][:3] == b.get()[1][:3] == list(gold["plain_values"][:3])


def test_metric_order_and_names_follow_the_configuration():
    m = M()
    assert m.pretrain_metrics().get()[0] == ["MLMAcc", "MVRCAccuracy", "RelLoss", "MLMLoss", "MVRCLoss"]
    assert m.pretrain_metrics(with_rel_loss=True).get()[0][:2] == ["RelAcc", "MLMAcc"]
    multi = m.pretrain_metrics(multitask=True, loss_loggers=m.parse_loss_loggers(["mlm_loss_wvc,MLMLossWVC", "mlm_loss_aux,MLMLossAUX", "mvrc_loss,MVRCLoss"]))
    assert multi.get()[0] == ["MLMAccWVC", "MLMAccAUX", "MVRCAccuracy", "MLMLossWVC", "MLMLossAUX", "MVRCLoss"]
    assert m.host_metric_name(False) == "MLMAcc" and m.host_metric_name(True) == "MLMAccWVC"
    # a logger of an output the module does not produce counts the batch and adds nothing (pretrain_metrics.py:13-17)
    lost = m.pretrain_metrics(multitask=True)              # default loggers name mlm_loss, which the multitask module does not output
    eng = FakeEngine()
    eng.losses.fill_(3.0)
    lost.update(eng)
    assert dict(zip(*lost.get()))["MLMLoss"] == 0.0 and dict(zip(*lost.get()))["MVRCLoss"] == 3.0


def test_validation_monitor_keeps_the_best_epoch_by_the_reference_rule(capsys):
    m = M()
    seq = [(1, 4), (3, 4), (3, 4), (2, 4)]                 # MLMAcc per epoch: 0.25, 0.75, 0.75 (not strictly greater), 0.5
    calls = []

    def val_func(net, loader, metrics, load_batch):
        metrics.reset()
        hits, n = seq[len(calls)]
        net.metric_acc[0] = torch.tensor([hits, n])
        net.losses.fill_(0.5)
        metrics.update(net)
        calls.append(loader)

    metrics = m.pretrain_metrics()
    mon = m.ValidationMonitor(val_func, "loader", metrics, host_metric_name="MLMAcc")
    assert (mon.best_epoch, mon.best_val) == (-1, -1.0)
    eng = FakeEngine()
    for epoch in range(4):
        mon(epoch, eng, None, None)
    assert (mon.best_epoch, mon.best_val) == (1, 0.75) and calls == ["loader"] * 4
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "New Best Val MLMAcc: 0.25, Epoch: 0"
    assert out[1] == "Epoch[0] \tVal-MLMAcc=0.250000,\tMVRCAccuracy=nan,\tRelLoss=0.500000,\tMLMLoss=0.500000,\tMVRCLoss=0.500000,\t"
    assert out[2] == "Best Val MLMAcc: 0.25, Epoch: 0"
    assert out[-1] == "Best Val MLMAcc: 0.75, Epoch: 1" and sum(l.startswith("New Best Val") for l in out) == 2
    sd = mon.state_dict()
    assert sd == {"best_epoch": 1, "best_val": 0.75}
    mon2 = m.ValidationMonitor(val_func, "loader", metrics, host_metric_name="MLMAcc")
    mon2.load_state_dict(sd)
    assert mon2.state_dict() == sd
    with pytest.raises(AssertionError):
        mon2.load_state_dict({"best_epoch": 0})


def test_do_validation_resets_then_feeds_every_batch():
    m = M()

    class Eng(FakeEngine):
        def __init__(self):
            super().__init__()
            self.seen = []

        def set_batch(self, hits, n):
            self.batch = (hits, n)

        def eval_step(self):
            self.metric_acc[2] += torch.tensor(self.batch)
            self.losses.fill_(float(self.batch[0]))
            self.seen.append(self.batch)

    eng = Eng()
    eng.metric_acc.fill_(9)                                   # stale counters must not leak into the run
    metrics = m.pretrain_metrics()
    m.do_validation(eng, [(1, 2), (2, 3)], metrics)
    v = dict(zip(*metrics.get()))
    assert eng.seen == [(1, 2), (2, 3)] and v["MVRCAccuracy"] == pytest.approx(3 / 5) and v["MVRCLoss"] == 1.5 and math.isnan(v["MLMAcc"])
    loaded = []
    m.do_validation(eng, [7], metrics, load_batch=lambda b: (loaded.append(b), eng.set_batch(1, 1)))
    assert loaded == [7] and dict(zip(*metrics.get()))["MVRCAccuracy"] == 1.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _allreduce_worker(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = M()
    metrics = m.pretrain_metrics(allreduce=True, num_replicas=world)
    eng = FakeEngine()
    # rank 0: 1 of 2 (0.5); rank 1: 9 of 10 (0.9) -> 10 / 12, not the mean of ratios 0.7; MVRC: only rank 1 counted rows
    eng.metric_acc[0] = torch.tensor([1, 2] if rank == 0 else [9, 10])
    eng.metric_acc[2] = torch.tensor([0, 0] if rank == 0 else [1, 4])
    eng.losses.fill_(1.0 if rank == 0 else 3.0)
    metrics.update(eng)
    v = dict(zip(*metrics.get()))
    assert v["MLMAcc"] == (torch.tensor(10.0) / torch.tensor(12.0)).item() and abs(v["MLMAcc"] - 0.7) > 0.1, v
    assert v["MVRCAccuracy"] == 0.25 and v["MLMLoss"] == 2.0, v
    empty = m.pretrain_metrics(allreduce=True, num_replicas=world)
    assert all(math.isnan(x) for x in empty.get()[1])
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_sums_numerator_and_denominator_before_dividing():
    mp.spawn(_allreduce_worker, args=(2, _free_port()), nprocs=2, join=True)


# ---- the numpy restatement of the kernels against the reference's counts and losses ------------------------------------------
@pytest.mark.parametrize("case", ["plain", "multi"])
def test_kernel_restatement_agrees_with_the_reference_fixture(case, gold):
    V, C = int(gold["V"]), int(gold["C"])
    for b in range(N_BATCH):
        pre = "%s_b%d_" % (case, b)
        counts, losses = gold[case + "_counts"][b], gold[case + "_losses"][b]
        for sfx, row, slot in ((("_wvc", 0, 0), ("_aux", 1, 2)) if case == "multi" else (("", 0, 0),)):
            lg, lb = gold[pre + "mlm_logits" + sfx], gold[pre + "mlm_label" + sfx]
            # padding columns behind V filled with the largest value on the grid: they must be ignored
            padded = np.concatenate((lg.reshape(-1, V), np.full((lg.shape[0] * lg.shape[1], 3), 8.0, np.float32)), 1)
            r = MR.ce_eval_ref(padded, V, lb.reshape(-1))
            assert [r["hits"], r["n"]] == list(counts[row]), (case, b, sfx)
            if r["n"]:
                assert abs(r["loss"] - losses[slot]) <= 1e-5 * abs(losses[slot])
            assert (r["pred"] >= 0).sum() == r["n"] and r["pred"].max() < V
        s = MR.soft_ce_eval_ref(gold[pre + "mvrc_logits"].reshape(-1, C), C, gold[pre + "mvrc_label"].reshape(-1, C))
        assert [s["hits"], s["n"]] == list(counts[2]) and abs(s["loss"] - losses[1]) <= 1e-5 * abs(losses[1])
        assert not s["valid"][0] and not s["valid"][1] and s["valid"][2]       # sum 0, sum 1.2, the tied 0.5 / 0.5 row
        if case == "plain":
            r = MR.ce_eval_ref(gold[pre + "relationship_logits"], 2, gold[pre + "relationship_label"])
            assert [r["hits"], r["n"]] == list(counts[3]) and abs(r["loss"] - losses[3]) <= 1e-5 * abs(losses[3])
            assert r["pred"][0] == 0                                           # the planted tie: lowest index


def test_kernel_restatement_tie_and_empty_rules():
    x = np.full((3, 8), -4.0, np.float32)
    x[0, [2, 5]] = 1.0
    x[1, [2, 5]] = 1.0
    r = MR.ce_eval_ref(x, 6, np.array([2, 5, -1]))
    assert (r["hits"], r["n"], list(r["pred"])) == (1, 2, [2, 2, -1])
    e = MR.ce_eval_ref(x, 6, np.array([-1, -1, 7]))           # 7 >= V: not counted
    assert e["n"] == 0 and math.isnan(e["loss"]) and list(e["pred"]) == [-1, -1, -1]
    g = MR.grid_logits(np.random.RandomState(0), (4, 64))
    assert (g.astype(np.float16) == g).all() and (torch.from_numpy(g).to(torch.bfloat16).float().numpy() == g).all()
