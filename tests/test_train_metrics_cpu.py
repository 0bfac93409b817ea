"""CPU checks of the training-time metrics: the entry point's flag, the engine's refusal in module-API mode, the metric classes of
vl-bert_amd/common/metrics.py over a stand-in for PretrainEngine.train_metrics_source, and the host restatement of the counters
(tests/train_metrics_ref.py) against torch.argmax on the reference fixture's logits."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

from tests import train_metrics_ref as TR

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = os.path.join(HERE, "fixtures", "pretrain_small.yaml")


def test_dry_run_reports_the_flag_only_when_it_is_given(capsys):
    tr = importlib.import_module("vl-bert_amd.pretrain.train_end2end")
    plain = tr.main(["--cfg", CFG, "--dry-run"])
    out_plain = capsys.readouterr().out
    flagged = tr.main(["--cfg", CFG, "--dry-run", "--train-metrics"])
    out_flagged = capsys.readouterr().out
    assert "train_metrics" not in plain and "train_metrics" not in out_plain
    assert flagged == dict(plain, train_metrics=True) and '"train_metrics": true' in out_flagged
    assert "--train-metrics" in tr.parse_args.__globals__["__doc__"]
    with pytest.raises(SystemExit):
        tr.parse_args(["--help"])
    text = capsys.readouterr().out
    assert "--train-metrics" in text and "ETA" in text and "per-phase times" in " ".join(text.split()).replace("- ", "-")


def test_module_api_engine_refuses_train_metrics_by_name():
    E = importlib.import_module("vl-bert_amd.engine")
    with pytest.raises(ValueError, match="train_metrics=True") as e:
        E.PretrainEngine(E.ModelConfig(num_hidden_layers=2), 2, 8, 4, device="cpu", core=True, train_metrics=True)
    assert "core=True" in str(e.value)


class Source:
    """What the metric classes read of PretrainEngine.train_metrics_source: metric_acc, losses, reset_metrics()."""

    def __init__(self):
        self.metric_acc = torch.zeros((4, 2), dtype=torch.int64)
        self.losses = torch.zeros(4, dtype=torch.float32)

    def reset_metrics(self):
        self.metric_acc.zero_()


def test_metric_classes_move_the_training_counters_and_reset_per_epoch():
    m = importlib.import_module("vl-bert_amd.common.metrics")
    metrics = m.pretrain_metrics(loss_loggers=[("mlm_loss", "MLMLoss"), ("mvrc_loss", "MVRCLoss")])
    assert metrics.get()[0] == ["MLMAcc", "MVRCAccuracy", "MLMLoss", "MVRCLoss"]
    assert all(math.isnan(v) for v in metrics.get()[1])                       # nothing counted yet: the empty metric
    src = Source()
    for hits, n, mv, loss in ((1, 4, (0, 0), 2.0), (3, 4, (1, 2), 4.0)):        # two batches; the first has no valid MVRC row
        src.metric_acc[0] += torch.tensor([hits, n])                          # what a forward adds
        src.metric_acc[2] += torch.tensor(mv)
        src.losses.copy_(torch.tensor([loss, loss / 2, 0.0, 0.0]))
        metrics.update(src)
        assert int(src.metric_acc.abs().sum()) == 0                           # moved, not copied
    v = dict(zip(*metrics.get()))
    assert v == {"MLMAcc": 0.5, "MVRCAccuracy": 0.5, "MLMLoss": 3.0, "MVRCLoss": 1.5}
    metrics.reset()                                                            # epoch start
    assert all(math.isnan(x) for x in metrics.get()[1])
    src.metric_acc[0] += torch.tensor([2, 2])
    src.losses.fill_(2.0)
    metrics.update(src)
    v = dict(zip(*metrics.get()))
    assert v["MLMAcc"] == 1.0 and math.isnan(v["MVRCAccuracy"]) and v["MLMLoss"] == 2.0


@pytest.mark.parametrize("case", ["plain", "multi"])
def test_host_restatement_agrees_with_torch_argmax_on_the_fixture(case):
    g = dict(np.load(os.path.join(HERE, "golden", "metrics", "pretrain_metrics_small.npz"), allow_pickle=False))
    V, C = int(g["V"]), int(g["C"])

    def torch_hard(lg, lab, width):
        lg, lab = torch.from_numpy(lg).reshape(-1, lg.shape[-1])[:, :width], torch.from_numpy(lab).reshape(-1)
        keep = (lab >= 0) & (lab < width)
        return int((torch.argmax(lg[keep], 1) == lab[keep]).sum()), int(keep.sum())

    for b in range(3):
        pre = "%s_b%d_" % (case, b)
        heads, want = {}, {k: (0, 0) for k in TR.ROWS}
        for name, sfx in ((("mlm", "_wvc"), ("mlm_aux", "_aux")) if case == "multi" else (("mlm", ""),)):
            lg, lab = g[pre + "mlm_logits" + sfx], g[pre + "mlm_label" + sfx]
            heads[name] = (lg.reshape(-1, V), lab.reshape(-1))
            want[name] = torch_hard(lg, lab, V)
        xl, tl = torch.from_numpy(g[pre + "mvrc_logits"]).reshape(-1, C), torch.from_numpy(g[pre + "mvrc_label"]).reshape(-1, C)
        valid = (tl.sum(1) - 1.0).abs() < 0.1
        heads["mvrc"] = (xl.numpy(), tl.numpy())
        want["mvrc"] = (int((torch.argmax(xl[valid], 1) == torch.argmax(tl[valid], 1)).sum()), int(valid.sum()))
        if case == "plain":
            heads["relationship"] = (g[pre + "relationship_logits"], g[pre + "relationship_label"])
            want["relationship"] = torch_hard(g[pre + "relationship_logits"], g[pre + "relationship_label"], 2)
        got = TR.counts_ref(heads, V, C)
        assert got == want, (case, b, got, want)
        assert [list(got[k]) for k in TR.ROWS] == g[case + "_counts"][b].tolist()      # and both are the reference's own numbers
