"""CPU checks of the fine-tuning evaluation layer: the numpy restatement of the kernels (tests/finetune_metrics_ref.py) against what
the REFERENCE's metric classes produced (tests/golden/metrics/finetune_metrics_small.npz, tools/make_finetune_metrics_golden.py);
the result-file writers of vl-bert_amd/common/finetune_eval.py byte for byte against the files the reference's json / pandas calls
wrote; the label-index handling of do_validation / joint_validation / ValidationMonitor on stub nets; the entry point's --dry-run."""
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import finetune_metrics_ref as FR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "metrics")
N_BATCH = 3
U = 2.0 ** -24                      # unit roundoff of fp32


def FE():
    return importlib.import_module("vl-bert_amd.common.finetune_eval")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "finetune_metrics_small.npz"), allow_pickle=False))


def batch(gold, case, b):
    pre = "%s_b%d_" % (case, b)
    return {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}


def restate(case, name, out, state):
    """One update of metric `name` by the restatement: state = (sum, count) -> (sum, count)."""
    s, n = state
    if name == "SoftAcc":
        r = FR.argmax_eval_ref(out["label_logits"], out["label_logits"].shape[1], FR.GATHER, out["label"], s, n)
    elif name == "Acc":
        r = FR.argmax_eval_ref(out["label_logits"], out["label_logits"].shape[1], FR.HARD, out["label"], s, n)
    elif name == "RefAcc":
        r = FR.argmax_eval_ref(out["label_logits"], out["label_logits"].shape[1], FR.GATHER_GT, out["label"], s, n)
    elif name == "JointAcc":
        C = out["answer_label_logits"].shape[1]
        h, rows = FR.joint_hits_ref(FR.argmax_ref(out["answer_label_logits"], C), out["answer_label"],
                                    FR.argmax_ref(out["rationale_label_logits"], C), out["rationale_label"])
        return s + h, n + rows
    elif name in ("ClsAcc", "ClsPosAcc", "ClsPosFrac"):
        a = FR.binary_cls_ref(out["label_logits"], out["label"], out["label_logits"].shape[1])
        num, den = {"ClsAcc": (0, 1), "ClsPosAcc": (2, 3), "ClsPosFrac": (3, 1)}[name]
        return s + a[num], n + a[den]
    else:
        raise KeyError(name)
    return r["sum"], r["count"]


LOSS_OUTPUT = {"AnsLoss": "ans_loss", "AnsLossLog": "ans_loss", "CNNRegLoss": "cnn_regularization_loss", "PosFraction": "positive_fraction",
               "ClsLoss": "cls_loss", "no_such_loss": "no_such_loss"}


@pytest.mark.parametrize("case", ["vqa", "vcr", "refcoco"])
def test_restatement_reproduces_the_reference_metric_classes(case, gold):
    names = [str(n) for n in gold[case + "_names"]]
    assert names == {"vqa": ["SoftAcc", "AnsLoss"], "vcr": ["Acc", "AnsLoss", "CNNRegLoss", "PosFraction", "AnsLossLog", "no_such_loss", "JointAcc"],
                     "refcoco": ["RefAcc", "ClsAcc", "ClsPosAcc", "ClsPosFrac", "ClsLoss"]}[case]
    for k, name in enumerate(names):
        state, soft_bound = (0, 0), 0.0
        for b in range(N_BATCH):
            out = batch(gold, case, b)
            ref_sum, ref_n = float(gold[case + "_sum_metric"][b, k]), float(gold[case + "_num_inst"][b, k])
            if name in LOSS_OUTPUT:
                # the reference adds float(mean) to an fp32 scalar; the mean of B fp32 values is good to B roundoffs, the add to one
                key = LOSS_OUTPUT[name]
                s = state[0]
                if key in out:
                    v = np.asarray(out[key], dtype=np.float64)
                    s = float(np.float32(np.float32(s) + np.float32(v.mean())))
                    assert abs(s - ref_sum) <= (v.size + 1) * U * abs(ref_sum), (name, b, s, ref_sum)
                else:
                    assert s == ref_sum, (name, b)
                state = (ref_sum, state[1] + 1)               # (continue from the reference's own fp32 value)
                assert state[1] == ref_n, (name, b)
                continue
            state = restate(case, name, out, state)
            assert state[1] == ref_n, (name, b, state, ref_n)
            if name == "SoftAcc":
                # the reference's fp32 per-batch .sum(): at most n * 2^-24 * sum(score) per batch (the fp32 summation bound)
                n_rows = out["label_logits"].shape[0]
                score = FR.argmax_eval_ref(out["label_logits"], out["label_logits"].shape[1], FR.GATHER, out["label"])["score"]
                soft_bound += n_rows * U * float(np.abs(score.astype(np.float64)).sum())
                print("SoftAcc batch %d: restatement %.17g reference %.17g |diff| %.3e bound %.3e" % (b, state[0], ref_sum, abs(state[0] - ref_sum), soft_bound))
                assert abs(state[0] - ref_sum) <= soft_bound, (b, state[0], ref_sum, soft_bound)
            else:
                assert state[0] == ref_sum, (name, b, state, ref_sum)
        value, ref = (FR.fp32_div(*state) if state[1] else float("nan")), float(gold[case + "_values"][k])
        assert (math.isnan(value) and math.isnan(ref)) or abs(value - ref) <= 2.0 ** -23 * abs(ref) + (soft_bound / state[1] if name == "SoftAcc" else 0.0), \
            (name, value, ref)


def test_restatement_argmax_rules_are_those_of_torch_argmax():
    x = np.array([[1.0, 3.0, 3.0, 2.0], [0.0, np.nan, 5.0, np.nan], [-np.inf] * 4, [np.inf, np.nan, np.inf, 0.0]], np.float32)
    want = torch.from_numpy(x).argmax(1).tolist()
    assert want == [1, 1, 0, 1] and FR.argmax_ref(x, 4).tolist() == want
    padded = np.concatenate((x, np.full((4, 2), 8.0, np.float32)), 1)
    assert FR.argmax_ref(padded, 4).tolist() == want                      # columns >= C are never read
    assert FR.binary_cls_ref(np.array([[0.0, -1e-30, 1e-30, np.nan, 2.0, 2.0]], np.float32),
                             np.array([[0.0, 1.0, 0.7, -0.5, -1.0, 1.0]], np.float32), 6) == [3, 5, 1, 2]
    assert FR.joint_hits_ref([1, 2, 3], [1, 2, 0], [0, 1, 3], [0, 0, 3]) == [1, 3]


# ---- result files ----------------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    with open(a, "rb") as f, open(b, "rb") as g:
        return f.read() == g.read()


def test_vqa_and_refcoco_writers_reproduce_the_fixture_files(gold, tmp_path):
    fe = FE()
    p = str(tmp_path / "vqa.json")
    fe.write_vqa_result(p, gold["vqa_question_ids"], gold["vqa_answer_ids"], [str(a) for a in gold["vqa_answer_vocab"]])
    assert same_bytes(p, os.path.join(GOLD, "vqa_result.json"))
    fe.write_vqa_result(p, gold["vqa_question_ids"].tolist(), torch.from_numpy(gold["vqa_answer_ids"]), [str(a) for a in gold["vqa_answer_vocab"]])
    assert same_bytes(p, os.path.join(GOLD, "vqa_result.json"))
    q = str(tmp_path / "ref.json")
    for boxes in (gold["refcoco_pred_boxes"], torch.from_numpy(gold["refcoco_pred_boxes"]), gold["refcoco_pred_boxes"].tolist()):
        fe.write_refcoco_result(q, gold["refcoco_ref_ids"], boxes)
        assert same_bytes(q, os.path.join(GOLD, "refcoco_result.json"))
    with open(q) as f:
        assert [r["ref_id"] for r in json.load(f)] == gold["refcoco_ref_ids"].tolist()


@pytest.mark.parametrize("task", ["Q2A", "QA2R"])
def test_vcr_writer_reproduces_the_fixture_files(task, gold, tmp_path):
    fe = FE()
    c, n = str(tmp_path / "r.csv"), str(tmp_path / "r.npy")
    fe.write_vcr_result(c, n, [str(a) for a in gold["vcr_%s_annot_ids" % task]], gold["vcr_%s_probs" % task], task)
    assert same_bytes(c, os.path.join(GOLD, "vcr_result_%s.csv" % task))
    assert same_bytes(n, os.path.join(GOLD, "vcr_result_%s.npy" % task))
    with open(c) as f:
        head = f.readline().strip().split(",")
    assert head[0] == "annot_id" and head[1:] == fe.vcr_columns(task) and len(head) == (5 if task == "Q2A" else 17)
    with pytest.raises(ValueError):
        fe.write_vcr_result(c, n, ["a"], gold["vcr_%s_probs" % task][:1, :3], task)
    with pytest.raises(ValueError):
        fe.vcr_columns("R2A")


def test_vcr_merge_reproduces_the_fixture_file(tmp_path):
    fe = FE()
    out = str(tmp_path / "sub" / "merged.csv")                           # the directory is made, as merge_result does
    fe.merge_vcr_results(os.path.join(GOLD, "vcr_result_Q2A.csv"), os.path.join(GOLD, "vcr_result_QA2R.csv"), out)
    assert same_bytes(out, os.path.join(GOLD, "vcr_result_merged.csv"))
    with open(out) as f:
        lines = f.read().splitlines()
    assert [l.split(",")[0] for l in lines[1:]] == ["test-0", "test-1", "test-3", "test-4"]       # inner join, the left file's order


def test_refcoco_accuracy_follows_the_reference_iou_convention():
    fe = FE()
    gt = [[0, 0, 9, 9]]                                   # xywh -> xyxy (0, 0, 9, 9): 10 x 10 pixels with the +1 convention
    assert fe.refcoco_accuracy([[0, 0, 9, 9]], gt) == 1.0
    # IoU exactly 0.5: the prediction covers the left half, 50 of 100 pixels -- counts (>=)
    half = np.array([[0, 0, 4, 9]], dtype=np.float64)
    assert fe.calculate_iou(half, np.array([[0, 0, 9, 9]], dtype=np.float64))[0] == 0.5
    assert fe.refcoco_accuracy(half, gt) == 1.0
    assert fe.refcoco_accuracy([[0, 0, 3, 9]], gt) == 0.0                # 40 / 100
    # without the +1 the left half would be 4 * 9 / 81 < 0.5: the convention matters
    # degenerate boxes: a point prediction (1 pixel with +1), an inverted one (negative area), a zero-size ground truth
    assert fe.refcoco_accuracy([[5, 5, 5, 5]], gt) == 0.0                # 1 / 100
    assert fe.refcoco_accuracy([[5, 5, 5, 5]], [[5, 5, 0, 0]]) == 1.0    # point on point: 1 / 1
    assert fe.refcoco_accuracy([[9, 9, 0, 0]], gt) == 0.0                # inverted: the areas go negative, as in the reference
    acc = fe.refcoco_accuracy([[0, 0, 9, 9], [0, 0, 3, 9], [0, 0, 4, 9], [50, 50, 60, 60]], [[0, 0, 9, 9]] * 4)
    assert acc == 0.5
    gt_in = np.array([[1.0, 2.0, 3.0, 4.0]])
    fe.refcoco_accuracy([[1, 2, 4, 6]], gt_in)
    assert gt_in.tolist() == [[1.0, 2.0, 3.0, 4.0]]                      # the caller's array is not modified


# ---- validation loops on stub nets -------------------------------------------------------------------------------------------
class StubNet:
    def __init__(self, tag):
        self.tag, self.calls, self.mode = tag, [], None

    def eval(self):
        self.mode = "eval"
        return self

    def __call__(self, *datas):
        assert self.mode == "eval" and not torch.is_grad_enabled()
        self.calls.append([None if d is None else int(d.reshape(-1)[0]) for d in datas])
        return {"label_logits": torch.tensor([[float(len(self.calls))]]), "tag": self.tag}


class StubMetrics:
    def __init__(self):
        self.updates, self.resets = [], 0

    def reset(self):
        self.resets += 1
        self.updates = []

    def update(self, outputs):
        self.updates.append(outputs)

    def get(self):
        return ["Acc"], [0.25 * len(self.updates)]


def stub_batch(base, n=9):
    return [torch.tensor([base + i]) for i in range(n)]


@pytest.mark.parametrize("index", [-1, 7])
def test_do_validation_takes_the_label_out_by_index(index):
    fe = FE()
    net, metrics = StubNet("a"), StubMetrics()
    metrics.updates = ["stale"]
    loader = [stub_batch(0), stub_batch(100)]
    loader[1][4] = None                                                   # (a None entry passes through, as VCR's align matrices)
    fe.do_validation(net, loader, metrics, index)
    pos = index % 9
    want = [i for i in range(9) if i != pos]
    assert net.mode == "eval" and metrics.resets == 1 and len(metrics.updates) == 2
    assert net.calls[0] == want and net.calls[1] == [None if i == 4 else 100 + i for i in want]
    assert [int(o["label"]) for o in metrics.updates] == [pos, 100 + pos]
    assert [float(o["label_logits"]) for o in metrics.updates] == [1.0, 2.0]


@pytest.mark.parametrize("index", [-1, 7])
def test_joint_validation_prefixes_the_outputs_and_takes_both_labels_out(index):
    fe = FE()
    a, r, metrics = StubNet("a"), StubNet("r"), StubMetrics()
    fe.joint_validation(a, r, [stub_batch(0), stub_batch(20)], [stub_batch(1000), stub_batch(1020), stub_batch(1040)], metrics, index)
    pos = index % 9
    want = [i for i in range(9) if i != pos]
    assert a.mode == r.mode == "eval" and metrics.resets == 1 and len(metrics.updates) == 2       # zip: the shorter loader ends it
    assert a.calls == [want, [20 + i for i in want]] and r.calls == [[1000 + i for i in want], [1020 + i for i in want]]
    o = metrics.updates[1]
    assert (o["answer_tag"], o["rationale_tag"]) == ("a", "r")
    assert (int(o["answer_label"]), int(o["rationale_label"])) == (20 + pos, 1020 + pos)
    assert {"answer_label_logits", "rationale_label_logits"} <= set(o) and "label" not in o


def test_validation_monitor_hands_the_label_index_to_the_val_func(capsys):
    M = importlib.import_module("vl-bert_amd.common.metrics")
    fe = FE()
    for index in (-1, 7):
        net, metrics = StubNet("a"), StubMetrics()
        mon = M.ValidationMonitor(fe.do_validation, [stub_batch(0)], metrics, host_metric_name="Acc", label_index_in_batch=index)
        assert mon.load_batch == index
        mon(0, net)
        assert [int(o["label"]) for o in metrics.updates] == [index % 9] and net.calls == [[i for i in range(9) if i != index % 9]]
        assert (mon.best_epoch, mon.best_val) == (0, 0.25)
    out = capsys.readouterr().out.splitlines()
    assert "Epoch[0] \tVal-Acc=0.250000,\t" in out
    old = M.ValidationMonitor(lambda *a: None, "loader", StubMetrics())       # the keyword is optional: the old form is unchanged
    assert old.load_batch is None
    assert M.ValidationMonitor(lambda *a: None, "loader", StubMetrics(), load_batch=len).load_batch is len


def test_composite_feeds_outputs_dicts_and_engines_alike():
    M = importlib.import_module("vl-bert_amd.common.metrics")

    class Count(M.EvalMetric):
        def update(self, source):
            self._add(torch.tensor(1), torch.tensor(2))

    comp = M.CompositeEvalMetric()
    comp.add(Count("c"))
    comp.update({"label_logits": None})                                    # a dict has no counters to clear
    assert comp.get() == (["c"], [0.5])


# ---- the entry point -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["vqa", "vcr", "refcoco"])
def test_dry_run_is_unchanged_without_val_steps(task, capsys):
    F = importlib.import_module("vl-bert_amd.common.finetune_entry")
    cfg = os.path.join(HERE, "fixtures", task + "_small.yaml")
    r = F.main(task, ["--cfg", cfg, "--dry-run"])
    out = capsys.readouterr().out
    assert list(r) == ["task", "module", "per_gpu_batch", "accumulate", "world", "lr", "optimizer", "momentum", "weight_decay", "clip_grad_norm",
                       "lr_schedule", "warmup_steps", "compute", "loss_scale", "precomputed", "seed"]
    config = F.load_config(task, cfg)
    assert out == json.dumps({"resolved": r, "NETWORK.VLBERT": dict(config.NETWORK.VLBERT)}, indent=1, default=str) + "\n"
    r2 = F.main(task, ["--cfg", cfg, "--dry-run", "--val-steps", "3"])
    assert r2 == r and capsys.readouterr().out == out
    args = F.parse_args(task, ["--cfg", cfg])
    assert args.val_steps == 0
    assert F.VAL_LABEL_INDEX == {"vqa": 4, "refcoco": 4, "vcr": 7}
