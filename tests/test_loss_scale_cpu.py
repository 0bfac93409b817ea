"""CPU checks of dynamic loss scaling: the numpy restatement of the rule (tests/loss_scale_ref.py) on a hand-written trajectory, how the
entry points resolve TRAIN.FP16_LOSS_SCALE, and the scaler's checkpoint key (host dict only: no GPU here)."""
import importlib
import os

import numpy as np
import pytest

from tests import loss_scale_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def LS():
    return importlib.import_module("vl-bert_amd.loss_scale")


def test_reference_rule_on_a_hand_written_trajectory():
    """Overflow at step 1, growth at the interval, the clamps at min and max -- every expected number written out by hand."""
    s = R.initial(init_scale=8.0, growth_interval=3, min_scale=2.0, max_scale=16.0)
    #        overflow   scale  unskipped  skipped_total  skipped_in_a_row
    steps = [(True,     4.0,   0,         1,             1),      # step 1 overflows: halve, count
             (False,    4.0,   1,         1,             0),
             (False,    4.0,   2,         1,             0),
             (False,    8.0,   0,         1,             0),      # third clean step = the interval: double, window restarts
             (True,     4.0,   0,         2,             1),
             (True,     2.0,   0,         3,             2),
             (True,     2.0,   0,         4,             3),      # floor: max(min_scale, 1.0)
             (False,    2.0,   1,         4,             0),
             (True,     2.0,   0,         5,             1),      # an overflow restarts the window
             (False,    2.0,   1,         5,             0),
             (False,    2.0,   2,         5,             0),
             (False,    4.0,   0,         5,             0),
             (False,    4.0,   1,         5,             0),
             (False,    4.0,   2,         5,             0),
             (False,    8.0,   0,         5,             0),
             (False,    8.0,   1,         5,             0),
             (False,    8.0,   2,         5,             0),
             (False,    16.0,  0,         5,             0),
             (False,    16.0,  1,         5,             0),
             (False,    16.0,  2,         5,             0),
             (False,    16.0,  0,         5,             0)]      # ceiling: min(max_scale, 32.0)
    for i, (ovf, scale, unskipped, total, in_a_row) in enumerate(steps):
        s = R.update(s, ovf)
        assert (float(s[0]), int(s[4]), int(s[5]), int(s[6])) == (scale, unskipped, total, in_a_row), "step %d" % (i + 1)
        assert list(s[[1, 2, 3, 7, 8]]) == [2.0, 0.5, 3.0, 2.0, 16.0]      # the configuration never moves
    assert s.dtype == np.float32
    assert R.run(R.initial(init_scale=8.0, growth_interval=3, min_scale=2.0, max_scale=16.0), [t[0] for t in steps])[-1].tolist() == s.tolist()
    # what counts as an overflow: the fp32 squared norm is inf or NaN (a finite gradient whose sum of squares overflows included)
    assert R.overflowed(np.inf) and R.overflowed(np.nan) and R.overflowed(1e39) and not R.overflowed(3.0e38) and not R.overflowed(0.0)


def test_defaults_are_apex_plus_a_floor():
    d = R.as_dict(R.initial())
    assert d == dict(scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, unskipped=0, skipped_total=0,
                     skipped_in_a_row=0, min_scale=1.0, max_scale=16777216.0)
    L = LS()
    assert L.FIELDS == R.FIELDS and L.DynamicLossScale().initial_values() == R.initial().tolist()
    assert L.values_to_dict(L.DynamicLossScale().initial_values()) == d
    # thirty-two halvings from any legal scale reach the floor
    s = R.initial(init_scale=2.0 ** 24)
    floor = R.run(s, [True] * L.MAX_SKIPPED_IN_A_ROW)[-1]
    assert float(floor[0]) == 1.0 and L.stuck(floor.tolist())
    # a gentler backoff has not reached its floor after 32 skips: that run is still recovering, not stuck
    slow = R.run(R.initial(init_scale=2.0 ** 16, backoff_factor=0.9), [True] * L.MAX_SKIPPED_IN_A_ROW)[-1]
    assert float(slow[0]) > 1.0 and int(slow[6]) == 32 and not L.stuck(slow.tolist())
    assert len({L.DynamicLossScale(), L.DynamicLossScale(), L.DynamicLossScale(init_scale=2.0)}) == 2      # hashable, by value
    assert isinstance(L.resolve("dynamic"), L.DynamicLossScale) and L.resolve(None) is None and L.resolve(4096.0) is None
    with pytest.raises(ValueError):
        L.resolve("static")
    with pytest.raises(ValueError):
        L.DynamicLossScale(init_scale=0.5)           # below the floor
    with pytest.raises(ValueError):
        L.DynamicLossScale(growth_interval=0)


def test_dry_run_resolves_fp16_loss_scale(tmp_path):
    tr = importlib.import_module("vl-bert_amd.pretrain.train_end2end")
    mine = os.path.join(ROOT, "cfgs", "pretrain", "base_e2e_16x16G_fp16.yaml")
    assert tr.main(["--cfg", mine, "--dry-run"])["loss_scale"] == "dynamic"
    ref = "/root/reference/cfgs/pretrain/base_e2e_16x16G_fp16.yaml"
    if os.path.isfile(ref):
        assert tr.main(["--cfg", ref, "--dry-run"])["loss_scale"] == "dynamic"
    F = importlib.import_module("vl-bert_amd.common.finetune_entry")
    fx = os.path.join(ROOT, "tests", "fixtures", "vcr_small.yaml")
    r = F.main("vcr", ["--cfg", fx, "--dry-run", "--compute", "cfg"])
    assert r["loss_scale"] == 128.0 and isinstance(r["loss_scale"], float)
    # the same file asking for the dynamic scaler, and a numeric value in a pre-training file
    y = tmp_path / "vcr_dynamic.yaml"
    y.write_text(open(fx).read().replace("FP16_LOSS_SCALE: 128.0", "FP16_LOSS_SCALE: 'dynamic'"))
    assert F.main("vcr", ["--cfg", str(y), "--dry-run", "--compute", "cfg"])["loss_scale"] == "dynamic"
    y2 = tmp_path / "pre_static.yaml"
    y2.write_text(open(mine).read().replace("FP16_LOSS_SCALE: 'dynamic'", "FP16_LOSS_SCALE: 1024"))
    assert tr.main(["--cfg", str(y2), "--dry-run"])["loss_scale"] == 1024.0


def test_checkpoint_round_trip_of_the_scaler_key():
    L = LS()
    spec = L.DynamicLossScale(init_scale=2.0 ** 12, growth_interval=500)
    values = R.run(np.array(spec.initial_values(), dtype=np.float32), [True, True, False, False])[-1].tolist()
    ck = {"state_dict": {}, "optimizer": {}}
    L.put_in_checkpoint(ck, values)
    assert set(ck) == {"state_dict", "optimizer", L.CHECKPOINT_KEY}      # one extra top-level key, the reference's two untouched
    assert ck[L.CHECKPOINT_KEY] == dict(scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=500, unskipped=2, skipped_total=2,
                                        skipped_in_a_row=0, min_scale=1.0, max_scale=2.0 ** 24)
    assert L.values_from_checkpoint(ck, spec) == values
    # a checkpoint without the key (a static run's, or the reference's): the initial state; a static run stores nothing
    plain = L.put_in_checkpoint({"state_dict": {}, "optimizer": {}}, None)
    assert L.CHECKPOINT_KEY not in plain and L.values_from_checkpoint(plain, spec) == spec.initial_values()
    with pytest.raises(ValueError):
        L.values_from_checkpoint({L.CHECKPOINT_KEY: {"scale": 2.0}}, spec)
    C = importlib.import_module("vl-bert_amd.common.checkpoint")
    assert C.put_in_checkpoint is L.put_in_checkpoint and C.values_from_checkpoint is L.values_from_checkpoint
