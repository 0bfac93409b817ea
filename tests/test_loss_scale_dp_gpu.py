"""Dynamic loss scaling under data parallelism (-m gpu): two engine ranks share the one GPU over gloo, launched like the oracle anchor
of tests/test_dp_gpu.py; the per-rank body is tests/dp2_loss_scale_check.py.  An inf in ONE rank's local gradient must make BOTH ranks
skip (the decision rides on the reduced gradient / the all-reduced squared norm: no extra communication), and the first real step
after a first-step skip must gather correct 16-bit weights."""
import os

import pytest

from tests.test_dp_gpu import _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["sharded", "allreduce"])
def test_two_ranks_skip_together_and_stay_identical(mode):
    out = _run(["--mode", mode], tool=os.path.join("tests", "dp2_loss_scale_check.py"), marker="LOSS-SCALE DP OK=True")
    assert out.count("step 1 skipped on an inf in rank 1's local gradient; scale 512") == 2
