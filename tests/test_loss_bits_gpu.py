"""The bits of the fused loss kernels (-m gpu): every entry point of csrc/loss.hip behind which a row kernel stands, in each of its DS x
ACC x logits_copy forms, on the inputs of tests/loss_bits_cases.py, against what the library wrote when the fixture was recorded
(tests/golden/loss_bits/loss_bits_small.npz, tools/make_loss_bits_golden.py: the commit before the row code was shared between the
plain and the row-weighted kernels).  Gradients are compared as 16-bit patterns with torch.equal, counters and counts exactly, a
loss slot -- a float atomicAdd across rows -- only where exactly one row adds to it (each entry point has such a launch);
elsewhere the tolerance tests of test_ops_gpu.py, test_train_metrics_gpu.py and test_objectives_gpu.py remain the check.  The build uses -ffp-contract=fast, so moving
code between functions can move a last bit (csrc/loss.hip, above online_merge_as_plain): this is the test that says it did not.

The fp16 build runs the same cases in one child process against the arrays recorded from the fp16 build."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:      # (run as a script by the fp16 child)
    sys.path.insert(0, ROOT)
from tests import loss_bits_cases as LB      # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, "tests", "golden", "loss_bits", "loss_bits_small.npz")
_cache = {}


def recorded():
    if "z" not in _cache:
        with np.load(FIXTURE, allow_pickle=False) as z:
            _cache["z"] = {str(k): z["blob_%d" % b] for k, b in zip(z["keys"], z["blob_of"])}
    return _cache["z"]


def compare(name):
    """-> number of outputs compared; raises on the first that differs."""
    want = {k: v for k, v in recorded().items() if k.startswith("%s/%s/" % (LB.precision(), name))}
    got = {"%s/%s" % (LB.precision(), k): v for k, v in LB.run(name).items()}
    assert sorted(got) == sorted(want) and want
    for k in sorted(got):
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert torch.equal(torch.from_numpy(g), torch.from_numpy(w)), "%s: %d of %d elements differ" % (k, int((g != w).sum()), g.size)
    return len(got)


def test_fixture_is_small_and_holds_both_builds():
    assert os.path.getsize(FIXTURE) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "objectives", "objectives_small.npz"))
    keys = sorted(recorded())
    for prec in ("bf16", "f16"):
        assert {k.split("/")[1] for k in keys if k.startswith(prec + "/")} == set(LB.CASES)
    assert [k[5:] for k in keys if k.startswith("bf16/")] == [k[4:] for k in keys if k.startswith("f16/")]


@pytest.mark.parametrize("name", sorted(LB.CASES))
def test_loss_entry_points_write_the_recorded_bits(name):
    compare(name)


def test_fp16_build_writes_the_recorded_bits():
    if LB.precision() == "f16":
        pytest.fail("the parent process already runs with VLB_PRECISION=f16")
    env = dict(os.environ, VLB_PRECISION="f16")
    env.pop("VLB_LIB_PATH", None)      # (an A/B run's bf16 library is not the fp16 build)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and "f16: all %d cases equal" % len(LB.CASES) in r.stdout


if __name__ == "__main__":
    assert LB.precision() == "f16"
    n = sum(compare(name) for name in sorted(LB.CASES))
    print("f16: all %d cases equal (%d outputs)" % (len(LB.CASES), n))
