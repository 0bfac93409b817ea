"""The per-kernel parity files on the IEEE fp16 build (libvlbert_hip_f16.so, -DVLB_ACT_F16).  One precision is chosen per process
(vl-bert_amd/_lib.py), so each case starts one child `python -m pytest <file> -m gpu -q -k <selection>` with VLB_PRECISION=f16 under
its own time limit and asserts: return code 0, exactly the hard-coded number of passed tests (from `pytest --collect-only -q -m gpu
-k <selection>`), no `failed`, no `skipped`.  The child's full output goes to f16_kernels_<file>.log in the directory of the parity
report (gpu_util.REPORT), its tail is printed.

A child that ends with a signal, an abort or at its time limit stops the runner: the remaining cases fail at once without starting
another process on the device.  The runner itself fails if the parent process already runs with VLB_PRECISION=f16.

Bars on the fp16 build: 16-bit outputs of tests/test_ops_gpu.py and tests/test_vision_gpu.py use gpu_util.bar16 (0.2 x the bf16
bar: 1e-2 -> 2e-3); fp32 outputs, the attention bars and the files that were written against act_dtype() from the start keep theirs.
"""
import os
import re
import subprocess
import sys
import tempfile
import time

import pytest

from tests.gpu_util import REPORT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.dirname(REPORT)          # where the parity report and the other logs of a run go

# tests/test_ops_gpu.py: everything but the workload-sized tests.  Of each epilogue battery the two smallest shapes per core / tile,
# one-tile-per-wg and mid-stream-drain: (1000, 520, 128) and (700, 2306, 384) are the small edge shapes of the large-tile core (the
# KEEPB = false tile takes its one-tile form only at (2600, 768, 768)), (1000, 520, 512) and (3232, 768, 768) those of the ring
# kernels -- every EPI instantiation of the fp16 object code, interior and edge drains.
OPS = ("not headline_shapes and not 256_tile_kernel_large_b_operand and not engine_step_through_large_tile_core "
       "and (not large_tile_core_epilogues or ((1000-520-128 or 700-2306-384) and not (4k0 and one-tile-per-wg)) "
       "or 2600-768-768-4k0-one-tile-per-wg) "
       "and (not ring_kernel_epilogues or 1000-520-512 or 3232-768-768)")
# tests/test_vision_gpu.py: the kernel tests (row-scaled weight gradients at their smallest shapes on either core), the e2e engine
# step and the VisionStack against the reference fixture; not the ResNet-101 headline-size and entry-point tests.
VISION = ("gemm_conv_epilogues or im2col or conv_weight_prepare_and_finalize or pool_and_resample or roi_align_nhwc "
          "or avgpool_rows_and_relu_mask or conv3x3_implicit_equals_explicit or conv3x3_forward_dgrad_wgrad "
          "or (test_wgrad_tn_rowscale and (300-70-198 or 64-128-128 or 2560-1500-1030 or refuses)) "
          "or (conv3x3_wgrad_tn_rowscale and not 40-512-512) or conv_prepare_batch "
          "or test_engine_e2e_step_vs_oracle or vision_stack_matches_reference_golden")
WHOLE = "not child and not fp16_build"

# (file, -k selection, N passed expected, time limit s)     # wall time of the child measured on an MI355X (the engine parity
# selection of tests/test_f16_build_gpu.py, the yardstick for "too long", has a limit of 1500 s)
CASES = [
    ("test_ops_gpu.py", OPS, 125, 300),                        # 17.6 s
    ("test_vision_gpu.py", VISION, 46, 300),                  # 7.6 s
    ("test_embed_attn_ops_gpu.py", WHOLE, 67, 180),           # 6.3 s
    ("test_step_ends_gpu.py", WHOLE, 31, 180),                # 4.3 s
    ("test_heads_gpu.py", WHOLE, 21, 180),                    # 4.3 s
    ("test_metrics_gpu.py", WHOLE, 16, 180),                  # 4.0 s
    ("test_refcoco_gpu.py", "test_grounding", 5, 180),       # 4.4 s
    ("test_f16_edges_gpu.py", "test_", 3, 180),              # 3.7 s
]
_stopped = []          # set by the first child that ended with a signal, an abort or at its time limit


@pytest.mark.parametrize("fname,select,expected,limit", CASES, ids=[c[0][len("test_"):-len("_gpu.py")] for c in CASES])
def test_kernel_parity_on_the_fp16_build(fname, select, expected, limit):
    if os.environ.get("VLB_PRECISION", "bf16").lower() in ("f16", "fp16"):
        pytest.fail("the parent process already runs with VLB_PRECISION=f16")
    if _stopped:
        pytest.fail("not started: %s" % _stopped[0])
    env = dict(os.environ, VLB_PRECISION="f16", PYTHONUNBUFFERED="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", fname), "-m", "gpu", "-q", "-s", "-k", select]
    try:          # the child writes its log as it runs (kept when it is killed at the time limit)
        os.makedirs(OUT_DIR, exist_ok=True)
        log = open(os.path.join(OUT_DIR, "f16_kernels_%s.log" % fname[:-len(".py")]), "w+")
    except OSError:
        log = tempfile.TemporaryFile("w+")
    t0 = time.time()
    with log, tempfile.TemporaryFile("w+") as errf:
        try:
            rc = subprocess.run(cmd, env=env, cwd=ROOT, stdout=log, stderr=errf, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        wall = time.time() - t0
        log.seek(0)
        errf.seek(0)
        out, err = log.read(), errf.read()
        log.seek(0, os.SEEK_END)
        log.write("\n---- stderr ----\n" + err + "\n---- return code %d, %.1f s ----\n" % (rc, wall))
    print(out[-4000:])
    print(err[-1500:])
    print("fp16 child %s: return code %d, %.1f s" % (fname, rc, wall))
    if rc < 0 or rc in (124, 134, 137, 139):
        _stopped.append("the fp16 child of %s ended with return code %d (signal, abort or time limit)" % (fname, rc))
        pytest.fail(_stopped[0])
    assert rc == 0, out[-3000:]
    summary = out.strip().splitlines()[-1] if out.strip() else ""
    m = re.search(r"(\d+) passed", summary)
    assert m and int(m.group(1)) == expected, "expected %d passed: %s" % (expected, summary)
    assert "failed" not in summary and "skipped" not in summary and "error" not in summary, summary
