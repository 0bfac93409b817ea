"""The GEMM kernels' work-item -> tile map (vl-bert_amd/csrc/tile_order.h) checked on the host: tests/tile_order_check.cpp includes the
header the kernels include, is built with the address and undefined-behaviour sanitizers and run directly.  It asserts that the map is
a bijection onto the tile grid for any tile count and group height, that every XCD owns one contiguous run, and the values of the
near-square group rule."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = next((c for c in (shutil.which(n) for n in ("c++", "g++", "clang++")) if c), None)

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler installed")


def test_tile_order_is_a_bijection_with_contiguous_xcd_runs(tmp_path):
    exe = str(tmp_path / "tile_order_check")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "tile_order_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert "tile order ok" in run.stdout
