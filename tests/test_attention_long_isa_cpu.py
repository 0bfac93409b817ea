"""Compile-outcome contracts of the streaming attention kernels (vl-bert_amd/csrc/attention_long.hip) on the ISA hipcc emits, in both
builds (no GPU: hipcc cross-compiles gfx950 here): nothing spills, no scratch, the register count at or under the occupancy step the
kernel header states (128 VGPRs: two 8-wave workgroups = 4 waves per SIMD), no instruction touches an LDS read still in flight, and
no load sits alone in front of a full wait (tools/isa_lint.py; see tests/test_isa_cpu.py for the short-sequence kernels)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(ROOT, "tools", "isa_lint.py"))
L = importlib.util.module_from_spec(spec)
spec.loader.exec_module(L)

pytestmark = pytest.mark.skipif(not L.available(), reason="hipcc not installed")
SRC = os.path.join(ROOT, "vl-bert_amd", "csrc", "attention_long.hip")
KERNELS = ("attn_long_fwd_kernel", "attn_long_bwd_kv_kernel", "attn_long_bwd_q_kernel")


def stated_vgpr_budget():
    """The budget the kernel header states: 'at most N VGPRs'."""
    with open(SRC) as f:
        head = f.read().split("#include")[0]
    m = re.search(r"at most (\d+) VGPRs", head)
    assert m, "the header of attention_long.hip must state its register budget"
    return int(m.group(1))


@pytest.mark.parametrize("defines", [(), ("-DVLB_ACT_F16",)], ids=["bf16", "f16"])
def test_streaming_attention_kernels_compile_clean(defines):
    budget = stated_vgpr_budget()
    assert budget == 128          # 512 registers per SIMD lane / 4 waves: what __launch_bounds__(512) + waves_per_eu(4, 4) assume
    ks = L.kernels(L.compile_isa(SRC, defines))
    assert len(ks) == len(KERNELS), sorted(ks)
    for name in KERNELS:
        k = L.find(ks, name)
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k["spill"], k["scratch"])
        assert k["vgpr"] + k["agpr"] <= budget, (name, k["vgpr"], k["agpr"])
        assert not L.landing_register_violations(k["body"]), name
        assert L.serialized_loads(k["body"]) == 0, name
        assert not any(re.match(r"^\s+scratch_", l) for l in k["body"]), name


def test_streaming_attention_prologues_issue_their_loads_in_one_burst():
    ks = L.kernels(L.compile_isa(SRC))
    # forward: K and V blocks (4 x 16 B per thread), the Q fragments (2), the mask row
    assert L.loads_before_first_wait(L.find(ks, "attn_long_fwd_kernel")["body"]) >= 7
    # dQ role: K and V blocks (4), Q / dO / O rows (6), lse, the mask row
    assert L.loads_before_first_wait(L.find(ks, "attn_long_bwd_q_kernel")["body"]) >= 12
    # dK / dV role: K and V rows (4), the key's mask
    assert L.loads_before_first_wait(L.find(ks, "attn_long_bwd_kv_kernel")["body"]) >= 5
