"""Per-kernel parity (-m gpu) of vlb_attention_probs (vl-bert_amd/csrc/attention_probs.hip): the attention probabilities of the fused
16-bit path, recomputed from the QKV and the row log-sum-exp a forward left behind, written in fp32.

The kernel alone: B = 5 (the five mask kinds of R.attn_masks: full | holes with key 0 masked | one live key | all zero | prefix of 1),
nh = 2, H = 128, qkv ~ N(0, 1) rounded to the 16-bit type (scaled scores of O(1)), lse from ops.attention_fwd on the same inputs, probs
into a sentinel-filled buffer with guard words on both sides.  Reference: float64 softmax(Q K^T / 8 + (1 - mask) * -10000) from the same
16-bit inputs over every query q < n, padded ones included (tests/attention_probs_ref.py).  Bar: 2e-3 absolute -- the project's lse
class (an lse error of delta is a relative error of delta in a value <= 1), and what the all-masked sample needs by itself: one fp32 ulp
of a score near -10000 is 9.8e-4.  The error per mask kind is printed.

S puts a single key, a partial 32-key group, exactly one 128-key block, one row in a second block, a ragged third block and the cap on
the kernel; n = S and n = S - 5 (n no multiple of 4, rows the kernel must not write), ldp = n rounded up to 32, and to 4 in two cases;
one case with ldp = 200 at S = 37 runs the zero fill of output columns beyond the last 128-key block.
"""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import attention_probs_ref as AR
from tests import embed_attn_refs as R
from tests.gpu_util import act_dtype, dev, pkg, report, to_gpu_bf16

pytestmark = pytest.mark.gpu
SENT = 7.25          # sentinel for memory the kernel must (or must not) overwrite
GUARD = 256          # floats in front of and behind the output
BAR = 2e-3
B, NH, H = 5, 2, 128
ERR_ARG = -1         # VLB_ERR_ARG (include/vlbert_hip.h)
SIZES = (1, 37, 128, 129, 301, 512)
BATTERY = sorted({(S, n, AR.ceil_to(n, 32)) for S in SIZES for n in (S, max(1, S - 5))}) + [(37, 37, 40), (301, 301, 304), (37, 37, 200)]
KIND = ("full", "holes", "one key", "all masked", "prefix of 1")


@pytest.fixture(scope="module")
def ops():
    o = pkg("ops")
    name, cus = pkg("_lib").device_info(0)
    assert name.startswith("gfx950"), "these kernels are built for gfx950 only (got %s)" % name
    return o


@functools.lru_cache(maxsize=None)
def host_case(S):
    """Inputs and the float64 references of one S, computed once and shared (left unchanged by every test)."""
    g = torch.Generator().manual_seed(500 + S)
    qkv = R.rounder(act_dtype())(torch.randn(B * S, 3 * H, generator=g))
    mask, kinds = R.attn_masks(B, S, seed=S)
    return dict(S=S, qkv=qkv, mask=mask, kinds=kinds, ref=AR.probs_ref(qkv, mask, B, S, H, NH),
                ref_nomask=AR.probs_ref(qkv, mask, B, S, H, NH, use_mask=False))


@functools.lru_cache(maxsize=None)
def case(S):
    c = host_case(S)
    return dict(c, qg=to_gpu_bf16(c["qkv"]), mg=c["mask"].to(dev()))


def forward(ops, c, p=0.0, seedv=0, tag=0):
    """ops.attention_fwd -> (ctx, lse, seed tensor)"""
    S = c["S"]
    seed = torch.tensor([seedv], dtype=torch.int32, device=dev())
    ctx = torch.full((B * S, H), SENT, dtype=act_dtype(), device=dev())
    lse = torch.full((B, NH, S), SENT, device=dev())
    ops.attention_fwd(c["qg"], c["mg"], ctx, lse, B, S, H, NH, drop_p=p, seed=seed, tag=tag)
    return ctx, lse, seed


def guarded(n, ldp):
    big = torch.full((GUARD + B * NH * n * ldp + GUARD,), SENT, device=dev())
    return big, big[GUARD:GUARD + B * NH * n * ldp].view(B, NH, n, ldp)


def guards_intact(big):
    return bool((big[:GUARD] == SENT).all()) and bool((big[-GUARD:] == SENT).all())


def run_probs(ops, c, lse, n, ldp, p=0.0, seed=None, tag=0):
    big, out = guarded(n, ldp)
    view = ops.attention_probs(c["qg"], c["mg"], lse, B, c["S"], H, NH, n=n, drop_p=p, seed=seed, tag=tag, out=out)
    torch.cuda.synchronize()
    assert view.shape == (B, NH, n, n) and guards_intact(big), "sentinel overwritten outside [b, h, q < n, k < ldp]"
    return out.cpu()


def max_err(got, ref):
    return float((got.double() - ref).abs().max())


@pytest.mark.parametrize("S,n,ldp", BATTERY)
def test_attention_probs_battery(ops, S, n, ldp):
    c = case(S)
    _, lse, _ = forward(ops, c)
    out = run_probs(ops, c, lse, n, ldp)
    kc = min(S, ldp)                                   # columns that hold keys
    got, ref = out[:, :, :, :kc], c["ref"][:, :, :n, :kc]
    name = "attention_probs S%d n%d ldp%d " % (S, n, ldp)
    assert bool(torch.isfinite(out).all())
    for b, k in enumerate(c["kinds"]):
        print(name + "%-12s max abs err %.3e" % (KIND[k], max_err(got[b], ref[b])))
    report(name + "vs float64", got, ref, BAR, 0)
    # the bar bites: another head's probabilities and the unmasked softmax both miss it (samples of kind 0 / 1: O(1) differences)
    if S > 1:
        assert max_err(got, ref.roll(1, dims=1)) > BAR
        assert max_err(got, c["ref_nomask"][:, :, :n, :kc]) > BAR
    # exact zeros: masked keys of every sample that has a live key; the columns beyond S
    live = torch.tensor([k != 3 for k in c["kinds"]])
    dead = (c["mask"][:, :kc] == 0) & live[:, None]
    assert float((got * dead[:, None, None, :]).abs().max()) == 0.0
    assert float(out[:, :, :, kc:].abs().max() if ldp > kc else 0.0) == 0.0
    if n == S:
        assert float((got.double().sum(-1) - 1.0).abs().max()) <= BAR


def test_the_two_mutant_references_differ_by_more_than_the_bar():
    """CPU only: the head-rolled and the unmasked float64 references are further than 2e-3 from the true one at every S > 1 of the
    battery, so 'the bar bites' above holds by construction."""
    for S in SIZES[1:]:
        c = host_case(S)
        assert max_err(c["ref"].roll(1, dims=1).float(), c["ref"]) > BAR and max_err(c["ref_nomask"].float(), c["ref"]) > BAR


@pytest.mark.parametrize("S", [37, 301])
def test_attention_probs_after_dropout_are_the_forwards(ops, S):
    """drop_p = 0.1: the result is P_eval x keep / (1 - p_eff) with the restated counter-RNG mask; rounded to the 16-bit type and
    multiplied with V it is the ctx the forward wrote under the same (seed, tag) -- the masks are the FORWARD's --, and another tag
    misses both."""
    c = case(S)
    p, seedv, tag = 0.1, 4242, 8
    ctx, lse, seed = forward(ops, c, p, seedv, tag)
    n, ldp = S, AR.ceil_to(S, 32)
    got = run_probs(ops, c, lse, n, ldp, p, seed, tag)[:, :, :, :S]
    ref = c["ref"] * AR.keep_scale(seedv, tag, B, NH, S, p)
    report("attention_probs S%d p0.1 vs float64 x keep / 0.9" % S, got, ref, BAR, 0)
    v = c["qkv"].view(B, S, 3, NH, 64)[:, :, 2].permute(0, 2, 1, 3).double()               # [B, nh, S, 64]
    ctx_ref = ctx.float().cpu().view(B, S, NH, 64).permute(0, 2, 1, 3)

    def ctx_of(pr):
        return (R.rounder(act_dtype())(pr).double() @ v).float()

    report("attention_probs S%d p0.1: probs (16-bit) @ V vs the forward's ctx" % S, ctx_of(got), ctx_ref, 2e-3, 1e-2)
    other = run_probs(ops, c, lse, n, ldp, p, seed, tag + 1)[:, :, :, :S]
    assert max_err(other, ref) > BAR
    assert max_err(ctx_of(other), ctx_ref.double()) > 2e-3 + 1e-2 * float(ctx_ref.abs().max())


def test_attention_probs_are_deterministic(ops):
    c = case(301)
    _, lse, seed = forward(ops, c, 0.1, 99, 16)
    first = run_probs(ops, c, lse, 301, 320, 0.1, seed, 16)
    again = run_probs(ops, c, lse, 301, 320, 0.1, seed, 16)
    assert torch.equal(first, again)


def test_argument_refusals_of_the_c_abi(ops):
    """S = 513, n = S + 1, ldp < n (with and without ldp % 4 == 0), ldp % 4 != 0, H != 64 nh and an output off a
    16-byte boundary return VLB_ERR_ARG before any launch:
    the sentinel-filled output is untouched."""
    lib = pkg("_lib").load()
    stream = torch.cuda.current_stream().cuda_stream
    S = 40
    qkv = torch.zeros((B * 520, 3 * H), dtype=act_dtype(), device=dev())
    mask = torch.ones((B, 520), device=dev())
    lse = torch.zeros((B, NH, 520), device=dev())
    out = torch.full((B * NH * 64 * 64,), SENT, device=dev())

    def rc(S, Hh, nh, n, ldp):
        return lib.vlb_attention_probs(qkv.data_ptr(), mask.data_ptr(), lse.data_ptr(), out.data_ptr(), B, S, Hh, nh, n, ldp, 0.0, None, 0,
                                       stream)

    assert rc(513, H, NH, 40, 64) == ERR_ARG and b"S=513" in lib.vlb_last_error()
    assert rc(S, H, NH, S + 1, 64) == ERR_ARG
    assert rc(S, H, NH, 40, 36) == ERR_ARG             # ldp < n, both multiples of 4
    assert rc(S, H, NH, 40, 39) == ERR_ARG             # ldp = n - 1
    assert rc(S, H, NH, 36, 38) == ERR_ARG             # ldp >= n but no multiple of 4
    assert rc(S, H + 64, NH, 40, 64) == ERR_ARG        # H != 64 nh
    assert rc(S, H, NH, 0, 64) == ERR_ARG
    odd = out[1:]                                      # 4 bytes off a 16-byte boundary: refused, not a faulting 16-byte store
    assert lib.vlb_attention_probs(qkv.data_ptr(), mask.data_ptr(), lse.data_ptr(), odd.data_ptr(), B, S, H, NH, 40, 40, 0.0, None, 0,
                                   stream) == ERR_ARG and b"16-byte aligned" in lib.vlb_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    with pytest.raises(RuntimeError, match="vlb_attention_probs"):
        ops.attention_probs(qkv, mask, lse, B, 513, H, NH, n=40)
    assert rc(S, H, NH, 40, 40) == 0                   # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert not bool((out[:B * NH * 40 * 40] == SENT).any()) and bool((out[B * NH * 40 * 40:] == SENT).all())


def test_attention_probs_battery_on_the_fp16_build_in_a_child_process():
    """The library's 16-bit type is chosen once per process (VLB_PRECISION): the battery runs again in a fresh child process on the
    IEEE fp16 build."""
    if os.environ.get("VLB_PRECISION", "bf16") == "f16":
        pytest.fail("the parent process already runs with VLB_PRECISION=f16")
    env = dict(os.environ, VLB_PRECISION="f16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-k", "test_attention_probs_battery and not child"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    print(r.stderr[-1000:])
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == len(BATTERY) and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
