"""Per-kernel parity (-m gpu) of the streaming attention kernels for 256 < S <= 512 (vl-bert_amd/csrc/attention_long.hip): forward
with the online softmax over key blocks of 128, the two backward roles (dK / dV per key block, dQ per query block).

Built like test_attention_masks_and_short_sequences (tests/test_embed_attn_ops_gpu.py): float64 reference R.attn_ref on the same
16-bit-rounded inputs, the dropout mask from gpu_util.keep_mask over R.attn_drop_index, the five mask kinds of R.attn_masks (b % 5:
full | holes with key 0 masked | one live key anywhere | all zero | prefix of 1), results per group of R.attn_groups, and the same bars:
lse 2e-3 + 1e-3, ctx 2e-3 + 1e-2, gradients 2e-3 + 2e-2; dq / dk of the one-key samples max(class bar, 4 x the error of the rounding
restatement R.attn_rounded_f32 against the float64 reference on the same inputs), printed.

The S values put one key, a full block and one past it on the boundaries of the 128-key blocks (257, 383 / 384 / 385, 511 / 512) and
inside a block at an odd length (288 is a multiple of 32, 449 leaves one key in the last 32-key block).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import embed_attn_refs as R
from tests.gpu_util import act_dtype, dev, drop_scale, drop_thr, keep_mask, pkg, report, to_gpu_bf16

pytestmark = pytest.mark.gpu
SENT = 7.25          # sentinel for memory a kernel must overwrite
BATTERY = [(5, s, 2, 0.0) for s in (257, 288, 383, 384, 385, 449, 511, 512)] + \
          [(5, 257, 2, 0.1), (5, 385, 2, 0.1), (5, 512, 2, 0.1), (5, 300, 12, 0.1), (3, 300, 16, 0.0)]


@pytest.fixture(scope="module")
def ops():
    o = pkg("ops")
    name, cus = pkg("_lib").device_info(0)
    assert name.startswith("gfx950"), "these kernels are built for gfx950 only (got %s)" % name
    return o


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return R.rounder(act_dtype())(torch.randn(*shape, generator=g))


def a16(*shape, fill=0.0):
    return torch.full(shape, fill, dtype=act_dtype(), device=dev())


def run_attention(ops, qkv, mask, dctx, B, S, nh, p, seedv, tag):
    """Forward + backward into sentinel-filled outputs.  Returns (ctx, lse, dqkv) on the device."""
    H = nh * 64
    seed = torch.tensor([seedv], dtype=torch.int32, device=dev())
    qg, mg = to_gpu_bf16(qkv), mask.to(dev())
    ctx = a16(B * S, H, fill=SENT)
    lse = torch.full((B, nh, S), SENT, device=dev())
    ops.attention_fwd(qg, mg, ctx, lse, B, S, H, nh, drop_p=p, seed=seed, tag=tag)
    dqkv = a16(B * S, 3 * H, fill=SENT)
    ops.attention_bwd(qg, mg, ctx, lse, to_gpu_bf16(dctx), dqkv, B, S, H, nh, drop_p=p, seed=seed, tag=tag)
    torch.cuda.synchronize()
    return ctx, lse, dqkv


@pytest.mark.parametrize("B,S,nh,p", BATTERY)
def test_long_attention_battery(ops, B, S, nh, p):
    H = nh * 64
    qkv, dctx = rnd(B * S, 3 * H, seed=30 + S), rnd(B * S, H, seed=32 + S)
    mask, kinds = R.attn_masks(B, S, seed=S)
    tag, seedv = 3, 777
    thr = drop_thr(p)
    keep = None
    if thr:
        keep = keep_mask(seedv, tag, R.attn_drop_index(B, nh, S), thr).reshape(B, nh, S, S)
        keep = torch.from_numpy(keep.astype(np.float64)) * drop_scale(thr)
    ctx_ref, lse_ref, g_ref = R.attn_ref(qkv, mask, B, S, H, nh, keep=keep, dctx=dctx)
    _, g32 = R.attn_rounded_f32(qkv, mask, B, S, H, nh, act_dtype(), keep=None if keep is None else keep.float(), dctx=dctx)
    ctx, lse, dqkv = run_attention(ops, qkv, mask, dctx, B, S, nh, p, seedv, tag)
    assert bool(torch.isfinite(ctx.float()).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(dqkv.float()).all())
    name = "attn-long B%d S%d h%d p%.1f " % (B, S, nh, p)
    zero_b = torch.tensor([k == 3 for k in kinds])
    report(name + "lse", lse.cpu()[~zero_b], lse_ref[~zero_b], 2e-3, 1e-3)
    if zero_b.any():
        report(name + "lse all-zero sample", lse.cpu()[zero_b], lse_ref[zero_b], 2e-3, 1e-3)
    for gname, rows in R.attn_groups(mask, kinds, S).items():
        if not rows.any():
            continue
        report(name + "ctx " + gname, ctx.cpu()[rows], ctx_ref[rows], 2e-3, 1e-2)
        for j, nm in enumerate(("dq", "dk", "dv")):
            got, ref = dqkv.cpu()[rows, j * H:(j + 1) * H], g_ref[rows, j * H:(j + 1) * H]
            if gname == "one-key samples" and nm != "dv":
                err32 = (g32[rows, j * H:(j + 1) * H].double() - ref).abs().max().item()
                print(name + nm + " one-key samples: error of the rounding restatement %.3e" % err32)
                report(name + nm + " " + gname, got, ref, max(R.bar(ref, (2e-3, 2e-2)), 4 * err32), 0.0)
            else:
                report(name + nm + " " + gname, got, ref, 2e-3, 2e-2)


def test_long_attention_is_deterministic(ops):
    """Forward + backward twice from the same inputs and seed: bit-identical (no atomics, no cross-workgroup sums)."""
    B, S, nh, p = 5, 385, 2, 0.1
    H = nh * 64
    qkv, dctx = rnd(B * S, 3 * H, seed=1), rnd(B * S, H, seed=2)
    mask, _ = R.attn_masks(B, S, seed=S)
    first = run_attention(ops, qkv, mask, dctx, B, S, nh, p, 4242, 5)
    again = run_attention(ops, qkv, mask, dctx, B, S, nh, p, 4242, 5)
    for nm, a, b in zip(("ctx", "lse", "dqkv"), first, again):
        assert torch.equal(a, b), nm


def test_sequence_length_limits_of_the_c_abi(ops):
    """S = 513 is refused with the library's argument error (naming 512); 256 (whole-sequence kernels) and 257 (streaming) both run."""
    nh, H, B = 2, 128, 1
    for S in (256, 257):
        qkv = rnd(B * S, 3 * H, seed=S)
        mask = torch.ones(B, S)
        ctx, lse = a16(B * S, H, fill=SENT), torch.full((B, nh, S), SENT, device=dev())
        ops.attention_fwd(to_gpu_bf16(qkv), mask.to(dev()), ctx, lse, B, S, H, nh)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ctx.float()).all()) and not bool((lse == SENT).any())
    S = 513
    qkv = a16(B * S, 3 * H)
    mask = torch.ones(B, S, device=dev())
    ctx, lse = a16(B * S, H), torch.zeros((B, nh, S), device=dev())
    with pytest.raises(RuntimeError, match=r"S=513 unsupported \(1\.\.512\)"):
        ops.attention_fwd(qkv, mask, ctx, lse, B, S, H, nh)
    with pytest.raises(RuntimeError, match=r"S=513 unsupported \(1\.\.512\)"):
        ops.attention_bwd(qkv, mask, ctx, lse, a16(B * S, H), a16(B * S, 3 * H), B, S, H, nh)


def test_long_attention_battery_on_the_fp16_build_in_a_child_process():
    """The library's 16-bit type is chosen once per process (VLB_PRECISION): the battery runs again in a fresh child process on the
    IEEE fp16 build."""
    if os.environ.get("VLB_PRECISION", "bf16") == "f16":
        pytest.fail("the parent process already runs with VLB_PRECISION=f16")
    env = dict(os.environ, VLB_PRECISION="f16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-k", "test_long_attention_battery and not child"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    print(r.stderr[-1000:])
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == len(BATTERY) and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
