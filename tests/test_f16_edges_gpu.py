"""Tests that only make sense on the IEEE fp16 build (VLB_PRECISION=f16, libvlbert_hip_f16.so): inputs spread over fp16's exponent
range, subnormals included.  Skipped on the bf16 build; tests/test_f16_kernels_gpu.py runs this file in a child process on the fp16
build (one precision per process, vl-bert_amd/_lib.py).

ROIAlign gather backward: `roi_align_nhwc_bwd_gather_kernel` (csrc/vision.hip) used to decode `dout` and `act` by bit pattern as
bfloat16 on both builds (an fp16 1.0 = 0x3C00 read as 2^-7); with the decode through bflo / bfhi the kernel follows the build's type.
fp16-subnormal GEMM operands: what the matrix instruction does with subnormal inputs decides how far below 2^-14 a scaled gradient may
fall before its products vanish (the static loss scale of 4096).
"""
import os

import numpy as np
import pytest
import torch

from oracle import roi_align_oracle as RA
from tests.gpu_util import bar16, dev, pkg, report

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("VLB_PRECISION", "bf16").lower() not in ("f16", "fp16"),
                                 reason="fp16 build only (child of tests/test_f16_kernels_gpu.py)")]


@pytest.fixture(scope="module")
def ops():
    o = pkg("ops")
    assert o.BF16 == torch.float16, "VLB_PRECISION=f16 did not select the fp16 build"
    return o


def h16(t):
    """Round to IEEE fp16 (subnormals kept), back in fp32."""
    return t.to(torch.float16).float()


@pytest.mark.parametrize("sr", [1, 0])
def test_roi_align_gather_backward_over_the_fp16_exponent_range(ops, sr):
    """vlb_roi_align_nhwc_bwd_gather with dout = N(0, 1) x 2^-18 (every element an fp16 subnormal), x 1 and x 2^10 in three separate
    calls, dout and act rounded to fp16, against the float64 scatter reference of test_roi_align_nhwc on the same rounded inputs.
    C / 4 = 2 < 64: the idle lanes of the wave shadow the last channel chunk.  Bars: dx_f32 1e-4 + 1e-4 max|ref|, the 16-bit dx with
    the ReLU mask 1e-4 + bar16(4e-3) max|ref|.  Each call is reported on its own; the 2^-18 call is reported a second time in units
    of its scale (a division by a power of two is exact), because max|ref| ~ 1e-5 lies under the absolute term of the bar there: the
    fp32 output at the same bar, the 16-bit output with 2^-25 / scale added for the rounding of an fp16-subnormal result."""
    N, R, C, H, W, ph = 1, 3, 8, 6, 8, 7
    X, Y = 16.0 * W - 1, 16.0 * H - 1
    boxes = torch.tensor([[[10.0, 12.0, 0.7 * X, 0.8 * Y, 9.0], [-6.0, -4.0, X, Y, 9.0], [-2.0, -2.0, -2.0, -2.0, 9.0]]])
    mask = boxes[:, :, 0] > -1.5
    rois = torch.cat((mask.nonzero()[:, :1].float(), boxes[mask][:, :4]), 1).numpy()
    bx = boxes.view(N * R, 5).contiguous().to(dev())
    g = torch.Generator().manual_seed(77 + sr)
    base = torch.randn(N * R, C, ph, ph, generator=g)
    act = h16(torch.randn(N * H * W, C, generator=g))
    ws = ops.roi_align_gather_workspace(N * R, H, W, ph, dev())
    failed = []
    for e in (-18, 0, 10):
        scale = 2.0 ** e
        dout = h16(base * scale)
        if e == -18:
            assert float(dout.abs().max()) < 2.0 ** -14 and float(dout.abs().max()) > 0.0       # all fp16-subnormal
        ref = torch.from_numpy(RA.roi_align_backward(dout[mask.view(-1)].double().numpy(), rois, 1.0 / 16, ph, ph, N, C, H, W, sr))
        ref = ref.permute(0, 2, 3, 1).reshape(-1, C).double()
        ref16 = ref * (act > 0)
        g32 = torch.full((N * H * W, C), 7.0, device=dev())
        g16 = torch.full((N * H * W, C), 7.0, dtype=torch.float16, device=dev())
        ops.roi_align_nhwc_bwd_gather(dout.permute(0, 2, 3, 1).reshape(-1, C).to(torch.float16).to(dev()), bx, R, ws, N, H, W, C,
                                      act=act.to(torch.float16).to(dev()), dx_bf16=g16, dx_f32=g32, pooled=ph, spatial_scale=1.0 / 16,
                                      sampling_ratio=sr)
        torch.cuda.synchronize()
        tag = "f16 roi_align bwd gather sr%d dout x 2^%d " % (sr, e)
        checks = [(tag + "dx_f32", g32, ref, 1e-4, 1e-4), (tag + "dx 16-bit + relu mask", g16, ref16, 1e-4, bar16(4e-3))]
        if e < 0:
            checks += [(tag + "dx_f32 / scale", g32.cpu().double() / scale, ref / scale, 1e-4, 1e-4),
                       (tag + "dx 16-bit + relu mask / scale", g16.cpu().double() / scale, ref16 / scale, 1e-4 + 2.0 ** -25 / scale,
                        bar16(4e-3))]
        for c in checks:                                   # every call and output reports, then the test fails on any of them
            try:
                report(*c)
            except AssertionError as ex:
                failed.append(str(ex))
    assert not failed, "\n".join(failed)


def _subnormal_operands(rows_a, rows_b, K, seed):
    """A [rows_a, K] ~ N(0, 1) x 2^-17 (fp16-subnormal after rounding), B [rows_b, K] ~ N(0, 1) x 2^8; both fp16-rounded."""
    g = torch.Generator().manual_seed(seed)
    A = h16(torch.randn(rows_a, K, generator=g) * 2.0 ** -17)
    B = h16(torch.randn(rows_b, K, generator=g) * 2.0 ** 8)
    assert float(A.abs().max()) < 2.0 ** -14 and float((A != 0).float().mean()) > 0.9
    return A, B


def _flush(t):
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def _two_behaviours(name, got, full, flushed):
    """Exactly two behaviours pass: the float64 product of the rounded inputs, or that product after flushing subnormal inputs to
    zero, each to 1e-4 max|full product|."""
    bar = 1e-4 * float(full.abs().max())
    got = got.detach().double().cpu()
    e_full, e_flush = float((got - full).abs().max()), float((got - flushed).abs().max())
    held = "subnormal inputs kept" if e_full <= bar else ("subnormal inputs flushed to zero" if e_flush <= bar else "NEITHER")
    print("%s: max err vs full product %.3e, vs flushed-input product %.3e, bar %.3e -> %s" % (name, e_full, e_flush, bar, held))
    report(name + " (" + held + ")", got, full if e_full <= bar else flushed, bar, 0.0)
    assert held != "NEITHER"
    return held


def test_fp16_subnormal_gemm_operands(ops):
    """vlb_gemm_nt_bf16 at 128 x 128 x 64 with fp32 output and vlb_wgrad_tn_bf16 at (R, Mo, No) = (64, 128, 128) on the fp16 build, one
    operand entirely fp16-subnormal (~2^-17), the other ~2^8."""
    M, N, K = 128, 128, 64
    A, B = _subnormal_operands(M, N, K, 5)
    C = torch.full((M, N), 7.0, device=dev())
    ops.gemm_nt(A.to(torch.float16).to(dev()), B.to(torch.float16).to(dev()), C, out_mode=ops.OUT_F32)
    torch.cuda.synchronize()
    h1 = _two_behaviours("f16 subnormal-A gemm_nt 128x128x64 fp32 out", C, A.double() @ B.double().t(), _flush(A).double() @ B.double().t())
    R, Mo, No = 64, 128, 128
    dY, X = _subnormal_operands(R, R, Mo, 6)          # [R, Mo] subnormal, [R, No] ~2^8 (Mo == No)
    Cw = torch.full((Mo, No), 7.0, device=dev())
    ws = torch.empty(max(ops.wgrad_workspace_floats(Mo, No, R), 4), dtype=torch.float32, device=dev())
    ops.wgrad_tn(dY.to(torch.float16).to(dev()), X.to(torch.float16).to(dev()), Cw, workspace=ws, accumulate=False)
    torch.cuda.synchronize()
    h2 = _two_behaviours("f16 subnormal-dY wgrad_tn 64x128x128", Cw, dY.double().t() @ X.double(), _flush(dY).double().t() @ X.double())
    print("fp16 MFMA on subnormal operands: gemm_nt %s, wgrad_tn %s" % (h1, h2))
