"""Per-kernel parity tests (-m gpu): every HIP kernel, called through the C ABI, against a plain
PyTorch fp32 CPU statement of the same op on the same (bf16-rounded) inputs.

Tolerances: outputs are bf16 (8-bit mantissa, 2^-8 relative per rounding) with fp32 accumulation,
so the bar is  max|got-ref| <= atol + rtol*max|ref|  with rtol 1e-2 (north_star's bf16 bound);
fp32 outputs (weight gradients, optimizer) use 2e-3 / 1e-5.

Both builds: every 16-bit buffer is of act_dtype(), and tests/test_f16_kernels_gpu.py runs this file again on the IEEE fp16 build in a
child process.  There the relative bar of a 16-bit output is gpu_util.bar16(bar) = 0.2 x the bf16 bar (1e-2 -> 2e-3: the unit roundoffs
are 2^-9 and 2^-12); fp32 outputs and the attention bars are the same on both builds.  No test of this file needed a bar looser than
bar16 on the fp16 build (MI355X: the worst output of the file reaches 0.26 of its bar there, the 16-bit parameter copy of AdamW).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import act_dtype, bar16, bf, dev, drop_scale, drop_thr, keep_mask, pkg, report, to_gpu_bf16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    o = pkg("ops")
    name, cus = pkg("_lib").device_info(0)
    print("device:", name, cus, "CUs")
    assert name.startswith("gfx950"), "these kernels are built for gfx950 only (got %s)" % name
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return bf(torch.randn(*shape, generator=g) * scale)


# ------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 256, 128), (300, 200, 192), (3232, 768, 768), (101, 2304, 768),
                                   (64, 1601, 128), (515, 64, 256)])
def test_gemm_plain_bias(ops, M, N, K):
    A, B = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3))
    ldc = (N + 63) // 64 * 64
    C = torch.zeros((M, ldc), dtype=act_dtype(), device=dev())
    ops.gemm_nt(to_gpu_bf16(A), to_gpu_bf16(B), C[:, :N], bias=bias.to(dev()))
    ref = A @ B.t() + bias
    report("gemm %dx%dx%d bias" % (M, N, K), C[:, :N], ref, 1e-3, bar16(1e-2))
    if ldc > N:
        assert float(C[:, N:].float().abs().max()) == 0.0, "pad columns were written"


def test_gemm_splitk_bf16_and_batched_transpose(ops):
    # few output tiles, very long K: slab split-K with the bf16-converting reduce
    M, N, K = 200, 136, 64 * 150
    A, B = rnd(M, K, seed=31, scale=0.5), rnd(N, K, seed=32, scale=0.05)
    C = torch.zeros((M, 192), dtype=act_dtype(), device=dev())[:, :N]
    ws = torch.empty(max(ops.wgrad_workspace_floats(M, N, K), 4), device=dev())
    assert ws.numel() > 4, "cost model should split this shape"
    ops.gemm_nt_splitk(to_gpu_bf16(A), to_gpu_bf16(B), C, workspace=ws)
    report("gemm splitk bf16", C, A @ B.t(), 1e-3, bar16(1e-2))
    C2 = torch.zeros_like(C)
    ops.gemm_nt_splitk(to_gpu_bf16(A), to_gpu_bf16(B), C2, workspace=None)        # single pass fallback
    report("gemm splitk bf16 (no workspace)", C2, A @ B.t(), 1e-3, bar16(1e-2))
    # batched transposes: ragged shapes, padded destinations
    g = torch.Generator().manual_seed(33)
    pairs, refs = [], []
    for R, C_ in ((70, 130), (64, 64), (300, 72), (5, 8)):
        src = torch.randn((R, C_), generator=g).to(act_dtype()).to(dev())
        dst = torch.zeros((C_, (R + 63) // 64 * 64), dtype=act_dtype(), device=dev())
        pairs.append((src, dst))
        refs.append(src.float().cpu().t())
    tb = ops.TransposeBatch(pairs, dev())
    tb.run()
    for (src, dst), ref in zip(pairs, refs):
        R = src.shape[0]
        assert torch.equal(dst[:, :R].float().cpu(), ref)
        assert float(dst[:, R:].float().abs().max() if dst.shape[1] > R else 0.0) == 0.0


def test_gemm_256_tile_kernel_large_b_operand(ops):
    """Plain / bias GEMM whose B operand exceeds the L2s and that has >= 512 tiles of 256x256: served by the 3-stage
    256x256 kernel (interior tiles staged through LDS, ragged last tile row / column, non-multiple-of-64 N)."""
    M, N, K = 4096 + 40, 8197, 1536
    g = torch.Generator().manual_seed(41)
    A = (torch.rand((M, K), generator=g) * 2 - 1).to(act_dtype())
    B = ((torch.rand((N, K), generator=g) * 2 - 1) * 0.05).to(act_dtype())
    bias = 0.2 * torch.randn(N, generator=g)
    ldc = (N + 63) // 64 * 64
    C = torch.zeros((M, ldc), dtype=act_dtype(), device=dev())
    ops.gemm_nt(A.to(dev()), B.to(dev()), C[:, :N], bias=bias.to(dev()))
    ref = A.float() @ B.float().t() + bias
    report("gemm 256-tile kernel %dx%dx%d bias" % (M, N, K), C[:, :N], ref, 1e-3, bar16(1e-2))
    assert float(C[:, N:].float().abs().max()) == 0.0, "pad columns were written"


def test_gemm_epilogues(ops):
    M, N, K = 384, 320, 256
    A, B = rnd(M, K, seed=4), rnd(N, K, seed=5, scale=0.08)
    bias = 0.3 * torch.randn(N, generator=torch.Generator().manual_seed(6))
    res, aux = rnd(M, N, seed=7), rnd(M, N, seed=8)
    Ag, Bg, bg = to_gpu_bf16(A), to_gpu_bf16(B), bias.to(dev())
    acc = A @ B.t()
    # gelu + pre-activation
    C = torch.empty((M, N), dtype=act_dtype(), device=dev())
    pre = torch.empty_like(C)
    ops.gemm_nt(Ag, Bg, C, bias=bg, act=ops.ACT_GELU, pre=pre)
    u = acc + bias
    report("gemm gelu pre", pre, u, 1e-3, bar16(1e-2))
    report("gemm gelu out", C, u * 0.5 * (1 + torch.erf(u / math.sqrt(2))), 1e-3, bar16(1e-2))
    # relu
    ops.gemm_nt(Ag, Bg, C, bias=bg, act=ops.ACT_RELU)
    report("gemm relu", C, torch.relu(u), 1e-3, bar16(1e-2))
    # dgelu: acc * gelu'(aux)
    ops.gemm_nt(Ag, Bg, C, act=ops.ACT_DGELU, aux=to_gpu_bf16(aux))
    cdf = 0.5 * (1 + torch.erf(aux / math.sqrt(2)))
    pdf = torch.exp(-0.5 * aux * aux) / math.sqrt(2 * math.pi)
    report("gemm dgelu", C, acc * (cdf + aux * pdf), 1e-3, bar16(1e-2))
    # gelu with the derivative saved for backward (act 4) and the plain-multiply backward epilogue (act 5)
    ops.gemm_nt(Ag, Bg, C, bias=bg, act=ops.ACT_GELU_D, pre=pre)
    cdf_u = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
    report("gemm gelu_d out", C, u * cdf_u, 1e-3, bar16(1e-2))
    report("gemm gelu_d deriv", pre, cdf_u + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi), 1e-3, bar16(1e-2))
    ops.gemm_nt(Ag, Bg, C, act=ops.ACT_MULAUX, aux=to_gpu_bf16(aux))
    report("gemm mulaux", C, acc * bf(aux), 1e-3, bar16(1e-2))
    out = torch.empty_like(C)
    ops.mul_bf16(to_gpu_bf16(res), to_gpu_bf16(aux), out)
    report("mul_bf16", out, bf(res) * bf(aux), 1e-3, bar16(1e-2))
    # bias + residual
    ops.gemm_nt(Ag, Bg, C, bias=bg, res=to_gpu_bf16(res))
    report("gemm bias+res", C, u + res, 1e-3, bar16(1e-2))
    # fp32 store
    C32 = torch.empty((M, N), dtype=torch.float32, device=dev())
    ops.gemm_nt(Ag, Bg, C32, out_mode=ops.OUT_F32)
    report("gemm fp32 store", C32, acc, 1e-4, 1e-5)
    # split-K atomic accumulate on top of existing contents
    base = torch.randn(M, N, generator=torch.Generator().manual_seed(9))
    for sk in (0, 1, 3, 4):
        C32 = base.clone().to(dev())
        ops.gemm_nt(Ag, Bg, C32, out_mode=ops.OUT_F32_ATOMIC, splitk=sk)
        report("gemm atomic splitk=%d" % sk, C32, base + acc, 1e-4, 2e-5)


# the run-time names of the option table (csrc/options.h) with their defaults
OPTION_DEFAULTS = {"p8_mode": 1, "p8_keepb": 1, "p8_group": 2, "p8_min_tiles": 160, "p8_wgs": 256, "p8_ablate": 0, "p8_tile192": 1,
                   "p8_drain": 0, "p8_lastw": 0, "nt_ring": 1, "nt_stagger": 0, "tn8_mode": 1, "tn8_wgs": 256, "tn8_ablate": 0,
                   "ln_fwd_rows": 0, "ln_bwd4": 1}


def test_gemm_set_option_names():
    """vlb_gemm_set_option takes every name of the table, rejects unknown names and negative values; only set calls, defaults last."""
    lib = pkg("_lib")
    try:
        with pytest.raises(RuntimeError, match="unknown option"):
            lib.gemm_set_option("no_such_option", 1)
        with pytest.raises(RuntimeError, match="negative value"):
            lib.gemm_set_option("p8_mode", -1)
        for retired in ("tn8_m32", "tn8_uneven", "tn_waves8", "attn_bwd2"):      # variants that lost their measurements
            with pytest.raises(RuntimeError, match="unknown option"):
                lib.gemm_set_option(retired, 0)
    finally:
        for name, value in OPTION_DEFAULTS.items():
            lib.gemm_set_option(name, value)


@pytest.fixture
def force_p8():
    """Route every eligible bf16 GEMM through the large-tile 8-phase core (gemm_p8.hip) whatever its tile count."""
    lib = pkg("_lib")
    lib.gemm_set_option("p8_min_tiles", 1)
    yield lib
    lib.gemm_set_option("p8_min_tiles", 160)
    lib.gemm_set_option("p8_mode", 1)
    lib.gemm_set_option("p8_wgs", 256)
    lib.gemm_set_option("p8_keepb", 1)


# wgs = persistent workgroups per launch.  256 (one per CU, the default): these shapes have <= 36 tiles, so every workgroup owns ONE
# tile and drains it through the "last tile" path (shared slab over the idle operand ring).  8: every workgroup owns SEVERAL tiles and
# drains all but its last one MID-STREAM, beside the live operand ring -- `p8_drain_w<FMH, EPI, EDGE>` (wave-private, round 3), the path
# ~10 of the 15.9 GEMM ms of the headline bench spend their epilogues in (M = 25856: 303-1212 tiles on 256 workgroups), interior and
# edge tiles; tile "4k0" = the 256-row tile without the kept B fragments (KEEPB = false instantiations).
@pytest.mark.parametrize("wgs", [256, 8], ids=["one-tile-per-wg", "mid-stream-drain"])
@pytest.mark.parametrize("tile", [3, 4, "4k0", 5])
@pytest.mark.parametrize("M,N,K", [(2048, 1024, 256), (1000, 520, 128), (2600, 768, 768), (700, 2306, 384)])
def test_gemm_large_tile_core_epilogues(ops, force_p8, tile, M, N, K, wgs):
    """vl-bert_amd/csrc/gemm_p8.hip (192-, 256- and 320-row tiles, 8-phase schedule, fp32-staged epilogue): every fused epilogue of the
    training step against the fp32 statement of the same op, interior and edge tiles (M, N not multiples of the tile, N % 8 != 0),
    the shortest K the pipeline accepts (two K tiles), several output tiles per workgroup; dropout against the numpy restatement of
    the counter RNG.  Padding columns of C must stay untouched.  (The 192-row tile is what the launcher picks for the N = 3072
    GEMMs of a 32-sample per-GPU batch -- the 8-GPU strong-scaling regime.)"""
    if tile == "4k0":
        if wgs == 256 and (M, N, K) != (2600, 768, 768):
            pytest.skip("KEEPB = false: the mid-stream cases + one single-tile shape")
        force_p8.gemm_set_option("p8_keepb", 0)
        tile = 4
    force_p8.gemm_set_option("p8_mode", tile)
    force_p8.gemm_set_option("p8_wgs", wgs)
    _epilogue_battery(ops, "p8/%d%s %dx%dx%d " % (64 * tile, " wgs8" if wgs == 8 else "", M, N, K), M, N, K, vision=True)


@pytest.mark.parametrize("ring", [2, 3], ids=["ring-128x128", "ring-128x64"])
@pytest.mark.parametrize("M,N,K", [(3232, 768, 768), (1000, 520, 512), (1300, 776, 3072)])
def test_gemm_ring_kernel_epilogues(ops, force_p8, ring, M, N, K):
    """`gemm_nt_ring_kernel` (gemm.hip: the 128x128 / 128x64 tiles behind a 4- / 3-stage operand ring with counted waits) -- the
    kernel the launcher picks for the N = 768 GEMMs at M = 1024..8192 (per-GPU batches 32-64 of a 4-8-GPU strong-scaling run).
    Every fused epilogue instantiation (EPI 0 bias, 1 GELU + GELU', 2 x aux, 3 dropout + residual, 4 bias + residual, 5 ReLU) against
    the fp32 statement; the generic instantiation (EPI -1: LayerNorm-residual / fp16 output) is covered by
    test_gemm_layernorm_residual_fp16_stream[ring-*]."""
    force_p8.gemm_set_option("p8_mode", 0)
    force_p8.gemm_set_option("nt_ring", ring)
    try:
        _epilogue_battery(ops, "ring/%s %dx%dx%d " % ("128x128" if ring == 2 else "128x64", M, N, K), M, N, K)
    finally:
        force_p8.gemm_set_option("nt_ring", 1)


def _epilogue_battery(ops, tag, M, N, K, vision=False):
    A, B = rnd(M, K, seed=4), rnd(N, K, seed=5, scale=0.08)
    bias = 0.3 * torch.randn(N, generator=torch.Generator().manual_seed(6))
    res, aux = rnd(M, N, seed=7), rnd(M, N, seed=8)
    Ag, Bg, bg = to_gpu_bf16(A), to_gpu_bf16(B), bias.to(dev())
    ldc = (N + 63) // 64 * 64
    pad = lambda t: torch.cat((t, torch.zeros(M, ldc - N)), 1).to(act_dtype()).to(dev())[:, :N]
    resg, auxg = pad(res), pad(aux)
    acc = A @ B.t()
    u = acc + bias
    Cf = torch.full((M, ldc), 3.0, dtype=act_dtype(), device=dev())
    C = Cf[:, :N]
    pre = torch.full((M, ldc), 3.0, dtype=act_dtype(), device=dev())[:, :N]
    ops.gemm_nt(Ag, Bg, C, bias=bg)
    report(tag + "bias", C, u, 1e-3, bar16(1e-2))
    assert bool((Cf[:, N:] == 3.0).all())
    ops.gemm_nt(Ag, Bg, C)
    report(tag + "plain", C, acc, 1e-3, bar16(1e-2))
    ops.gemm_nt(Ag, Bg, C, bias=bg, act=ops.ACT_GELU_D, pre=pre)
    cdf_u = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
    report(tag + "gelu_d out", C, u * cdf_u, 1e-3, bar16(1e-2))
    report(tag + "gelu_d deriv", pre, cdf_u + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi), 1e-3, bar16(1e-2))
    ops.gemm_nt(Ag, Bg, C, act=ops.ACT_MULAUX, aux=auxg)
    report(tag + "mulaux", C, acc * aux, 1e-3, bar16(1e-2))
    ops.gemm_nt(Ag, Bg, C, bias=bg, res=resg)
    report(tag + "bias+res", C, u + res, 1e-3, bar16(1e-2))
    ops.gemm_nt(Ag, Bg, C, bias=bg, act=ops.ACT_RELU)
    report(tag + "relu", C, torch.relu(u), 1e-3, bar16(1e-2))
    # in-place residual (C aliases res): the epilogue reads and writes the same 16-B group from one thread
    Cr = resg.clone()
    Crf = torch.zeros((M, ldc), dtype=act_dtype(), device=dev())
    Crf[:, :N] = Cr
    ops.gemm_nt(Ag, Bg, Crf[:, :N], bias=bg, res=Crf[:, :N])
    report(tag + "in-place residual", Crf[:, :N], u + res, 1e-3, bar16(1e-2))
    # dropout + residual against the numpy RNG
    p, seed_v, tg = 0.1, 4242, 9
    seed = torch.tensor([seed_v], dtype=torch.int32, device=dev())
    ops.gemm_nt(Ag, Bg, C, bias=bg, res=resg, drop_p=p, seed=seed, tag=tg)
    thr = drop_thr(p)
    idx = (np.arange(M, dtype=np.int64)[:, None] * N + np.arange(N, dtype=np.int64)[None, :])
    keep = torch.from_numpy(keep_mask(seed_v, tg, idx.reshape(-1), thr).reshape(M, N))
    report(tag + "dropout+res", C, torch.where(keep, u * drop_scale(thr), torch.zeros_like(u)) + res, 1e-3, bar16(1e-2))
    assert bool((Cf[:, N:] == 3.0).all())
    if vision:      # the two epilogues of the e2e trunk that run on this core (EPI 8 / 10): Bottleneck tail, ReLU backward in a dgrad
        ops.gemm_nt(Ag, Bg, C, bias=bg, res=resg, act=ops.ACT_RES_RELU)
        report(tag + "relu(bias+res)", C, torch.relu(u + res), 1e-3, bar16(1e-2))
        ops.gemm_nt(Ag, Bg, C, act=ops.ACT_RELU_MASK, aux=auxg)
        report(tag + "acc where aux>0", C, acc * (aux > 0), 1e-3, bar16(1e-2))
        assert bool((Cf[:, N:] == 3.0).all())


@pytest.mark.parametrize("core", ["128x128", "p8-192", "p8-256", "p8-320", "p8-192-midstream", "p8-256-midstream", "p8-320-midstream",
                                  "ring-128x128", "ring-128x64"])
def test_gemm_layernorm_residual_fp16_stream(ops, force_p8, core):
    """vlb_gemm_nt_bf16_ex: residual = LayerNorm output re-materialised in fp32 from fp16 pre-LN rows + (mean, rstd) + gamma / beta,
    result stored as fp16 (the encoder's residual stream, BertSelfOutput / BertOutput); with and without dropout; and the LayerNorm
    kernels reading fp16 rows.  Reference: fp32 torch on the same (fp16 / bf16 rounded) inputs."""
    lib = force_p8
    if core.endswith("-midstream"):      # several tiles per workgroup: EPI 6 / 7 through the mid-stream drain (see the epilogue test)
        core = core[:-len("-midstream")]
        lib.gemm_set_option("p8_wgs", 8)
    lib.gemm_set_option("p8_mode", {"128x128": 0, "p8-192": 3, "p8-256": 4, "p8-320": 5}.get(core, 0))
    lib.gemm_set_option("nt_ring", {"ring-128x128": 2, "ring-128x64": 3}.get(core, 0))
    try:
        _ln_residual_checks(ops, core)
    finally:
        lib.gemm_set_option("nt_ring", 1)


def _ln_residual_checks(ops, core):
    M, N, K = 1300, 776, 256
    A, B = rnd(M, K, seed=14), rnd(N, K, seed=15, scale=0.08)
    bias = 0.3 * torch.randn(N, generator=torch.Generator().manual_seed(16))
    gam = 1.0 + 0.2 * torch.randn(N, generator=torch.Generator().manual_seed(17))
    bet = 0.1 * torch.randn(N, generator=torch.Generator().manual_seed(18))
    zprev = (torch.randn(M, N, generator=torch.Generator().manual_seed(19)) * 2.0 + 0.3).half().float()
    mean = zprev.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(zprev.var(1, unbiased=False, keepdim=True) + 1e-12)
    ln_out = (zprev - mean) * rstd * gam + bet
    u = A @ B.t() + bias
    ldc = (N + 63) // 64 * 64
    zg = torch.zeros((M, ldc), dtype=torch.float16, device=dev())[:, :N]
    zg.copy_(zprev.to(dev()))
    st = torch.cat((mean, rstd), 1).contiguous().to(dev())
    Cf = torch.full((M, ldc), 3.0, dtype=torch.float16, device=dev())
    C = Cf[:, :N]
    Ag, Bg = to_gpu_bf16(A), to_gpu_bf16(B)
    ops.gemm_nt(Ag, Bg, C, bias=bias.to(dev()), res=zg, res_ln=(st, gam.to(dev()), bet.to(dev())))
    ref = u + ln_out
    report("gemm LN-residual -> fp16 (%s)" % core, C, ref, 2e-3, 2e-3)          # fp16 output: 2^-11 relative
    assert bool((Cf[:, N:] == 3.0).all())
    p, seed_v, tg = 0.1, 777, 5
    seed = torch.tensor([seed_v], dtype=torch.int32, device=dev())
    ops.gemm_nt(Ag, Bg, C, bias=bias.to(dev()), res=zg, res_ln=(st, gam.to(dev()), bet.to(dev())), drop_p=p, seed=seed, tag=tg)
    thr = drop_thr(p)
    idx = (np.arange(M, dtype=np.int64)[:, None] * N + np.arange(N, dtype=np.int64)[None, :])
    keep = torch.from_numpy(keep_mask(seed_v, tg, idx.reshape(-1), thr).reshape(M, N))
    report("gemm dropout + LN-residual -> fp16 (%s)" % core, C, torch.where(keep, u * drop_scale(thr), torch.zeros_like(u)) + ln_out, 2e-3, 2e-3)
    # plain bf16 residual, fp16 output (encoder layer 0)
    resb = rnd(M, N, seed=20)
    rg = torch.zeros((M, ldc), dtype=act_dtype(), device=dev())[:, :N]
    rg.copy_(resb.to(dev()))
    ops.gemm_nt(Ag, Bg, C, bias=bias.to(dev()), res=rg)
    report("gemm bf16 residual -> fp16 (%s)" % core, C, u + resb, 2e-3, 2e-3)
    # LayerNorm forward / backward on fp16 rows
    H = 768
    rows = 257
    x = (torch.randn(rows, H, generator=torch.Generator().manual_seed(21)) * 1.7 - 0.2).half().float()
    g2 = 1.0 + 0.1 * torch.randn(H, generator=torch.Generator().manual_seed(22))
    b2 = 0.1 * torch.randn(H, generator=torch.Generator().manual_seed(23))
    dy = rnd(rows, H, seed=24)
    xr = x.clone().requires_grad_(True)
    mu = xr.mean(1, keepdim=True)
    yref = (xr - mu) / torch.sqrt(((xr - mu) ** 2).mean(1, keepdim=True) + 1e-12) * g2 + b2
    yref.backward(dy)
    y = torch.empty((rows, H), dtype=act_dtype(), device=dev())
    stats = torch.empty((rows, 2), dtype=torch.float32, device=dev())
    xg = x.half().to(dev())
    ops.layernorm_fwd(xg, g2.to(dev()), b2.to(dev()), y, stats)
    report("layernorm fwd on fp16 rows", y, yref.detach(), 1e-3, bar16(1e-2))
    dx = torch.empty((rows, H), dtype=act_dtype(), device=dev())
    dg, db = torch.zeros(H, device=dev()), torch.zeros(H, device=dev())
    ops.layernorm_bwd(to_gpu_bf16(dy), xg, stats, g2.to(dev()), dx=dx, dgamma=dg, dbeta=db)
    report("layernorm bwd dx on fp16 rows", dx, xr.grad, 1e-3, bar16(1e-2))
    report("layernorm bwd dgamma on fp16 rows", dg, (dy * ((x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-12))).sum(0), 1e-3, 2e-3)


HEADLINE_GEMMS = [      # (name, N, K, epilogue) of one encoder layer at the headline batch: M = 256 x 101 = 25856 rows
    ("qkv fwd", 2304, 768, "bias"), ("attn-out fwd", 768, 768, "drop_lnres"), ("ffn1 fwd", 3072, 768, "gelu_d"),
    ("ffn2 fwd", 768, 3072, "drop_lnres"), ("attn-out dgrad", 768, 768, "plain"), ("qkv dgrad", 768, 2304, "res"),
    ("ffn1 dgrad", 768, 3072, "res"), ("ffn2 dgrad", 3072, 768, "mulaux")]


@pytest.mark.parametrize("name,N,K,epi", HEADLINE_GEMMS, ids=[g[0].replace(" ", "-") for g in HEADLINE_GEMMS])
def test_gemm_headline_shapes_with_the_launchers_own_selection(ops, name, N, K, epi):
    """The eight NT GEMMs of an encoder layer EXACTLY as bench.py times them -- M = 25856 rows (batch 256 x 101 positions), the library's
    default kernel selection (no option forced: 243-1212 tiles of the large-tile core, mid-stream wave-private drains, the
    last-tile slab drain, 320- / 256-row tiles as the cost model picks), the epilogue each one carries in the step -- against an fp32
    CPU statement of the same op on the same 16-bit inputs.  (tools/p8_check.py check covered these shapes as a tool only; the
    round-3 review found no suite test with more than 204 tiles and a fused epilogue.)"""
    M = 256 * 101
    g = torch.Generator().manual_seed(500 + N + K)
    A = bf((torch.rand((M, K), generator=g) * 2 - 1))
    B = bf((torch.rand((N, K), generator=g) * 2 - 1) * 0.06)
    bias = 0.3 * torch.randn(N, generator=g)
    Ag, Bg, bg = to_gpu_bf16(A), to_gpu_bf16(B), bias.to(dev())
    acc = A @ B.t()
    tag = "headline %s %dx%dx%d " % (name, M, N, K)
    C = torch.full((M, N), 3.0, dtype=act_dtype(), device=dev())
    if epi == "bias":
        ops.gemm_nt(Ag, Bg, C, bias=bg)
        report(tag + "bias", C, acc + bias, 1e-3, bar16(1e-2))
    elif epi == "plain":
        ops.gemm_nt(Ag, Bg, C)
        report(tag + "plain", C, acc, 1e-3, bar16(1e-2))
    elif epi == "gelu_d":
        pre = torch.full((M, N), 3.0, dtype=act_dtype(), device=dev())
        ops.gemm_nt(Ag, Bg, C, bias=bg, act=ops.ACT_GELU_D, pre=pre)
        u = acc + bias
        cdf = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
        report(tag + "gelu out", C, u * cdf, 1e-3, bar16(1e-2))
        report(tag + "gelu' saved", pre, cdf + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi), 1e-3, bar16(1e-2))
    elif epi == "res":
        res = bf(torch.randn((M, N), generator=g))
        ops.gemm_nt(Ag, Bg, C, bias=bg, res=to_gpu_bf16(res))
        report(tag + "bias+res", C, acc + bias + res, 1e-3, bar16(1e-2))
    elif epi == "mulaux":
        aux = bf(torch.rand((M, N), generator=g) * 1.2 - 0.1)
        ops.gemm_nt(Ag, Bg, C, act=ops.ACT_MULAUX, aux=to_gpu_bf16(aux))
        report(tag + "x aux", C, acc * aux, 1e-3, bar16(1e-2))
    else:       # dropout + LayerNorm-residual from fp16 rows, fp16 output: BertSelfOutput / BertOutput as the engine runs them
        gam = 1.0 + 0.2 * torch.randn(N, generator=g)
        bet = 0.1 * torch.randn(N, generator=g)
        z = (torch.randn((M, N), generator=g) * 2.0 + 0.3).half()
        zf = z.float()
        mean = zf.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(zf.var(1, unbiased=False, keepdim=True) + 1e-12)
        st = torch.cat((mean, rstd), 1).contiguous().to(dev())
        Ch = torch.full((M, N), 3.0, dtype=torch.float16, device=dev())
        p, seed_v, tg = 0.1, 991, 21
        seed = torch.tensor([seed_v], dtype=torch.int32, device=dev())
        ops.gemm_nt(Ag, Bg, Ch, bias=bg, res=z.to(dev()), res_ln=(st, gam.to(dev()), bet.to(dev())), drop_p=p, seed=seed, tag=tg)
        thr = drop_thr(p)
        keep = torch.from_numpy(keep_mask(seed_v, tg, np.arange(M * N, dtype=np.int64), thr).reshape(M, N))
        u = acc + bias
        report(tag + "dropout + LN-residual -> fp16", Ch, torch.where(keep, u * drop_scale(thr), torch.zeros_like(u)) +
               ((zf - mean) * rstd * gam + bet), 2e-3, 2e-3 if act_dtype() == torch.float16 else 4e-3)


def test_engine_step_through_large_tile_core(force_p8):
    """The whole VL-BERT step with EVERY eligible GEMM forced through gemm_p8.hip (one mostly-clamped 256-row tile at this size)
    against the same engine on the 128x128 kernels: logits / losses / gradients must agree to bf16 rounding."""
    from oracle import vlbert_oracle as O
    E, syn = pkg("engine"), pkg("synthetic")
    cfg = O.VLBertConfig(num_hidden_layers=2)
    params = O.init_params(cfg, seed=91)
    batch = syn.make_batch(4, 32, 10, seed=92, ragged=True)
    outs = []
    for mode in (0, 4, 5):
        force_p8.gemm_set_option("p8_mode", mode)
        mc = E.ModelConfig(num_hidden_layers=2)
        eng = E.PretrainEngine(mc, 4, 32, 10, device="cuda:0", keep_logits=True, train=False)
        eng.load_state_dict({k: v.to(dev()) for k, v in params.items()})
        eng.set_batch(*[t.to(dev()) for t in batch])
        eng.zero_grad()
        eng.forward(train=False)
        eng.backward(train=False)
        torch.cuda.synchronize()
        outs.append((eng.mlm_logits_copy.float().cpu(), eng.loss_values()["loss"], eng.grad_norm(), {k: v.cpu() for k, v in eng.grads().items()}))
    for k in (1, 2):
        report("engine via p8 (mode %d) mlm logits vs 128x128 kernels" % (4 if k == 1 else 5), outs[k][0], outs[0][0], 2e-3, 1e-2)
        assert abs(outs[k][1] - outs[0][1]) < 2e-3 * abs(outs[0][1])
        assert abs(outs[k][2] - outs[0][2]) < 5e-3 * outs[0][2]
        # (obj_downsample: a ReLU unit within bf16 rounding of 0 may flip between two kernels' roundings -- whole gradient rows change)
        worst = max((float((outs[k][3][n].double() - g.double()).norm() / max(float(g.double().norm()), 1e-12)) /
                     (4.0 if "obj_downsample" in n else 1.0), n)
                    for n, g in outs[0][3].items() if float(g.norm()) > 1e-6 * outs[0][2])
        print("engine via p8: worst per-tensor rel-fro gradient difference %.3e (%s)" % worst)
        assert worst[0] < 3e-2, worst


def test_gemm_wgrad_shape(ops):
    """dW[N,K] = dY^T[N,Mp] (X^T[K,Mp])^T through the transpose kernel, zero-padded reduction dim."""
    M, N, K = 1000, 192, 320
    Mp = (M + 63) // 64 * 64
    dY, X = rnd(M, N, seed=10), rnd(M, K, seed=11)
    dYt = torch.zeros((N, Mp), dtype=act_dtype(), device=dev())
    Xt = torch.zeros((K, Mp), dtype=act_dtype(), device=dev())
    db = torch.zeros((N,), dtype=torch.float32, device=dev())
    ops.transpose(to_gpu_bf16(dY), dYt, colsum=db)
    ops.transpose(to_gpu_bf16(X), Xt)
    report("transpose", dYt[:, :M], dY.t(), 0, 0)
    assert float(dYt[:, M:].float().abs().max()) == 0.0
    report("transpose colsum", db, dY.sum(0), 1e-3, 1e-5)
    dW = torch.zeros((N, K), dtype=torch.float32, device=dev())
    ops.gemm_nt(dYt, Xt, dW, out_mode=ops.OUT_F32_ATOMIC)
    report("wgrad via transposes", dW, dY.t() @ X, 1e-3, 2e-5)


@pytest.mark.parametrize("M,N,K,ws", [(192, 320, 1024, True), (768, 768, 8192, True), (300, 70, 640, True), (256, 256, 2048, False),
                                      (1601, 128, 1152, True)])
def test_wgrad_slab_splitk(ops, M, N, K, ws):
    """C += A B^T through fp32 slabs + reduce (no atomics); accumulates on top of existing contents."""
    A, B = rnd(M, K, seed=15), rnd(N, K, seed=16, scale=0.1)
    base = torch.randn(M, N, generator=torch.Generator().manual_seed(17))
    ldc = (N + 3) // 4 * 4
    C = torch.zeros((M, ldc), dtype=torch.float32, device=dev())
    C[:, :N] = base.to(dev())
    work = torch.empty(max(ops.wgrad_workspace_floats(M, N, K), 4), dtype=torch.float32, device=dev()) if ws else None
    print("wgrad %dx%dx%d workspace floats: %d" % (M, N, K, 0 if work is None else work.numel()))
    ops.wgrad_nt(to_gpu_bf16(A), to_gpu_bf16(B), C[:, :N], workspace=work)
    report("wgrad slab split-K %dx%dx%d ws=%s" % (M, N, K, ws), C[:, :N], base + A @ B.t(), 1e-3, 2e-5)
    if ldc > N:
        assert float(C[:, N:].abs().max()) == 0.0


# (the last four shapes -- reduction a multiple of 128 rows, enough 256x256 tiles x K slices -- run on the large-tile core, gemm_tn8.hip)
@pytest.mark.parametrize("R,Mo,No", [(1000, 192, 320), (2048, 768, 768), (300, 70, 200), (101, 1601, 128), (6464, 2304, 768),
                                     (64, 128, 128), (4096, 30522, 64), (4096, 768, 768), (2560, 1000, 520), (12928, 768, 3072)])
def test_wgrad_tn_lds_transpose_reads(ops, R, Mo, No):
    """dW += dY^T X and db += colsum(dY) straight from row-major operands (ds_read_b64_tr_b16 fragments)."""
    lda, ldb = (Mo + 63) // 64 * 64, (No + 7) // 8 * 8
    dY, X = rnd(R, Mo, seed=18), rnd(R, No, seed=19, scale=0.2)
    dYg = torch.full((R, lda), 9.0, dtype=act_dtype(), device=dev())   # pad columns hold junk on purpose
    Xg = torch.full((R, ldb), 7.0, dtype=act_dtype(), device=dev())
    dYg[:, :Mo] = to_gpu_bf16(dY)
    Xg[:, :No] = to_gpu_bf16(X)
    base = torch.randn(Mo, No, generator=torch.Generator().manual_seed(20))
    ldc = (No + 3) // 4 * 4
    C = torch.zeros((Mo, ldc), dtype=torch.float32, device=dev())
    C[:, :No] = base.to(dev())
    db = torch.ones(Mo, dtype=torch.float32, device=dev())
    Rp = (R + 63) // 64 * 64
    work = torch.empty(max(ops.wgrad_workspace_floats(Mo, No, Rp), 4), dtype=torch.float32, device=dev())
    ops.wgrad_tn(dYg[:, :Mo], Xg[:, :No], C[:, :No], colsum=db, workspace=work)
    report("wgrad TN %dx%dx%d" % (R, Mo, No), C[:, :No], base + dY.t() @ X, 1e-3, 2e-5)
    report("wgrad TN colsum", db, 1 + dY.sum(0), 1e-3, 1e-5)
    if ldc > No:
        assert float(C[:, No:].abs().max()) == 0.0
    # overwrite mode: previous contents (here: the accumulated result) are ignored, the bias sum still accumulates
    ops.wgrad_tn(dYg[:, :Mo], Xg[:, :No], C[:, :No], colsum=db, workspace=work, accumulate=False)
    report("wgrad TN overwrite %dx%dx%d" % (R, Mo, No), C[:, :No], dY.t() @ X, 1e-3, 2e-5)
    report("wgrad TN colsum (2nd)", db, 1 + 2 * dY.sum(0), 1e-3, 2e-5)
    if ldc > No:
        assert float(C[:, No:].abs().max()) == 0.0
    # ranged zero helper
    buf = torch.ones(5000, device=dev())
    zr = ops.ZeroRanges(buf, [(0, 3), (10, 10), (17, 1100), (4000, 5000)])
    zr.run()
    ref = torch.ones(5000)
    ref[0:3] = 0; ref[17:1100] = 0; ref[4000:] = 0
    assert torch.equal(buf.cpu(), ref)


@pytest.mark.parametrize("R,accumulate", [(2560, True), (1024, False), (300, True)])
def test_wgrad_tn_grouped_layer(ops, R, accumulate):
    """vlb_wgrad_tn_group_bf16: the four weight gradients of a transformer block in one launch (large-tile core, 2 K slices; R = 300
    takes the per-gradient fallback) against fp32 torch; bias column sums; accumulate and overwrite."""
    H, I = 768, 3072
    shapes = [(H, I), (I, H), (H, H), (3 * H, H)]          # (Mo, No): output.dense, intermediate.dense, attention.output, fused QKV
    items, refs = [], []
    for k, (Mo, No) in enumerate(shapes):
        dY, X = rnd(R, Mo, seed=30 + k, scale=0.5), rnd(R, No, seed=40 + k, scale=0.2)
        base = torch.randn(Mo, No, generator=torch.Generator().manual_seed(50 + k))
        C = base.clone().to(dev())
        db = torch.ones(Mo, dtype=torch.float32, device=dev())
        items.append((to_gpu_bf16(dY), to_gpu_bf16(X), C, db))
        refs.append(((base if accumulate else 0) + dY.t() @ X, 1 + dY.sum(0)))
    work = torch.empty(2 * sum(a * b for a, b in shapes) + 64, dtype=torch.float32, device=dev())
    ops.wgrad_tn_group(items, workspace=work, accumulate=accumulate)
    for k, ((_, _, C, db), (rc, rb)) in enumerate(zip(items, refs)):
        report("grouped wgrad %d (R=%d)" % (k, R), C, rc, 1e-3, 2e-5)
        report("grouped wgrad %d colsum" % k, db, rb, 1e-3, 2e-5)


@pytest.mark.parametrize("R", [25856, 12928 + 128, 6528])
def test_wgrad_tn_grouped_layer_encoder_rows(ops, R):
    """The grouped launch at the encoder's row counts (batch 256 / 128 / 64): 108 tiles x 2 equal K slices, against an fp32 torch.mm of
    the same bf16 operands."""
    H, I = 768, 3072
    shapes = [(H, I), (I, H), (H, H), (3 * H, H)]
    ins = [(to_gpu_bf16(rnd(R, Mo, seed=60 + k, scale=0.5)), to_gpu_bf16(rnd(R, No, seed=70 + k, scale=0.2))) for k, (Mo, No) in enumerate(shapes)]
    work = torch.empty(2 * sum(a * b for a, b in shapes) + 64, dtype=torch.float32, device=dev())
    items = [(dY, X, torch.full((Mo, No), 0.5, dtype=torch.float32, device=dev()), torch.ones(Mo, dtype=torch.float32, device=dev()))
             for (dY, X), (Mo, No) in zip(ins, shapes)]
    ops.wgrad_tn_group(items, workspace=work, accumulate=True)
    for k, (dY, X) in enumerate(ins):
        ref = 0.5 + dY.float().t() @ X.float()
        refb = 1 + dY.float().sum(0)
        report("grouped wgrad %d (R=%d)" % (k, R), items[k][2], ref.cpu(), 1e-3, 2e-4)
        report("grouped wgrad %d colsum" % k, items[k][3], refb.cpu(), 1e-3, 2e-4)


@pytest.mark.parametrize("R", [25856, 3328])
def test_wgrad_tn_core_variants(ops, R):
    """The large-tile weight-gradient core as the grouped launch of an encoder layer, as a ragged single product (Mo, No not multiples
    of the tile), and as the TABLE launch of two layers' products over full K (what the engine issues per layer pair): each against an
    fp32 torch.mm of the same bf16 operands."""
    H, I = 768, 3072
    shapes = [(H, I), (I, H), (H, H), (3 * H, H)]
    ins = [(to_gpu_bf16(rnd(R, Mo, seed=160 + k, scale=0.5)), to_gpu_bf16(rnd(R, No, seed=170 + k, scale=0.2))) for k, (Mo, No) in enumerate(shapes * 2)]
    rag = (to_gpu_bf16(rnd(4096, 1000, seed=180, scale=0.5)), to_gpu_bf16(rnd(4096, 520, seed=181, scale=0.2)))
    work = torch.empty(3 * sum(a * b for a, b in shapes) + 64, dtype=torch.float32, device=dev())
    mk = lambda Mo, No, c: (torch.full((Mo, No), c, dtype=torch.float32, device=dev()), torch.ones(Mo, dtype=torch.float32, device=dev()))
    items = [(dY, X) + mk(Mo, No, 0.5) for (dY, X), (Mo, No) in zip(ins[:4], shapes)]
    ops.wgrad_tn_group(items, workspace=work, accumulate=True)
    one = [(rag[0], rag[1], torch.full((1000, 520), -0.25, dtype=torch.float32, device=dev()), torch.zeros(1000, dtype=torch.float32, device=dev()))]
    ops.wgrad_tn_group(one, workspace=work, accumulate=True)
    pair = [(dY, X) + mk(Mo, No, 0.5) + (None,) for (dY, X), (Mo, No) in zip(ins, shapes * 2)]
    tab = ops.WgradTable(pair, dev(), accumulate=True)
    assert tab.ok and tab.nitems == 216
    tab.run()
    torch.cuda.synchronize()
    for k, (dY, X) in enumerate(ins[:4] + [rag]):
        base, cbase = (0.5, 1.0) if k < 4 else (-0.25, 0.0)
        ref = (base + dY.float().t() @ X.float()).cpu()
        refb = (cbase + dY.float().sum(0)).cpu()
        report("wgrad core product %d (R=%d)" % (k, R), (items + one)[k][2], ref, 1e-3, 2e-4)
        report("wgrad core colsum %d" % k, (items + one)[k][3], refb, 1e-3, 2e-4)
    for k, (dY, X) in enumerate(ins):
        ref = (0.5 + dY.float().t() @ X.float()).cpu()
        refb = (1.0 + dY.float().sum(0)).cpu()
        report("wgrad pair table product %d (R=%d)" % (k, R), pair[k][2], ref, 1e-3, 2e-4)
        report("wgrad pair table colsum %d" % k, pair[k][3], refb, 1e-3, 2e-4)


@pytest.mark.parametrize("accumulate", [True, False])
def test_wgrad_tn_table_many_products_one_launch(ops, accumulate):
    """vlb_wgrad_tn_table_*: weight gradients with DIFFERENT row counts, ragged output shapes (Mo / No below, at and beyond one
    256 x 256 tile, not multiples of 8 allowed only where the leading dimension still is), per-output-row scale (the frozen-BatchNorm
    fold of the vision path), optional column sums, accumulate / overwrite -- one launch, against fp32 torch on the same bf16 operands.
    A product whose row count is not a multiple of 128 makes the table refuse (ok = False) instead of computing garbage."""
    specs = [(19200, 256, 1024, True, False), (19200, 1024, 256, True, True), (384, 40, 264, False, True), (1280, 520, 72, True, False),
             (2560, 256, 512, False, False)]          # (R, Mo, No, rowscale?, colsum?)
    items, refs = [], []
    for k, (R, Mo, No, with_rs, with_cs) in enumerate(specs):
        g = torch.Generator().manual_seed(900 + k)
        valid = R - (48 if k < 2 else 0)                # the vision path's operands: M = 19152 rows + zero rows up to 19200
        dY = bf(torch.randn((R, Mo), generator=g) * 0.5)
        X = bf(torch.randn((R, No), generator=g) * 0.2)
        dY[valid:] = 0
        X[valid:] = 0
        base = torch.randn((Mo, No), generator=g)
        C = base.clone().to(dev())
        rs = (0.5 + torch.rand(Mo, generator=g)) if with_rs else None
        cs = torch.ones(Mo, dtype=torch.float32, device=dev()) if with_cs else None
        items.append((to_gpu_bf16(dY), to_gpu_bf16(X), C, cs, rs.to(dev()) if with_rs else None))
        prod = dY.t() @ X
        if with_rs:
            prod = prod * rs[:, None]
        refs.append(((base if accumulate else 0) + prod, (1 + dY.sum(0)) if with_cs else None))
    tab = ops.WgradTable(items, dev(), accumulate=accumulate)
    assert tab.ok and tab.n == len(specs) and tab.nitems == 4 + 4 + 2 + 3 + 2
    tab.run()
    tab.run() if accumulate is False else None          # overwrite mode is idempotent
    torch.cuda.synchronize()
    for k, ((_, _, C, cs, _), (rc, rb)) in enumerate(zip(items, refs)):
        report("table wgrad %d R=%d %dx%d" % (k, specs[k][0], specs[k][1], specs[k][2]), C, rc, 2e-3, 2e-4)
        if cs is not None:
            report("table wgrad %d colsum" % k, cs, (rb if accumulate else 1 + 2 * (rb - 1)), 1e-3, 2e-4)
    bad = ops.WgradTable([(items[2][0][:300], items[2][1][:300], items[2][2], None, None)], dev())
    assert not bad.ok
    with pytest.raises(RuntimeError):
        bad.run()


def test_gemm_dropout_and_ln_mask_agree(ops):
    """The GEMM-epilogue dropout mask and the LayerNorm-backward dx_drop mask are the same function."""
    M, N, K = 200, 256, 64
    p, tag, seedv = 0.1, 7, 12345
    seed = torch.tensor([seedv], dtype=torch.int32, device=dev())
    A = torch.ones((M, K))
    B = torch.ones((N, K)) / K
    C = torch.empty((M, N), dtype=act_dtype(), device=dev())
    ops.gemm_nt(to_gpu_bf16(A), to_gpu_bf16(B), C, drop_p=p, seed=seed, tag=tag)
    thr = drop_thr(p)
    keep = keep_mask(seedv, tag, np.arange(M * N), thr).reshape(M, N)
    ref = torch.from_numpy(keep.astype(np.float32)) * drop_scale(thr)
    report("gemm dropout mask (numpy RNG)", C, bf(ref), 1e-6, 0)
    frac = keep.mean()
    assert abs(frac - 0.9) < 0.01, frac
    # LayerNorm backward with dx_drop: zero pattern must match
    x = rnd(M, N, seed=13)
    dy = rnd(M, N, seed=14)
    stats = torch.empty((M, 2), dtype=torch.float32, device=dev())
    gamma = torch.ones(N, device=dev())
    y = torch.empty((M, N), dtype=act_dtype(), device=dev())
    ops.layernorm_fwd(to_gpu_bf16(x), gamma, torch.zeros(N, device=dev()), y, stats)
    dx = torch.empty_like(y)
    dxd = torch.empty_like(y)
    ops.layernorm_bwd(to_gpu_bf16(dy), to_gpu_bf16(x), stats, gamma, dx=dx, dx_drop=dxd, drop_p=p, seed=seed, tag=tag)
    report("ln bwd dx_drop == dx*mask", dxd, bf(dx.float().cpu() * ref), 2e-2, bar16(1e-2))


# ------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("rows,H", [(7, 128), (333, 768), (64, 1024), (5, 64), (7001, 768)])
def test_layernorm_fwd_bwd(ops, rows, H):
    x = bf(rnd(rows, H, seed=20, scale=2.0) + 0.5)
    g = torch.Generator().manual_seed(21)
    gamma = 1 + 0.2 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    dy = rnd(rows, H, seed=22)
    xr = x.clone().requires_grad_(True)
    gr = gamma.clone().requires_grad_(True)
    br = beta.clone().requires_grad_(True)
    u = xr.mean(-1, keepdim=True)
    s = (xr - u).pow(2).mean(-1, keepdim=True)
    yr = gr * ((xr - u) / torch.sqrt(s + 1e-12)) + br
    yr.backward(dy)
    y = torch.empty((rows, H), dtype=act_dtype(), device=dev())
    stats = torch.empty((rows, 2), dtype=torch.float32, device=dev())
    ops.layernorm_fwd(to_gpu_bf16(x), gamma.to(dev()), beta.to(dev()), y, stats)
    report("ln fwd %dx%d" % (rows, H), y, yr, 1e-3, bar16(1e-2))
    dx = torch.empty_like(y)
    dg = torch.zeros(H, device=dev())
    db = torch.zeros(H, device=dev())
    acc = torch.zeros((rows, H), device=dev())
    ops.layernorm_bwd(to_gpu_bf16(dy), to_gpu_bf16(x), stats, gamma.to(dev()), dx=dx, dx_acc=acc, dgamma=dg, dbeta=db)
    # workspace path for the parameter gradients (per-workgroup partial vectors + column-sum kernel; accumulates on top)
    ws = torch.full((ops.ln_bwd_workspace_floats(H),), 7.0, device=dev())
    dg2, db2 = dg.clone(), db.clone()
    ops.layernorm_bwd(to_gpu_bf16(dy), to_gpu_bf16(x), stats, gamma.to(dev()), dgamma=dg2, dbeta=db2, workspace=ws)
    report("ln bwd dgamma via workspace", dg2, 2 * dg.cpu(), 2e-3, 2e-3)
    report("ln bwd dbeta via workspace", db2, 2 * db.cpu(), 2e-3, 2e-3)
    report("ln bwd dx", dx, xr.grad, 1e-3, bar16(1e-2))
    report("ln bwd dx_acc(fp32)", acc, xr.grad, 1e-4, 1e-4)
    report("ln bwd dgamma", dg, gr.grad, 1e-3, 1e-4)
    report("ln bwd dbeta", db, br.grad, 1e-3, 1e-4)
    # fp32 dy path
    acc.zero_()
    ops.layernorm_bwd(dy.to(dev()), to_gpu_bf16(x), stats, gamma.to(dev()), dx_acc=acc)
    report("ln bwd (fp32 dy) dx_acc", acc, xr.grad, 1e-4, 1e-4)


# ------------------------------------------------------------------------------------ attention
def attn_ref(qkv, mask, B, S, H, nh, keep=None, scale_drop=1.0):
    d = H // nh
    q, k, v = [t.view(B, S, nh, d).permute(0, 2, 1, 3) for t in qkv.view(B, S, 3, H).unbind(2)]
    sc = q @ k.transpose(-1, -2) / math.sqrt(d) + ((1 - mask) * -10000.0)[:, None, None, :]
    p = torch.softmax(sc, -1)
    lse = torch.logsumexp(sc, -1)
    if keep is not None:
        p = p * keep * scale_drop
    ctx = (p @ v).permute(0, 2, 1, 3).reshape(B * S, H)
    return ctx, lse


@pytest.mark.parametrize("B,S,nh,p", [(2, 101, 2, 0.0), (3, 43, 1, 0.0), (1, 128, 3, 0.0), (2, 20, 2, 0.0), (2, 101, 2, 0.1),
                                      (1, 65, 1, 0.25),
                                      # S > 128: the 8-key-block / two-slices-per-wave instantiation (large + VCR configurations)
                                      (2, 229, 2, 0.0), (1, 256, 1, 0.0), (2, 129, 1, 0.0), (2, 200, 2, 0.1),
                                      # the step's head counts (head stride, B*nh workgroups) and S below one 32-key block / one wave
                                      (8, 101, 12, 0.0), (3, 101, 16, 0.0), (2, 1, 2, 0.0), (2, 17, 2, 0.0), (2, 33, 2, 0.1)])
def test_attention_fwd_bwd(ops, B, S, nh, p):
    H = nh * 64
    qkv = rnd(B * S, 3 * H, seed=30, scale=1.0)
    g = torch.Generator().manual_seed(31)
    lens = torch.randint(max(1, S // 2), S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).float()
    dctx = rnd(B * S, H, seed=32)
    tag, seedv = 3, 777
    keep = None
    thr = drop_thr(p)
    if p > 0:
        idx = np.arange(B * nh * S * S)
        keep = torch.from_numpy(keep_mask(seedv, tag, idx, thr).reshape(B, nh, S, S).astype(np.float32))
    qr = qkv.clone().requires_grad_(True)
    ctx_ref, lse_ref = attn_ref(qr, mask, B, S, H, nh, keep, drop_scale(thr))
    ctx_ref.backward(dctx)
    seed = torch.tensor([seedv], dtype=torch.int32, device=dev())
    qg, mg = to_gpu_bf16(qkv), mask.to(dev())
    ctx = torch.zeros((B * S, H), dtype=act_dtype(), device=dev())
    lse = torch.zeros((B, nh, S), dtype=torch.float32, device=dev())
    ops.attention_fwd(qg, mg, ctx, lse, B, S, H, nh, drop_p=p, seed=seed, tag=tag)
    name = "attn B%d S%d h%d p%.2f" % (B, S, nh, p)
    report(name + " lse", lse, lse_ref, 2e-3, 1e-3)
    report(name + " ctx", ctx, ctx_ref, 2e-3, 1e-2)
    dqkv = torch.zeros((B * S, 3 * H), dtype=act_dtype(), device=dev())
    ops.attention_bwd(qg, mg, ctx, lse, to_gpu_bf16(dctx), dqkv, B, S, H, nh, drop_p=p, seed=seed, tag=tag)
    gq = qr.grad
    report(name + " dq", dqkv[:, :H], gq[:, :H], 2e-3, 2e-2)
    report(name + " dk", dqkv[:, H:2 * H], gq[:, H:2 * H], 2e-3, 2e-2)
    report(name + " dv", dqkv[:, 2 * H:], gq[:, 2 * H:], 2e-3, 2e-2)


# ------------------------------------------------------------------------------------ embedding side
def test_seq_layout_and_embedding(ops):
    from oracle import vlbert_oracle as O
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                         vocab_size=512, max_position_embeddings=64, visual_region_classes=50)
    B, T, R = 4, 12, 5
    S = T + R + 1
    H = cfg.hidden_size
    boxes, im_info, text, rel, mlm_labels, mvrc_ops, mvrc_labels = syn.make_batch(B, T, R, vocab_size=512, region_classes=50,
                                                                                  seed=3, ragged=True)
    p = {k: bf(v) if v.dim() > 1 else v for k, v in O.init_params(cfg, seed=1).items()}
    text_mask, box_mask = text > 0, boxes[:, :, 0] > -1.5
    lay = ops.seq_layout(text_mask.to(dev()), box_mask.to(dev()), S)
    tl = text_mask.sum(1)
    no = box_mask.sum(1)
    assert torch.equal(lay["text_len"].cpu().long(), tl) and torch.equal(lay["nobj"].cpu().long(), no)
    am = (torch.arange(S)[None, :] <= (tl + no)[:, None]).float()
    assert torch.equal(lay["attn_mask"].cpu(), am)
    kinds = lay["code"].cpu() >> 16
    for b in range(B):
        exp = [1] * int(tl[b]) + [2] * int(no[b]) + [3] + [0] * (S - int(tl[b]) - int(no[b]) - 1)
        assert kinds[b].tolist() == exp
    # embedding forward vs the oracle (inputs: bf16-rounded visual parts)
    g = torch.Generator().manual_seed(5)
    text_vis_raw = bf(torch.randn(B, 1, H, generator=g))       # broadcast over tokens
    obj_vis_raw = bf(torch.randn(B, R, H, generator=g))
    obj_ling = bf(0.05 * torch.randn(B, R, H, generator=g))
    tv = bf(O.bert_layer_norm(text_vis_raw, p["vlbert.visual_ln_text.weight"], p["vlbert.visual_ln_text.bias"]))
    ov = bf(O.bert_layer_norm(obj_vis_raw, p["vlbert.visual_ln_object.weight"], p["vlbert.visual_ln_object.bias"]))
    # reference: oracle embedding with identity visual LN (feed the already-normalised parts)
    p_id = dict(p)
    for nme in ("text", "object"):
        p_id["vlbert.visual_ln_%s.weight" % nme] = torch.ones(H)
        p_id["vlbert.visual_ln_%s.bias" % nme] = torch.zeros(H)

    def ref_embed(tvv, ovv, olv, pp):
        # bypass the visual LN: (x-u)/sqrt(s) of an arbitrary vector is not identity, so add directly
        bs = B
        vl_text = F.embedding(text, pp["vlbert.word_embeddings.weight"]) + tvv.expand(B, T, H)
        vl_obj = olv + ovv
        grid = torch.arange(S)[None, :].expand(bs, S)
        te, oe = tl[:, None], (tl + no)[:, None]
        is_t, is_o, is_e = grid < te, (grid >= te) & (grid < oe), grid == oe
        vl = torch.zeros(bs, S, H)
        vl[is_t] = vl_text[text_mask]
        vl[is_o] = vl_obj[box_mask]
        vl[is_e] = pp["vlbert.end_embedding.weight"][0]
        typ = torch.zeros(bs, S, dtype=torch.long)
        typ[is_o | is_e] = 2
        pos = grid.clone()
        pos[is_o] = te.expand(bs, S)[is_o]
        pos[is_e] = (te + 1).squeeze(1)
        pre = vl + F.embedding(pos, pp["vlbert.position_embeddings.weight"]) + F.embedding(typ, pp["vlbert.token_type_embeddings.weight"])
        return pre, O.bert_layer_norm(pre, pp["vlbert.embedding_LayerNorm.weight"], pp["vlbert.embedding_LayerNorm.bias"])

    leaves = {k: p[k].clone().requires_grad_(True) for k in
              ("vlbert.word_embeddings.weight", "vlbert.end_embedding.weight", "vlbert.position_embeddings.weight",
               "vlbert.token_type_embeddings.weight", "vlbert.embedding_LayerNorm.weight", "vlbert.embedding_LayerNorm.bias")}
    tvr, ovr, olr = tv.clone().requires_grad_(True), ov.clone().requires_grad_(True), obj_ling.clone().requires_grad_(True)
    pre_ref, out_ref = ref_embed(tvr, ovr, olr, {**p, **leaves})
    dy = rnd(B, S, H, seed=6)
    valid = am.unsqueeze(-1)
    (out_ref * dy * valid).sum().backward()

    d = dev()
    pre = torch.empty((B * S, H), dtype=act_dtype(), device=d)
    out = torch.empty_like(pre)
    stats = torch.empty((B * S, 2), dtype=torch.float32, device=d)
    gw = lambda k: to_gpu_bf16(p[k])
    tvg, ovg, olg = to_gpu_bf16(tv.reshape(B, H)), to_gpu_bf16(ov.reshape(B * R, H)), to_gpu_bf16(obj_ling.reshape(B * R, H))
    ops.embed_fwd(lay, text.to(d), None, gw("vlbert.word_embeddings.weight"), gw("vlbert.position_embeddings.weight"),
                  gw("vlbert.token_type_embeddings.weight"), gw("vlbert.end_embedding.weight"), tvg, (H, 0), ovg, (R * H, H),
                  olg, (R * H, H), None, p["vlbert.embedding_LayerNorm.weight"].to(d), p["vlbert.embedding_LayerNorm.bias"].to(d),
                  pre, stats, out, B, T, R, S, H)
    report("embed fwd pre", pre.view(B, S, H), pre_ref, 1e-3, bar16(1e-2))
    report("embed fwd out", out.view(B, S, H), out_ref, 2e-3, bar16(1e-2))
    # backward
    V, P = cfg.vocab_size, cfg.max_position_embeddings
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=d)
    d_word, d_pos, d_type, d_end, d_g, d_b = z(V, H), z(P, H), z(3, H), z(1, H), z(H), z(H)
    d_tv, d_ov, d_ol = z(B, H), z(B * R, H), z(B * R, H)
    ops.embed_bwd(to_gpu_bf16((dy * valid).reshape(B * S, H)), pre, stats, p["vlbert.embedding_LayerNorm.weight"].to(d), lay,
                  text.to(d), None, None, d_word, d_pos, d_type, d_end, d_g, d_b, d_tv, (H, 0), d_ov, (R * H, H), d_ol,
                  (R * H, H), B, T, R, S, H)
    report("embed bwd d_word", d_word, leaves["vlbert.word_embeddings.weight"].grad, 2e-3, 1e-2)
    report("embed bwd d_pos", d_pos, leaves["vlbert.position_embeddings.weight"].grad, 2e-3, 1e-2)
    report("embed bwd d_type", d_type, leaves["vlbert.token_type_embeddings.weight"].grad, 2e-3, 1e-2)
    report("embed bwd d_end", d_end, leaves["vlbert.end_embedding.weight"].grad, 2e-3, 1e-2)
    report("embed bwd d_gamma", d_g, leaves["vlbert.embedding_LayerNorm.weight"].grad, 2e-3, 1e-2)
    report("embed bwd d_beta", d_b, leaves["vlbert.embedding_LayerNorm.bias"].grad, 2e-3, 1e-2)
    report("embed bwd d_text_vis", d_tv, tvr.grad.reshape(B, H), 2e-3, 1e-2)
    report("embed bwd d_obj_vis", d_ov, (ovr.grad * box_mask.unsqueeze(-1)).reshape(B * R, H), 2e-3, 1e-2)
    report("embed bwd d_obj_ling", d_ol, (olr.grad * box_mask.unsqueeze(-1)).reshape(B * R, H), 2e-3, 1e-2)
    # several workgroups per sample (the caller vouches that d_text_vis is zero): same results
    d_word2, d_pos2, d_type2, d_end2, d_g2, d_b2 = z(V, H), z(P, H), z(3, H), z(1, H), z(H), z(H)
    d_tv2, d_ov2, d_ol2 = z(B, H), z(B * R, H), z(B * R, H)
    ops.embed_bwd(to_gpu_bf16((dy * valid).reshape(B * S, H)), pre, stats, p["vlbert.embedding_LayerNorm.weight"].to(d), lay,
                  text.to(d), None, None, d_word2, d_pos2, d_type2, d_end2, d_g2, d_b2, d_tv2, (H, 0), d_ov2, (R * H, H), d_ol2,
                  (R * H, H), B, T, R, S, H, text_vis_zeroed=True)
    for name, a, b in (("d_word", d_word2, d_word), ("d_pos", d_pos2, d_pos), ("d_type", d_type2, d_type), ("d_end", d_end2, d_end),
                       ("d_gamma", d_g2, d_g), ("d_beta", d_b2, d_b), ("d_text_vis", d_tv2, d_tv), ("d_obj_vis", d_ov2, d_ov)):
        report("embed bwd split " + name, a, b.cpu(), 1e-4, 1e-4)
    # table mode for the linguistic part
    table = bf(0.05 * torch.randn(2, H, generator=g))
    sel = mvrc_ops.clone()
    olt = table[sel]
    pre_ref2, out_ref2 = ref_embed(tv, ov, olt, p)
    ops.embed_fwd(lay, text.to(d), None, gw("vlbert.word_embeddings.weight"), gw("vlbert.position_embeddings.weight"),
                  gw("vlbert.token_type_embeddings.weight"), gw("vlbert.end_embedding.weight"), tvg, (H, 0), ovg, (R * H, H),
                  to_gpu_bf16(table), (0, 0), sel.to(d), p["vlbert.embedding_LayerNorm.weight"].to(d),
                  p["vlbert.embedding_LayerNorm.bias"].to(d), pre, stats, out, B, T, R, S, H)
    report("embed fwd (table mode)", out.view(B, S, H), out_ref2, 2e-3, bar16(1e-2))


def test_obj_prep(ops):
    from oracle import vlbert_oracle as O
    syn = pkg("synthetic")
    B, R = 3, 6
    boxes, im_info, text, rel, mlm_labels, mvrc_ops, mvrc_labels = syn.make_batch(B, 8, R, vocab_size=512, region_classes=10,
                                                                                  seed=9, ragged=True)
    mask_emb = torch.rand(2048, generator=torch.Generator().manual_seed(1))
    out = torch.empty((B * R, 4096), dtype=act_dtype(), device=dev())
    ops.obj_prep_fwd(boxes.to(dev()), im_info.to(dev()), mvrc_ops.to(dev()), mask_emb.to(dev()), out)
    box_mask = boxes[:, :, 0] > -1.5
    feats = boxes[:, :, 4:].clone()
    feats[mvrc_ops == 1] = mask_emb
    b6 = torch.cat((boxes[:, :, :4], im_info[:, None, :2].expand(B, R, 2)), -1).reshape(B * R, 6)
    coord = O.coordinate_embeddings(b6, 256).reshape(B * R, 2048)
    ref = torch.cat((coord, feats.reshape(B * R, 2048)), -1) * box_mask.reshape(B * R, 1)
    report("obj_prep (coord || feature)", out, ref, 4e-3, bar16(4e-3))


def test_gather_combine_relu(ops):
    B, T, R, H = 3, 6, 4, 64
    S = T + R + 1
    g = torch.Generator().manual_seed(2)
    tm = torch.tensor([[1] * 6, [1] * 4 + [0] * 2, [1] * 5 + [0]], dtype=torch.bool)
    om = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0], [1, 1, 1, 0]], dtype=torch.bool)
    lay = ops.seq_layout(tm.to(dev()), om.to(dev()), S)
    x = rnd(B * S, H, seed=3)
    tout = torch.empty((B * T, H), dtype=act_dtype(), device=dev())
    oout = torch.empty((B * R, H), dtype=act_dtype(), device=dev())
    ops.gather_rows(to_gpu_bf16(x), lay["text_rows"].view(-1), tout)
    ops.gather_rows(to_gpu_bf16(x), lay["obj_rows"].view(-1), oout)
    xv = x.view(B, S, H)
    report("gather text rows", tout.view(B, T, H), xv[:, :T], 0, 0)
    ref_o = torch.zeros(B, R, H)
    tl = tm.sum(1)
    for b in range(B):
        n = int(om[b].sum())
        ref_o[b, :n] = xv[b, int(tl[b]):int(tl[b]) + n]
    report("gather object rows", oout.view(B, R, H), ref_o, 0, 0)
    dt, do = rnd(B * T, H, seed=4), rnd(B * R, H, seed=5)
    dx = torch.empty((B * S, H), dtype=act_dtype(), device=dev())
    ops.head_grad_combine(to_gpu_bf16(dt), to_gpu_bf16(do), lay["code"], dx, B, T, R, S, H)
    ref = torch.zeros(B, S, H)
    ref[:, :T] += dt.view(B, T, H)
    for b in range(B):
        n = int(om[b].sum())
        ref[b, int(tl[b]):int(tl[b]) + n] += do.view(B, R, H)[b, :n]
    report("head grad combine", dx.view(B, S, H), ref, 1e-6, bar16(8e-3))
    gsrc = torch.randn(B * R * H, generator=g)
    y = rnd(B * R * H, seed=6)
    o = torch.empty((B * R * H,), dtype=act_dtype(), device=dev())
    ops.relu_bwd_cast(gsrc.to(dev()), to_gpu_bf16(y), o)
    report("relu bwd cast", o, gsrc * (y > 0), 1e-6, bar16(8e-3))


# ------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("rows,V,ld", [(37, 512, 512), (16, 30522, 30528), (9, 300, 304)])
def test_ce_fwd_bwd(ops, rows, V, ld):
    x = rnd(rows, V, seed=40, scale=2.0)
    g = torch.Generator().manual_seed(41)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[torch.rand(rows, generator=g) < 0.5] = -1
    labels[0] = V - 1
    xr = x.clone().requires_grad_(True)
    loss = F.cross_entropy(xr, labels, ignore_index=-1)
    loss.backward()
    buf = torch.full((rows, ld), 7.0, dtype=act_dtype(), device=dev())
    buf[:, :V] = to_gpu_bf16(x)
    counts = torch.zeros(1, device=dev())
    lo = torch.zeros(1, device=dev())
    cp = torch.zeros((rows, ld), dtype=act_dtype(), device=dev())
    ops.ce_fwd_bwd(buf, V, labels.to(dev()), counts, lo, logits_copy=cp)
    report("ce loss V=%d" % V, lo, loss.detach().reshape(1), 1e-4, 1e-3)
    report("ce dlogits", buf[:, :V], xr.grad, 1e-5, bar16(1e-2))
    assert float(buf[:, V:].float().abs().max() if ld > V else 0.0) == 0.0
    report("ce logits copy", cp[:, :V], x, 0, 0)
    assert float(counts) == float((labels >= 0).sum())


def test_soft_ce_fwd_bwd(ops):
    from oracle import vlbert_oracle as O
    rows, C, ld = 29, 1601, 1664
    x = rnd(rows, C, seed=42, scale=2.0)
    g = torch.Generator().manual_seed(43)
    t = torch.softmax(torch.randn(rows, C, generator=g), -1)
    t[torch.rand(rows, generator=g) < 0.4] = 0
    t[1] = 0
    t[2] = torch.softmax(torch.randn(C, generator=g), -1) * 1.05
    xr = x.clone().requires_grad_(True)
    loss = O.soft_cross_entropy(xr, t)
    loss.backward()
    buf = torch.full((rows, ld), 3.0, dtype=act_dtype(), device=dev())
    buf[:, :C] = to_gpu_bf16(x)
    counts, lo, tsum = torch.zeros(1, device=dev()), torch.zeros(1, device=dev()), torch.zeros(rows, device=dev())
    ops.soft_ce_fwd_bwd(buf, C, t.to(dev()), tsum, counts, lo)
    report("soft-ce loss", lo, loss.detach().reshape(1), 1e-4, 1e-3)
    report("soft-ce dlogits", buf[:, :C], xr.grad, 1e-5, bar16(1e-2))
    assert float(buf[:, C:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------ optimizer
def test_adamw_and_sumsq(ops):
    from oracle import vlbert_oracle as O
    n = 100003
    g0 = torch.Generator().manual_seed(50)
    p = torch.randn(n, generator=g0)
    grads = [torch.randn(n, generator=g0) * 3 for _ in range(3)]
    lr, wd, max_norm = 1e-3, 1e-2, 10.0
    state = torch.tensor([lr, 0.9, 0.999, 1e-6, wd, 0.0, max_norm, 0.0], dtype=torch.float32, device=dev())
    pg, m, v = p.clone().to(dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    p16 = torch.empty(n, dtype=act_dtype(), device=dev())
    pr, mr, vr = p.clone(), torch.zeros(n), torch.zeros(n)
    for step, g in enumerate(grads, 1):
        gg = g.to(dev())
        ops.sumsq(gg, state[7:8])
        if step == 1:
            report("sumsq", state[7:8], (g.double() ** 2).sum().float().reshape(1), 0, 1e-5)
        ops.adamw_step(pg, gg, m, v, p16, state)
        coef = O.clip_coef(float(g.double().norm()), max_norm)
        O.adamw_step(pr, g * coef, mr, vr, step, lr, eps=1e-6, weight_decay=wd)
    report("adamw p after 3 steps", pg, pr, 1e-6, 1e-5)
    report("adamw m", m, mr, 1e-6, 1e-5)
    report("adamw v", v, vr, 1e-6, 1e-5)
    report("adamw bf16 copy", p16, pr, 1e-6, bar16(8e-3))
    assert float(state[5]) == 3.0 and float(state[7]) == 0.0


def test_adamw_and_sumsq_on_bf16_wire_gradient(ops):
    """vlb_sumsq_det / vlb_adamw_step with g_is_bf16: the optimizer fed with the bf16 wire image of the data-parallel exchange must
    equal the fp32 entry points fed with the same (bf16-representable) values; grad_scale = 1/world folded in."""
    from oracle import vlbert_oracle as O
    n = 70001
    g0 = torch.Generator().manual_seed(51)
    p = torch.randn(n, generator=g0)
    g = bf(torch.randn(n, generator=g0) * 2)
    lr, wd, max_norm, scale = 1e-3, 1e-2, 1.0, 0.125
    mk = lambda: torch.tensor([lr, 0.9, 0.999, 1e-6, wd, 0.0, max_norm, 0.0], dtype=torch.float32, device=dev())
    part = torch.zeros(2048, device=dev())
    res = []
    for wire in (torch.float32, act_dtype()):
        state = mk()
        pg, m, v = p.clone().to(dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
        p16 = torch.empty(n, dtype=act_dtype(), device=dev())
        gg = g.to(dev()).to(wire)
        ops.sumsq_det(gg, part, state[7:8])
        ss = float(state[7])
        ops.adamw_step(pg, gg, m, v, p16, state, grad_scale=scale)
        res.append((ss, pg.cpu(), m.cpu(), v.cpu(), p16.float().cpu()))
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a, b)
    pr, mr, vr = p.clone(), torch.zeros(n), torch.zeros(n)
    coef = O.clip_coef(float(g.double().norm()) * scale, max_norm) * scale
    O.adamw_step(pr, g * coef, mr, vr, 1, lr, eps=1e-6, weight_decay=wd)
    report("adamw (bf16 wire gradient) p", res[1][1], pr, 1e-6, 1e-5)


def test_sharded_optimizer_kernels_match_flat_adamw(ops):
    """vlb_sumsq_ranges_det / vlb_adamw_step_ranges (the data-parallel SHARDED optimizer: a rank updates its slice of every bucket from
    a compact reduced-gradient image and emits the bf16 copy into a compact image): the union of two 'ranks' owned slices must
    reproduce vlb_sumsq_*_det + vlb_adamw_step over the whole buffer bit for bit (sum of squares: to fp32 summation order)."""
    n, world = 64 * 2 * 531, 2
    g0 = torch.Generator().manual_seed(52)
    p = torch.randn(n, generator=g0)
    lr, wd, max_norm, scale = 1e-3, 1e-2, 1.0, 0.5
    mk = lambda: torch.tensor([lr, 0.9, 0.999, 1e-6, wd, 3.0, max_norm, 0.0], dtype=torch.float32, device=dev())
    part = torch.zeros(2048, device=dev())
    cuts = [0, 128 * 40, 128 * 300, n]                       # three buckets, each split evenly over the two ranks
    for wire in (torch.float32, act_dtype()):
        g = (torch.randn(n, generator=g0) * 2).to(wire).to(dev())
        state = mk()
        pf, m, v = p.clone().to(dev()), torch.full((n,), 0.01, device=dev()), torch.full((n,), 0.02, device=dev())
        p16 = torch.empty(n, dtype=act_dtype(), device=dev())
        ops.sumsq_det(g, part, state[7:8])
        ss = float(state[7])
        ops.adamw_step(pf, g, m, v, p16, state, grad_scale=scale)
        ps, ms, vs = p.clone().to(dev()), torch.full((n,), 0.01, device=dev()), torch.full((n,), 0.02, device=dev())
        w16 = torch.zeros(n, dtype=act_dtype(), device=dev())
        sq = torch.zeros(1, device=dev())
        shards = []
        for r in range(world):
            rows, comp = [], []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                k = (hi - lo) // world
                rows.append((lo + r * k, lo // world, k))
                comp.append(g[lo + r * k:lo + (r + 1) * k])
            tbl = ops.ShardRanges(rows, dev())
            gs = torch.cat(comp).contiguous()                # the compact image a reduce-scatter leaves
            st = mk()
            tbl.sumsq(gs, part, st[7:8])
            sq += st[7:8]
            shards.append((tbl, gs, rows))
        assert abs(float(sq) - ss) <= 1e-5 * ss
        for tbl, gs, rows in shards:
            st = mk()
            st[7] = ss                                       # the all-reduced norm
            ws = torch.zeros(n // world, dtype=act_dtype(), device=dev())
            tbl.adamw(ps, gs, ms, vs, ws, st, grad_scale=scale)
            assert float(st[5]) == 4.0 and float(st[7]) == 0.0        # one step advance per call, norm cleared
            for p0, c0, k in rows:
                w16[p0:p0 + k] = ws[c0:c0 + k]
        assert torch.equal(ps, pf) and torch.equal(ms, m) and torch.equal(vs, v) and torch.equal(w16, p16), str(wire)


def test_fp16_residual_stream_overflow_is_flagged(ops):
    """A pre-LayerNorm sum beyond the fp16 range (65504) becomes inf in the GEMM epilogue's conversion; the LayerNorm forward that
    reads the row raises the sticky device flag (vlb_nonfinite_status) instead of training on silently -- random-init tests never
    reach it, pretrained BERT's outlier channels could."""
    lib = pkg("_lib")
    lib.nonfinite_status(reset=True)
    M, N, K = 256, 128, 64
    A, B = to_gpu_bf16(rnd(M, K, seed=1)), to_gpu_bf16(rnd(N, K, seed=2))
    bias = torch.zeros(N, device=dev())
    Z = torch.zeros((M, N), dtype=torch.float16, device=dev())
    g, b = torch.ones(N, device=dev()), torch.zeros(N, device=dev())
    y, st = torch.zeros((M, N), dtype=act_dtype(), device=dev()), torch.zeros((M, 2), device=dev())
    ops.gemm_nt(A, B, Z, bias=bias)
    ops.layernorm_fwd(Z, g, b, y, st)
    assert lib.nonfinite_status() == 0
    bias[5] = 7.0e4                                      # > 65504: the fp16 store overflows
    ops.gemm_nt(A, B, Z, bias=bias)
    assert bool(torch.isinf(Z[:, 5]).all())
    ops.layernorm_fwd(Z, g, b, y, st)
    assert lib.nonfinite_status(reset=False) == 1        # bit 0: an fp16 row
    assert lib.nonfinite_status(reset=True) == 1 and lib.nonfinite_status() == 0      # sticky until reset


def test_bce_logits_and_dropout(ops):
    """vlb_bce_logits_fwd_bwd (VQA answer loss x answers, gradient in place, padded columns zeroed) and vlb_dropout_bf16."""
    B, A, Ap = 5, 37, 64
    g = torch.Generator().manual_seed(60)
    x = bf(torch.randn(B, A, generator=g) * 3)
    y = (torch.rand(B, A, generator=g) < 0.2).float() * torch.rand(B, A, generator=g)
    logits = torch.full((B, Ap), 9.0, dtype=act_dtype(), device=dev())
    logits[:, :A] = x.to(dev())
    copy = torch.zeros_like(logits)
    loss = torch.tensor([0.25], device=dev())
    ops.bce_logits_fwd_bwd(logits, A, y.to(dev()), loss, gscale=2.0, logits_copy=copy)
    xr = x.clone().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(xr, y) * A
    ref.backward()
    assert abs(float(loss) - 0.25 - float(ref)) < 1e-4 * float(ref)
    report("bce dlogits (x gscale)", logits[:, :A], 2.0 * xr.grad, 1e-4, bar16(1e-2))
    assert float(logits[:, A:].float().abs().max()) == 0.0 and torch.equal(copy[:, :A].float().cpu(), x)
    n = 10007
    v = rnd(n, seed=61)
    out = torch.zeros(n, dtype=act_dtype(), device=dev())
    seed = torch.tensor([777], dtype=torch.int32, device=dev())
    ops.dropout_bf16(to_gpu_bf16(v), out, 0.3, seed, 5)
    keep = torch.from_numpy(keep_mask(777, 5, np.arange(n), drop_thr(0.3)))
    report("dropout_bf16", out, v * keep * drop_scale(drop_thr(0.3)), 0, bar16(8e-3))
    ops.dropout_bf16(to_gpu_bf16(v), out, 0.0, None, 5)
    report("dropout_bf16 p=0", out, v, 0, 0)


def test_sumsq_deterministic(ops):
    """vlb_sumsq_det: right value, accumulates into *out, and the same bits on every call (the atomic version is not)."""
    n = 3_000_017
    g = torch.randn(n, generator=torch.Generator().manual_seed(51)).to(dev())
    ws = torch.zeros(2048, device=dev())
    outs = []
    for _ in range(4):
        out = torch.tensor([1.5], device=dev())
        ops.sumsq_det(g, ws, out)
        outs.append(float(out))
    want = float((g.double() ** 2).sum()) + 1.5
    assert abs(outs[0] - want) <= 2e-6 * want, (outs[0], want)
    assert len(set(outs)) == 1, outs
    small = torch.tensor([3.0, 4.0], device=dev())
    out = torch.zeros(1, device=dev())
    ops.sumsq_det(small, ws[:1], out)
    assert float(out) == 25.0


def test_lr_schedule_on_device(ops):
    """vlb_lr_schedule_step against torch's LambdaLR driven with the oracle's lr_lambda in the reference's order:
    scheduler.step() then optimizer.step() (common/trainer.py:131-147), so optimizer step k uses lambda(k)."""
    from oracle import vlbert_oracle as O
    base, warm, total = 1e-4, 5, 23
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=base)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: O.warmup_linear_lr(s, warm, total))
    state = torch.tensor([123.0, 0.9, 0.999, 1e-6, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev())
    n = 64
    p, g, m, v = (torch.zeros(n, device=dev()) for _ in range(4))
    for k in range(1, total + 4):
        w.grad = torch.zeros(1)
        opt.step()
        sch.step()                    # lr used by optimizer step k in the reference's loop
        want = opt.param_groups[0]["lr"]
        ops.lr_schedule_step(state, ops.LR_WARMUP_LINEAR, base, warm, total)
        got = float(state[0])
        assert abs(got - want) <= 1e-6 * base + 1e-12, (k, got, want)
        ops.adamw_step(p, g, m, v, None, state)        # advances state[5]
    assert float(state[5]) == total + 3 and float(state[0]) == 0.0
    # warmup-constant and constant kinds
    state[5] = 2.0
    ops.lr_schedule_step(state, ops.LR_WARMUP_CONSTANT, base, 10, 0)
    assert abs(float(state[0]) - base * 0.3) < 1e-10
    state[5] = 50.0
    ops.lr_schedule_step(state, ops.LR_WARMUP_CONSTANT, base, 10, 0)
    assert abs(float(state[0]) - base) < 1e-7 * base          # fp32 storage of the lr
    ops.lr_schedule_step(state, ops.LR_CONSTANT, 3e-5, 0, 0)
    assert abs(float(state[0]) - 3e-5) < 1e-7 * 3e-5
    with pytest.raises(Exception):
        ops.lr_schedule_step(state, 7, base, 0, 0)


# ------------------------------------------------------------------------------------ ROIAlign
@pytest.mark.parametrize("sr", [1, 2, 0, 3])
def test_roi_align(ops, sr):
    from oracle import roi_align_oracle as R
    rng = np.random.RandomState(1)
    x = rng.randn(2, 6, 12, 17).astype(np.float32)
    rois = np.array([[0, 3.1, 2.2, 150.5, 120.0], [1, -20.0, -8.0, 90.0, 70.0], [1, 100.0, 60.0, 400.0, 300.0],
                     [0, 10.0, 10.0, 10.5, 10.2], [1, 0, 0, 271.0, 191.0]], dtype=np.float32)
    ph, pw, scale = 7, 5, 1.0 / 16
    ref = R.roi_align_forward(x, rois, scale, ph, pw, sr)
    out = torch.empty((rois.shape[0], 6, ph, pw), dtype=torch.float32, device=dev())
    ops.roi_align_fwd(torch.from_numpy(x).to(dev()), torch.from_numpy(rois).to(dev()), out, scale, sr)
    report("roi_align fwd sr=%d" % sr, out, torch.from_numpy(ref).float(), 1e-5, 1e-5)
    dy = rng.randn(*ref.shape).astype(np.float32)
    gref = R.roi_align_backward(dy, rois, scale, ph, pw, 2, 6, 12, 17, sr)
    gin = torch.full((2, 6, 12, 17), 5.0, dtype=torch.float32, device=dev())
    ops.roi_align_bwd(torch.from_numpy(dy).to(dev()), torch.from_numpy(rois).to(dev()), gin, scale, sr)
    report("roi_align bwd sr=%d" % sr, gin, torch.from_numpy(gref).float(), 1e-5, 1e-5)


def test_roi_align_debug_fixture(ops):
    """The reference's own fixture (common/lib/roi_pooling/debug.py:10-11)."""
    feature = torch.arange(81 * 2 * 3).view(2, 3, 9, 9).float().to(dev())
    rois = torch.tensor([[0, 0, 0, 9, 9], [1, 0, 0, 9, 9], [1, 0, 0, 7, 7]], dtype=torch.float32, device=dev())
    out = torch.empty((3, 3, 3, 3), dtype=torch.float32, device=dev())
    ops.roi_align_fwd(feature, rois, out, 1.0, 1)
    report("roi_align debug.py fixture", out[0, 0], torch.tensor([[15., 18, 21], [42, 45, 48], [69, 72, 75]]), 1e-5, 0)


def test_roi_align_module_api_drop_in(ops):
    """The seam the reference itself exposes: `common.lib.roi_pooling.roi_align.ROIAlign` / `roi_align` and the
    `C_ROIPooling` functions behind them -- the reference's debug.py fixture through the MODULE, autograd backward against the numpy
    oracle, non-contiguous / non-fp32 inputs (the module casts, like the reference), an empty RoI list, and the error contract."""
    from oracle import roi_align_oracle as R
    RA = pkg("common.lib.roi_pooling.roi_align")
    C = pkg("common.lib.roi_pooling.C_ROIPooling")
    feature = torch.arange(81 * 2 * 3).view(2, 3, 9, 9).float().to(dev())
    rois = torch.tensor([[0, 0, 0, 9, 9], [1, 0, 0, 9, 9], [1, 0, 0, 7, 7]], dtype=torch.float32, device=dev())
    layer = RA.ROIAlign((3, 3), 1.0, 1)
    assert "output_size=(3, 3)" in repr(layer)
    out = layer(feature, rois)
    report("ROIAlign module, debug.py fixture", out[0, 0], torch.tensor([[15., 18, 21], [42, 45, 48], [69, 72, 75]]), 1e-5, 0)
    # autograd through the Function; half input + non-contiguous rois are cast / made contiguous by the wrapper chain
    rng = np.random.RandomState(3)
    x = torch.from_numpy(rng.randn(2, 6, 12, 17).astype(np.float32))
    rois_np = np.array([[0, 3.2, 2.1, 40.5, 30.0], [1, 0, 0, 60, 44], [1, 10, 5, 12, 9], [0, -4, -4, 20, 20]], dtype=np.float32)
    xg = x.to(dev()).requires_grad_(True)
    wide = torch.zeros((4, 7), device=dev())
    wide[:, :5] = torch.from_numpy(rois_np).to(dev())
    y = RA.roi_align(xg, wide[:, :5], (4, 5), 0.25, 2)
    ref = R.roi_align_forward(x.numpy(), rois_np, 0.25, 4, 5, 2)
    report("roi_align function fwd", y, torch.from_numpy(ref).float(), 1e-5, 1e-5)
    dy = rng.randn(*ref.shape).astype(np.float32)
    y.backward(torch.from_numpy(dy).to(dev()))
    gref = R.roi_align_backward(dy, rois_np, 0.25, 4, 5, 2, 6, 12, 17, 2)
    report("roi_align function bwd (autograd)", xg.grad, torch.from_numpy(gref).float(), 1e-5, 1e-5)
    yh = RA.ROIAlign((4, 5), 0.25, 2)(x.to(dev()).half(), torch.from_numpy(rois_np).to(dev()).double())
    assert yh.dtype == torch.float32
    report("ROIAlign module on half features / double rois", yh, torch.from_numpy(R.roi_align_forward(x.half().float().numpy(), rois_np, 0.25, 4, 5,
                                                                                                      2)).float(), 1e-5, 1e-5)
    empty = RA.ROIAlign((4, 5), 0.25, 2)(x.to(dev()), torch.zeros((0, 5), device=dev()))
    assert tuple(empty.shape) == (0, 6, 4, 5)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.roi_align_forward(x, torch.from_numpy(rois_np), 0.25, 4, 5, 2)
    with pytest.raises(RuntimeError, match="float32"):
        C.roi_align_forward(x.to(dev()).half(), torch.from_numpy(rois_np).to(dev()), 0.25, 4, 5, 2)
    with pytest.raises(RuntimeError, match="dead code"):
        C.roi_pool_forward(x, rois_np)


def test_error_path_raises(ops):
    A = torch.zeros((64, 100), dtype=act_dtype(), device=dev())
    C = torch.zeros((64, 64), dtype=act_dtype(), device=dev())
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ops.gemm_nt(A[:, :96], A[:, :96], C, K=96)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cast_f32_bf16(torch.zeros(4), torch.zeros(4, dtype=act_dtype()))


@pytest.mark.parametrize("rows,H,f16", [(7001, 768, True), (4099, 1024, False), (25856, 768, True), (5, 768, False)])
def test_layernorm_kernel_variants_agree(ops, rows, H, f16):
    """The forward with 1 / 2 / 4 rows per wave and the backward in its plain (1) and two-rows-in-flight (2) forms
    (vlb_gemm_set_option "ln_fwd_rows" / "ln_bwd4"): the same arithmetic per row.  The forward variants are one template and agree bit
    for bit; the backward variants are separate kernels whose fp32 expressions the compiler contracts into different FMA patterns, so
    they agree to one 16-bit rounding step, with IDENTICAL dropout masks; the parameter-gradient sums agree to fp32 summation order.
    Variant 1 is what test_layernorm_fwd_bwd pins to torch."""
    lib = pkg("_lib")
    g = torch.Generator().manual_seed(rows + H)
    x = (torch.randn(rows, H, generator=g) * 1.5 + 0.3)
    x = (x.half() if f16 else x.to(act_dtype())).to(dev())
    dy = to_gpu_bf16(torch.randn(rows, H, generator=g))
    gamma, beta = (1 + 0.2 * torch.randn(H, generator=g)).to(dev()), (0.1 * torch.randn(H, generator=g)).to(dev())
    seed = torch.tensor([777], dtype=torch.int32, device=dev())
    outs = {}
    try:
        for rpw in (1, 2, 4):
            lib.gemm_set_option("ln_fwd_rows", rpw)
            y = torch.full((rows, H), 9.0, dtype=act_dtype(), device=dev())
            st = torch.full((rows, 2), 9.0, device=dev())
            ops.layernorm_fwd(x, gamma, beta, y, st)
            outs["f%d" % rpw] = (y, st)
        for k in (2, 4):
            assert torch.equal(outs["f%d" % k][0], outs["f1"][0]) and torch.equal(outs["f%d" % k][1], outs["f1"][1]), k
        stats = outs["f1"][1]
        for mode in (1, 2):
            lib.gemm_set_option("ln_bwd4", mode)
            for form in ("both", "dx", "drop"):
                dx = torch.full((rows, H), 9.0, dtype=act_dtype(), device=dev()) if form != "drop" else None
                dd = torch.full((rows, H), 9.0, dtype=act_dtype(), device=dev()) if form != "dx" else None
                dg, db = torch.zeros(H, device=dev()), torch.zeros(H, device=dev())
                ws = torch.zeros(ops.ln_bwd_workspace_floats(H), device=dev())
                ops.layernorm_bwd(dy, x, stats, gamma, dx=dx, dx_drop=dd, drop_p=0.1 if dd is not None else 0.0, seed=seed, tag=3,
                                  dgamma=dg, dbeta=db, workspace=ws)
                outs[(mode, form)] = (dx, dd, dg, db)
        torch.cuda.synchronize()
        for mode in (2,):
            for form in ("both", "dx", "drop"):
                a, b = outs[(mode, form)], outs[(1, form)]
                for t, u in zip(a[:2], b[:2]):
                    assert (t is None) == (u is None), (mode, form)
                    if t is not None:
                        err = (t.float() - u.float()).abs()
                        bad = err > 2.0 ** -7 * u.float().abs() + 1e-6
                        if not torch.equal(t == 0, u == 0) or bool(bad.any()):      # (short message: the tensors are large)
                            raise AssertionError("ln_bwd4 %d vs 1, outputs %s: %d elements off, max |diff| %.3e, zero patterns equal %s, first bad row %s"
                                                 % (mode, form, int(bad.sum()), float(err.max()), torch.equal(t == 0, u == 0),
                                                    int(bad.any(dim=1).nonzero()[0]) if bool(bad.any()) else None))
                for t, u in zip(a[2:], b[2:]):
                    assert float((t - u).abs().max()) <= 1e-4 * max(1.0, float(u.abs().max())), (mode, form)
        d = outs[(2, "both")]
        assert float((d[1] == 0).float().mean()) > 0.05 and not torch.equal(d[0], d[1])
    finally:
        lib.gemm_set_option("ln_fwd_rows", 0)
        lib.gemm_set_option("ln_bwd4", 1)


def test_layernorm_bwd_deferred_parameter_gradients_batched(ops):
    """vlb_layernorm_bwd_deferred + vlb_ln_param_finalize_batch: three LayerNorm backwards leave their partial dgamma / dbeta vectors in
    workspaces of their own and ONE launch adds them into the gradients -- equal (up to fp32 summation order) to the per-call finalize
    of vlb_layernorm_bwd; dx is bit-identical; a small call (<= 32 workgroups) reports 0 partial vectors and adds its sums directly."""
    H = 768
    g = torch.Generator().manual_seed(7)
    entries, ref = [], []
    for k, rows in enumerate((1000, 4096, 700)):
        x = (torch.randn(rows, H, generator=g) * 1.5).half().to(dev())
        dy = to_gpu_bf16(torch.randn(rows, H, generator=g))
        gamma = torch.randn(H, generator=g).to(dev())
        y = torch.empty(rows, H, dtype=act_dtype(), device=dev())
        stats = torch.empty(rows, 2, device=dev())
        ops.layernorm_fwd(x, gamma, torch.zeros(H, device=dev()), y, stats)
        dx0, dx1 = torch.empty_like(dy), torch.empty_like(dy)
        dg0, db0 = torch.full((H,), 0.5, device=dev()), torch.full((H,), -0.25, device=dev())
        dg1, db1 = dg0.clone(), db0.clone()
        ws0 = torch.empty(ops.ln_bwd_workspace_floats(H), device=dev())
        ws1 = torch.empty(ops.ln_bwd_workspace_floats(H), device=dev())
        ops.layernorm_bwd(dy, x, stats, gamma, dx=dx0, dgamma=dg0, dbeta=db0, workspace=ws0)
        slabs = ops.layernorm_bwd(dy, x, stats, gamma, dx=dx1, dgamma=dg1, dbeta=db1, workspace=ws1, defer=True)
        assert torch.equal(dx0, dx1)
        assert slabs == (rows + 7) // 8
        entries.append((ws1, slabs, dg1, db1))
        ref.append((dg0, db0))
    ops.ln_param_finalize_batch(entries, H)
    torch.cuda.synchronize()
    for (ws, slabs, dg1, db1), (dg0, db0) in zip(entries, ref):
        assert float((dg1 - dg0).abs().max()) < 1e-4 * max(1.0, float(dg0.abs().max()))
        assert float((db1 - db0).abs().max()) < 1e-4 * max(1.0, float(db0.abs().max()))
    # small call: direct atomics, nothing deferred
    rows = 64
    x = torch.randn(rows, H, generator=g).half().to(dev())
    dy = to_gpu_bf16(torch.randn(rows, H, generator=g))
    gamma = torch.ones(H, device=dev())
    stats = torch.empty(rows, 2, device=dev())
    ops.layernorm_fwd(x, gamma, torch.zeros(H, device=dev()), torch.empty(rows, H, dtype=act_dtype(), device=dev()), stats)
    dg, db = torch.zeros(H, device=dev()), torch.zeros(H, device=dev())
    ws = torch.empty(ops.ln_bwd_workspace_floats(H), device=dev())
    assert ops.layernorm_bwd(dy, x, stats, gamma, dgamma=dg, dbeta=db, workspace=ws, defer=True) == 0
    torch.cuda.synchronize()
    assert float((db - dy.float().sum(0)).abs().max()) < 1e-2


# ------------------------------------------------------------------------------------ ranged copy, scale, casts
def test_copy_ranges_pack_unpack(ops):
    """vlb_copy_ranges_f32 (pack / unpack of the fp32-read parameters of the sharded optimizer): lengths below, at and above the
    1024-float block of block_start, unordered and non-adjacent offsets, 16-byte aligned on both sides / one side / neither (the
    kernel takes a vector or a scalar path per thread).  Equal to the plain indexed copy, everything outside the ranges untouched,
    pack + inverse unpack restores the source, an empty table launches nothing."""
    rows = [(9000, 17, 1), (0, 7000, 1023), (4003, 100, 1024), (2000, 3000, 1025), (10000, 9001, 5000)]      # (src, dst, length)
    n = 16000
    src = torch.randn(n, generator=torch.Generator().manual_seed(70))
    want = torch.full((n,), -7.0)
    for s, d, ln in rows:
        want[d:d + ln] = src[s:s + ln]
    srcg = src.to(dev())
    dst = torch.full((n,), -7.0, device=dev())
    pack = ops.CopyRanges(rows + [(5, 6, 0)], dev())           # (an empty row is dropped on the host)
    assert pack.n == len(rows) and pack.total == 1 + 1 + 1 + 2 + 5
    pack.run(srcg, dst)
    assert torch.equal(dst.cpu(), want)
    assert torch.equal(srcg.cpu(), src)
    back = torch.full((n,), -9.0, device=dev())
    ops.CopyRanges([(d, s, ln) for s, d, ln in rows], dev()).run(dst, back)
    restored = torch.full((n,), -9.0)
    for s, d, ln in rows:
        restored[s:s + ln] = src[s:s + ln]
    assert torch.equal(back.cpu(), restored)
    empty = ops.CopyRanges([], dev())
    assert empty.n == 0 and empty.total == 0
    empty.run(srcg, back)
    ops.CopyRanges([(1, 2, 0)], dev()).run(srcg, back)
    assert torch.equal(back.cpu(), restored)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 1024, 4099])
def test_scale_f32_exact(ops, n, off):
    """x *= alpha is one fp32 multiply per element: bit-identical to torch's, for a view that starts 16-byte aligned or not; the
    elements around the view keep their contents."""
    alpha = float(np.float32(0.3))
    x = torch.randn(n + off + 5, generator=torch.Generator().manual_seed(71 + n)) * 100
    want = x.clone()
    want[off:off + n] = x[off:off + n] * torch.tensor(alpha, dtype=torch.float32)
    buf = x.to(dev())
    ops.scale_f32(buf[off:off + n], alpha)
    assert torch.equal(buf.cpu(), want), "max diff %g" % float((buf.cpu() - want).abs().max())


def _cast_specials():
    """fp32 inputs at which a conversion to the library's 16-bit type can go wrong."""
    fi = torch.finfo(act_dtype())
    eps, big, tiny = fi.eps, fi.max, fi.tiny                   # 16-bit: spacing at 1, largest finite, smallest normal
    sub = tiny * eps                                           # smallest 16-bit subnormal
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float()
    nxt = lambda v, d: torch.nextafter(f32(v), f32(d))
    ulp_big = big * eps / (2.0 - eps)                          # 16-bit spacing below `big` = (2 - eps) 2^emax
    vals = [f32(1.0 + eps / 2), f32(-(1.0 + eps / 2)),         # ties: 1 (even) | 1 + eps -> down to 1
            f32(1.0 + 1.5 * eps), f32(-(1.0 + 1.5 * eps)),     # ties: 1 + eps | 1 + 2 eps (even) -> up
            nxt(1.0 + eps / 2, 2.0), nxt(1.0 + eps / 2, 0.0),  # just above / below a tie
            nxt(1.0 + 1.5 * eps, 2.0), nxt(1.0 + 1.5 * eps, 0.0),
            f32(0.0), f32(-0.0),
            f32(big), f32(-big), nxt(big, float("inf")), nxt(-big, float("-inf")),      # largest finite and the first fp32 beyond it
            f32(big + ulp_big / 2), nxt(big + ulp_big / 2, 0.0),                        # tie between `big` (odd) and 2^emax: -> inf | just below: big
            f32(tiny), nxt(tiny, 0.0), f32(sub), f32(-sub), f32(sub / 2), nxt(sub / 2, 1.0), f32(1.5 * sub), f32(2.5 * sub), f32(0.75 * sub),
            f32(1e-40), f32(-1e-40), f32(1.4e-45),                                       # fp32 subnormals
            f32(float("inf")), f32(float("-inf")), f32(float("nan"))]
    return torch.stack(vals)


@pytest.mark.parametrize("n", [1, 7, 8, 4099])
def test_cast_f32_to_16bit_rounds_like_torch(ops, n):
    """vlb_cast_f32_bf16 == x.to(the 16-bit type): round to nearest even, bit for bit (+-0 included), NaN stays NaN; every special
    value visits the vector body and the scalar tail of the kernel (n = 7: one of each; 4099: three tail elements); the buffer behind
    the n elements is untouched."""
    sp = _cast_specials()
    g = torch.Generator().manual_seed(72)
    pool = torch.cat((sp, torch.randn(61, generator=g), torch.randn(32, generator=g) * 1e-3, torch.randn(32, generator=g) * 3e4))
    for shift in range(0, len(sp) + 3, 3 if n > 1 else 1):
        x = pool[(torch.arange(n) + shift - n // 4 * 4) % len(pool)]          # pool[shift:] starts the scalar tail (if n has one)
        want = x.to(act_dtype())
        dst = torch.full((n + 9,), -3.0, dtype=act_dtype(), device=dev())
        ops.cast_f32_bf16(x.to(dev()), dst[:n])
        got = dst.cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got[:n]), nan), "shift %d: NaN positions differ" % shift
        gb, wb = got[:n].view(torch.int16)[~nan], want.view(torch.int16)[~nan]
        bad = (gb != wb).nonzero().flatten()
        assert bad.numel() == 0, "shift %d: %d differ, first: fp32 %r -> %r, torch %r" % (
            shift, bad.numel(), float(x[~nan][bad[0]]), float(got[:n][~nan][bad[0]]), float(want[~nan][bad[0]]))
        assert float((got[n:].float() + 3.0).abs().max()) == 0.0, "elements past n were written"


def test_cast_16bit_to_f32_every_pattern(ops):
    """vlb_cast_bf16_f32 over all 65 536 bit patterns of the 16-bit type: every finite one (subnormals, +-0 included) equals .float()
    bit for bit, infinities keep their sign and NaNs stay NaN; short odd lengths from an odd start; the buffer tail stays untouched."""
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(act_dtype())
    want = pat.float()
    src = pat.to(dev())
    dst = torch.full((65536 + 8,), -3.0, device=dev())
    ops.cast_bf16_f32(src, dst[:65536])
    got = dst.cpu()
    nan = torch.isnan(want)
    assert int(torch.isfinite(want).sum()) > 63000 and torch.equal(torch.isnan(got[:65536]), nan)
    assert torch.equal(got[:65536].view(torch.int32)[~nan], want.view(torch.int32)[~nan])
    assert float((got[65536:] + 3.0).abs().max()) == 0.0
    for n in (1, 7, 8, 4099):
        lo = 0x3001                                            # odd element offset; finite patterns in both 16-bit types
        dst = torch.full((n + 8,), -3.0, device=dev())
        ops.cast_bf16_f32(src[lo:lo + n], dst[:n])
        got = dst.cpu()
        assert torch.equal(got[:n].view(torch.int32), want[lo:lo + n].view(torch.int32)), n
        assert float((got[n:] + 3.0).abs().max()) == 0.0, n
