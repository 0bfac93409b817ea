"""Parity (-m gpu) of the six kernels at the two ends of the training step: vlb_seq_layout, vlb_obj_prep_fwd, vlb_masked_colsum
(embed.hip), the row-validity pass of vlb_soft_ce_fwd_bwd and vlb_mlm_compact (loss.hip), vlb_ln_param_finalize_batch (layernorm.hip).

The reference of every case is a float64 or integer CPU statement written here (tests/embed_attn_refs.py for the MLM compaction and
its input generator).  Where a kernel promises a summation ORDER (soft_valid: a lane adds its columns lane, lane + 64, ... ascending,
then the xor butterfly of wave_sum; LayerNorm finalize: a thread adds its partial vectors r, r + 32, ... ascending, the four threads of
a column meet as (p0 + p1) + (p2 + p3)), the CPU statement adds fp32 numbers in that order and the comparison is bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import embed_attn_refs as R
from tests.gpu_util import TAG_DOWNSAMPLE, act_dtype, dev, drop_scale, drop_thr, keep_mask, pkg, report, to_gpu_bf16

pytestmark = pytest.mark.gpu
SENT = 7.25


@pytest.fixture(scope="module")
def ops():
    o = pkg("ops")
    name, cus = pkg("_lib").device_info(0)
    assert name.startswith("gfx950"), "these kernels are built for gfx950 only (got %s)" % name
    return o


def _seed(v):
    return torch.tensor([v], dtype=torch.int32, device=dev())


# ------------------------------------------------------------------------------------------------------ seq_layout
def _layout_statement(tm, om, S):
    """The serial walk: text tokens, then objects, then END, then PAD."""
    B, T = tm.shape
    Rr = om.shape[1]
    code = np.zeros((B, S), dtype=np.int32)
    attn = np.zeros((B, S), dtype=np.float32)
    text_rows = np.zeros((B, T), dtype=np.int32)
    obj_rows = np.full((B, Rr), -1, dtype=np.int32)
    tl, no = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = 0
        for t in range(T):
            if tm[b, t]:
                code[b, n] = (1 << 16) | t
                n += 1
        tl[b] = n
        for r in range(Rr):
            if om[b, r]:
                obj_rows[b, r] = b * S + n
                code[b, n] = (2 << 16) | r
                n += 1
        no[b] = n - tl[b]
        code[b, n] = 3 << 16
        n += 1
        attn[b, :n] = 1.0
        text_rows[b] = b * S + np.arange(T)
    return dict(code=code, text_len=tl, nobj=no, text_rows=text_rows, obj_rows=obj_rows, attn_mask=attn)


@pytest.mark.parametrize("case", ["small", "chunks"])
def test_seq_layout(ops, case):
    """small: B = 3, T = 5, R = 2, ragged, sample 1 without objects, one pad position.  chunks: T = 130 and R = 70 (three and two
    64-entry chunks per wave, masks with holes), S with trailing pads.  code, text_len, nobj, text_rows, obj_rows and the attention
    mask are compared exactly."""
    if case == "small":
        tm = np.array([[1, 1, 1, 1, 1], [1, 1, 1, 0, 0], [1, 0, 1, 1, 0]], dtype=bool)
        om = np.array([[1, 1], [0, 0], [0, 1]], dtype=bool)
        S = 5 + 2 + 1 + 1
    else:
        g = np.random.RandomState(5)
        tm, om = g.rand(2, 130) < 0.7, g.rand(2, 70) < 0.6
        tm[0], om[0] = True, True
        S = 130 + 70 + 1 + 3
    ref = _layout_statement(tm, om, S)
    got = ops.seq_layout(torch.from_numpy(tm).to(dev()), torch.from_numpy(om).to(dev()), S)
    torch.cuda.synchronize()
    for k, v in ref.items():
        assert np.array_equal(got[k].cpu().numpy(), v), k


# ------------------------------------------------------------------------------------------------------ obj_prep
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_obj_prep_statement_and_dropout_pattern(ops, p):
    """B = 2, R = 3 with a padded box (x1 = -2 -> zero row) and a masked region (mvrc_ops == 1 -> the mask embedding in the feature
    half).  Coordinate half (sin | cos of pos / 1000^(j/256) per coordinate) and feature half against the float64 statement within
    the bar of tests/test_ops_gpu.py::test_obj_prep (4e-3 + 4e-3 max|ref|), each half reported on its own.  With dropout the
    statement is multiplied by keep(row * 4096 + e) x scale, and the zero pattern must be vlb_keep's: every dropped element is
    exactly zero, every kept element whose reference is not tiny is non-zero."""
    B, Rr = 2, 3
    g = torch.Generator().manual_seed(11)
    boxes = torch.zeros(B, Rr, 4 + 2048)
    x1, y1 = torch.rand(B, Rr, generator=g) * 300, torch.rand(B, Rr, generator=g) * 200
    boxes[..., 0], boxes[..., 1] = x1, y1
    boxes[..., 2], boxes[..., 3] = x1 + 5 + torch.rand(B, Rr, generator=g) * 200, y1 + 5 + torch.rand(B, Rr, generator=g) * 150
    boxes[..., 4:] = torch.rand(B, Rr, 2048, generator=g)
    boxes[1, 2, :4] = torch.tensor([-2.0, -2.0, -2.0, -2.0])                # padding
    im_info = torch.tensor([[640.0, 480.0, 1.0, 1.0, 0.0], [500.0, 375.0, 1.0, 1.0, 0.0]])
    mvrc_ops = torch.zeros(B, Rr, dtype=torch.int64)
    mvrc_ops[0, 1] = 1
    mask_emb = torch.rand(2048, generator=g) - 0.5
    seedv, tag = 4321, TAG_DOWNSAMPLE
    out = torch.full((B * Rr, 4096), SENT, dtype=act_dtype(), device=dev())
    ops.obj_prep_fwd(boxes.to(dev()), im_info.to(dev()), mvrc_ops.to(dev()), mask_emb.to(dev()), out, drop_p=p, seed=_seed(seedv), tag=tag)
    torch.cuda.synchronize()
    bx = boxes[..., :4].double()
    W, Hh = im_info[:, 0].double()[:, None], im_info[:, 1].double()[:, None]
    pos = torch.stack(((bx[..., 0] + bx[..., 2]) / 2 / W * 100, (bx[..., 1] + bx[..., 3]) / 2 / Hh * 100,
                       (bx[..., 2] - bx[..., 0]) / W * 100, (bx[..., 3] - bx[..., 1]) / Hh * 100), -1)            # [B, R, 4]
    dim = 1000.0 ** (torch.arange(256, dtype=torch.float64) / 256.0)
    ang = pos[..., None] / dim                                                                                      # [B, R, 4, 256]
    coord = torch.cat((torch.sin(ang), torch.cos(ang)), -1).reshape(B * Rr, 2048)
    feats = boxes[..., 4:].double().clone()
    feats[mvrc_ops == 1] = mask_emb.double()
    ref = torch.cat((coord, feats.reshape(B * Rr, 2048)), -1)
    valid = (boxes[..., 0] > -1.5).reshape(B * Rr, 1)
    ref = ref * valid
    thr = drop_thr(p)
    keep = np.ones((B * Rr, 4096), dtype=bool)
    if thr:
        idx = np.arange(B * Rr, dtype=np.int64)[:, None] * 4096 + np.arange(4096)[None, :]
        keep = keep_mask(seedv, tag, idx.reshape(-1), thr).reshape(B * Rr, 4096)
        ref = ref * torch.from_numpy(keep.astype(np.float64)) * drop_scale(thr)
    report("obj_prep coordinate half p=%.1f" % p, out[:, :2048], ref[:, :2048], 4e-3, 4e-3)
    report("obj_prep feature half p=%.1f" % p, out[:, 2048:], ref[:, 2048:], 4e-3, 4e-3)
    o = out.float().cpu()
    assert bool((o[5] == 0).all()), "the padded box's row must be zero"
    if thr:
        keep_t = torch.from_numpy(keep)
        assert bool((o[~keep_t] == 0).all()), "a dropped element is not zero"
        big = keep_t & (ref.abs() > 2e-2) & valid
        assert int(big.sum()) > 0.8 * 5 * 4096 * 0.9 * 0.9 and bool((o[big] != 0).all()), "a kept element is zero"
        assert 0.05 < float((~keep_t).float().mean()) < 0.15


# ------------------------------------------------------------------------------------------------------ masked_colsum
@pytest.mark.parametrize("rows,C,lds,off,which,p", [
    (5, 24, 40, 0, "none", 0.0), (9, 24, 40, 0, "all", 0.1),               # C = 24, lds = 40: three live lanes of one column group
    (5, 2048, 4096, 0, "none", 0.1), (9, 2048, 4096, 0, "all", 0.0),       # the benched width: four column groups of 512
    (9, 2048, 4096, 0, "all", 0.1),
    (9, 20, 40, 0, "all", 0.1),                                            # C % 8 != 0: scalar form
    (70, 16, 24, 1, "mix", 0.1),                                           # C and lds multiples of 8, rows not 16-byte aligned: scalar form
    (300, 1024, 1032, 0, "mix", 0.1),                                      # five 64-row chunks: a second workgroup row, two column groups
])
def test_masked_colsum_forms(ops, rows, C, lds, off, which, p):
    """dst[c] += sum over rows with sel == 1 of src[r][c] * mask(r * 4096 + 2048 + c) against the float64 statement (bar of
    tests/test_embed_attn_ops_gpu.py::test_masked_colsum); with no row selected dst keeps its bits; the floats behind dst stay."""
    g = torch.Generator().manual_seed(rows * 7 + C)
    src = R.rounder(act_dtype())(torch.randn(rows, lds, generator=g))
    if which == "none":
        sel = torch.tensor([0, 2, -1, 0, 3])[:rows]
    elif which == "all":
        sel = torch.ones(rows, dtype=torch.int64)
    else:
        sel = torch.tensor([1, 0, 1, 2, -1, 0, 0])[torch.randint(0, 7, (rows,), generator=g)]
        sel[rows - 1] = 1
    base = torch.randn(C + 8, generator=g)
    dst = base.clone().to(dev())
    seedv, tag = 991, TAG_DOWNSAMPLE
    thr = drop_thr(p)
    w = (sel == 1).double()[:, None].expand(rows, C)
    if thr:
        idx = np.arange(rows, dtype=np.int64)[:, None] * 4096 + 2048 + np.arange(C)[None, :]
        w = w * torch.from_numpy(keep_mask(seedv, tag, idx.reshape(-1), thr).reshape(rows, C).astype(np.float64)) * drop_scale(thr)
    ref = (src[:, off:off + C].double() * w).sum(0)
    ops.masked_colsum(to_gpu_bf16(src)[:, off:off + C], sel.to(dev()), dst[:C], drop_p=p, seed=_seed(seedv), tag=tag, row_elems=4096,
                      col_off=2048)
    torch.cuda.synchronize()
    if which == "none":
        assert torch.equal(dst.cpu(), base)
    report("masked_colsum rows=%d C=%d lds=%d %s p=%.1f" % (rows, C, lds, which, p), dst[:C].double().cpu() - base[:C].double(), ref,
           *R.FP32_GRAD_TOL)
    assert torch.equal(dst[C:].cpu(), base[C:])


# ------------------------------------------------------------------------------------------------------ soft_valid
def _lane_order_sum(t):
    """fp32 sum of a row the way soft_valid_kernel adds it: lane l takes t[l], t[l + 64], ... in ascending order, then the 64 lane
    sums meet in wave_sum's butterfly (v += v[lane ^ o] for o = 32, 16, ..., 1); lane 0's value."""
    C = t.shape[0]
    v = np.zeros(64, dtype=np.float32)
    for c0 in range(0, C, 64):
        chunk = t[c0:c0 + 64]
        v[:chunk.shape[0]] = v[:chunk.shape[0]] + chunk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[lanes ^ o]).astype(np.float32)
    return v[0]


@pytest.mark.parametrize("C", [1601, 7])
def test_soft_valid_sum_order_and_count(ops, C):
    """rows = 5: target rows that sum to 0, 1 (a softmax), 1.2, 1 again with a different spread, and 0.95.  tsum must carry the bits of
    the fp32 sum taken in the kernel's order; the valid count is the number of rows with |tsum - 1| < 0.1 in fp32."""
    rows = 5
    g = torch.Generator().manual_seed(C)
    sm = lambda: torch.softmax(torch.randn(C, generator=g) * 2, -1)
    t = torch.stack((torch.zeros(C), sm(), sm() * 1.2, sm(), sm() * 0.95)).float().contiguous()
    ld = (C + 7) // 8 * 8
    logits = torch.zeros((rows, ld), dtype=act_dtype(), device=dev())
    logits[:, :C] = to_gpu_bf16(torch.randn(rows, C, generator=g))
    tsum = torch.full((rows,), SENT, device=dev())
    counts, lo = torch.full((1,), SENT, device=dev()), torch.zeros(1, device=dev())
    ops.soft_ce_fwd_bwd(logits, C, t.to(dev()), tsum, counts, lo)
    torch.cuda.synchronize()
    exp = np.array([_lane_order_sum(t[r].numpy()) for r in range(rows)], dtype=np.float32)
    got = tsum.cpu().numpy()
    print("soft_valid C=%d tsum %s expected %s" % (C, got.tolist(), exp.tolist()))
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    valid = np.abs(exp - np.float32(1.0)) < np.float32(0.1)
    assert valid.tolist() == [False, True, False, True, True]
    assert float(counts) == float(valid.sum())
    assert bool((logits[~torch.from_numpy(valid)].float() == 0).all())      # invalid rows: zero gradient rows


# ------------------------------------------------------------------------------------------------------ mlm_compact
@pytest.mark.parametrize("n,rate,n_split,capmode", [
    (1, 0.0, 0, "above"), (1, 1.0, 1, "exact"),
    (1025, 0.0, 513, "above"), (1025, 1.0, 513, "below"), (1025, 1.0, 1025, "exact"),
    (16384, 0.0, 9000, "above"), (16384, 1.0, 9000, "below"), (16384, 1.0, 16384, "exact"), (16384, 0.15, 9000, "below"),
    (16384, 0.15, 9000, "above"),
    (16385, 1.0, 16384, "exact"), (16385, 0.15, 16385, "below"), (40000, 0.15, 16390, "above"),      # a second tile of 16384 positions
])
def test_mlm_compact_sizes(ops, n, rate, n_split, capmode):
    """n = 1, 1025 and 16384 (the benched size: exactly one tile of the kernel) at rate 0 and 1, with a cap below the count (overflow
    flag set, the first cap entries right, counts clipped), plus sizes that start a second tile.  Everything is compared exactly
    against embed_attn_refs.mlm_compact_ref; memory behind cap stays."""
    V = 30522
    d = dev()
    labels, src = R.mlm_case(n, rate, n_split, V, seed=n + n_split)
    total = int(((labels >= 0) & (labels < V)).sum())
    cap = {"exact": max(total, 1), "below": max(total - 1, 1), "above": total + 1000}[capmode]
    ref = R.mlm_compact_ref(labels, src, n_split, V, cap)
    assert ref["total"] == total and (capmode != "below" or total > cap)
    out = dict(sel_pos=torch.full((cap + 8,), 77, dtype=torch.int32, device=d), sel_src=torch.full((cap + 8,), 77, dtype=torch.int32, device=d),
               labels_c=torch.full((cap + 8,), 77, dtype=torch.int64, device=d), count0=torch.full((1,), 99.0, device=d),
               count1=torch.full((1,), 99.0, device=d), overflow=torch.zeros(1, dtype=torch.int32, device=d))
    ops.mlm_compact(labels.to(d), src.to(d), n_split, V, out["sel_pos"][:cap], out["sel_src"][:cap], out["labels_c"][:cap], out["count0"],
                    out["count1"], out["overflow"])
    torch.cuda.synchronize()
    for k in ("sel_pos", "sel_src", "labels_c"):
        assert torch.equal(out[k][:cap].cpu(), ref[k]), "%s differs (n=%d rate=%.2f split=%d cap=%d total=%d)" % (k, n, rate, n_split, cap, total)
        assert bool((out[k][cap:] == 77).all()), "%s: written behind cap" % k
    for k in ("count0", "count1", "overflow"):
        assert torch.equal(out[k].cpu(), ref[k]), "%s differs (n=%d rate=%.2f split=%d cap=%d total=%d)" % (k, n, rate, n_split, cap, total)


# ------------------------------------------------------------------------------------------------------ LayerNorm finalize
def _finalize_statement(ws, nslab, LW, H, cpl_log2, by):
    """Column sums of workgroup row `by` of ln_param_finalize_batch_kernel in fp32, in its order: thread ty adds the partial vectors
    by * 4 + ty, + 32, + 64, ... ascending; the four threads of an element meet as (p0 + p1) + (p2 + p3).  -> (dgamma[H], dbeta[H])."""
    part = np.zeros((4, 2 * LW), dtype=np.float32)
    for ty in range(4):
        for r in range(by * 4 + ty, nslab, 32):
            part[ty] = part[ty] + ws[r]
    s = ((part[0] + part[1]).astype(np.float32) + (part[2] + part[3]).astype(np.float32)).astype(np.float32)
    q = np.arange(2 * LW)
    r = q % LW
    cpl = 1 << cpl_log2
    col = ((r & 63) + 64 * (r >> (6 + cpl_log2))) * cpl + ((r >> 6) & (cpl - 1))
    dg, db = np.zeros(H, dtype=np.float32), np.zeros(H, dtype=np.float32)
    ok = col < H
    g_sel, b_sel = ok & (q < LW), ok & (q >= LW)
    dg[col[g_sel]] = s[g_sel]
    db[col[b_sel]] = s[b_sel]
    return dg, db


@pytest.mark.parametrize("H,nslab,n", [(768, 768, 1), (768, 33, 25), (128, 768, 25), (128, 33, 1)])
def test_ln_param_finalize_batch_order(ops, H, nslab, n):
    """The batched finalize on n workspaces of nslab partial vectors (4-column backward layout: LW = 256 ceil(H / 256), lane-major).
    The eight workgroup rows of an element add their sums with atomics in no fixed order, so for the bit-for-bit comparison only the
    partial vectors of ONE workgroup row (entry e: row e % 8) are non-zero: the others add exact zeros, and the gradient must then
    equal base + (that row's fp32 sum in the kernel's order) in one rounding.  A second pass with every partial vector random is
    held to the a-priori bound of recursive fp32 summation, nslab 2^-24 sum|x|, against the float64 column sums."""
    lib = pkg("_lib")
    lib.gemm_set_option("ln_bwd4", 1)
    LW, cpl_log2 = 256 * ((H + 255) // 256), 2
    d = dev()
    g = torch.Generator().manual_seed(H + nslab + n)
    for mode in ("one-row", "all"):
        entries, exp = [], []
        for e in range(n):
            ws = torch.randn(nslab, 2 * LW, generator=g)
            if mode == "one-row":
                ws[(torch.arange(nslab) % 32) // 4 != e % 8] = 0
            base_g, base_b = torch.randn(H, generator=g), torch.randn(H, generator=g)
            dgamma, dbeta = base_g.clone().to(d), (base_b.clone().to(d) if e % 5 != 4 else None)      # (a missing dbeta is skipped)
            entries.append((ws.to(d), nslab, dgamma, dbeta))
            exp.append((ws, base_g, base_b))
        ops.ln_param_finalize_batch(entries, H)
        torch.cuda.synchronize()
        for e, ((_, _, dgamma, dbeta), (ws, base_g, base_b)) in enumerate(zip(entries, exp)):
            if mode == "one-row":
                dg, db = _finalize_statement(ws.numpy(), nslab, LW, H, cpl_log2, e % 8)
                assert np.array_equal((base_g.numpy() + dg).view(np.uint32), dgamma.cpu().numpy().view(np.uint32)), "dgamma of entry %d" % e
                if dbeta is not None:
                    assert np.array_equal((base_b.numpy() + db).view(np.uint32), dbeta.cpu().numpy().view(np.uint32)), "dbeta of entry %d" % e
            else:
                q = np.arange(2 * LW)
                r = q % LW
                col = ((r & 63) + 64 * (r >> 8)) * 4 + ((r >> 6) & 3)
                w64 = ws.double().numpy()
                for name, got, base, sel in (("dgamma", dgamma, base_g, (q < LW) & (col < H)), ("dbeta", dbeta, base_b, (q >= LW) & (col < H))):
                    if got is None:
                        continue
                    ref, bound = np.zeros(H), np.zeros(H)
                    ref[col[sel]] = w64[:, sel].sum(0)
                    bound[col[sel]] = np.abs(w64[:, sel]).sum(0)
                    ref += base.double().numpy()
                    bound = (nslab + 8) * 2.0 ** -24 * (bound + np.abs(base.double().numpy()))
                    err = np.abs(got.double().cpu().numpy() - ref)
                    assert bool((err <= bound).all()), "%s of entry %d: max err %.3e over bound by %.3e" % (name, e, err.max(), (err - bound).max())
