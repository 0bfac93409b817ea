"""Per-kernel parity (-m gpu) of the kernels AROUND the GEMMs, in the forms the training step runs them: the embedding forward /
backward (embed.hip), MLM compaction + compact cross-entropy + row scatter (loss.hip, embed.hip), the small element-wise kernels,
and the attention edges (attention.hip).

Reference for everything: a plain float64 CPU statement of the operation (tests/embed_attn_refs.py) on the same 16-bit-rounded
inputs, gradients by autograd; dropout masks from gpu_util.keep_mask.  tests/test_embed_attn_refs_cpu.py shows on the CPU that a
wrong statement (type row folded, table rows swapped, position not clamped, object position s, unstable compaction, split off by
one, prefix mask in place of a holed one, key stride rounded to 32) misses these bars by >= 10x.

Bars (derived in the header of tests/test_ops_gpu.py): 16-bit outputs 1e-3 + 1e-2 max|ref|; the embedding's fp32 gradient outputs
2e-3 + 1e-2 max|ref|; attention lse 2e-3 + 1e-3, ctx 2e-3 + 1e-2, gradients 2e-3 + 2e-2 -- where max|ref| is taken over the
SUB-TENSOR being reported (a d_type row, a group of d_pos rows, a table row, the masked positions of attention), so that a large
destination does not hide a small one.  The file runs unchanged on the fp16 build (VLB_PRECISION=f16).
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import embed_attn_refs as R
from tests.gpu_util import TAG_EMBED, act_dtype, dev, drop_scale, drop_thr, keep_mask, pkg, report, to_gpu_bf16

pytestmark = pytest.mark.gpu
SENT = 7.25          # sentinel for memory a kernel must not touch (or must overwrite)


@pytest.fixture(scope="module")
def ops():
    o = pkg("ops")
    name, cus = pkg("_lib").device_info(0)
    assert name.startswith("gfx950"), "these kernels are built for gfx950 only (got %s)" % name
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return R.rounder(act_dtype())(torch.randn(*shape, generator=g) * scale)


def a16(*shape, fill=0.0):
    return torch.full(shape, fill, dtype=act_dtype(), device=dev())


# ------------------------------------------------------------------------------------------------------ A. embedding
def _embed_bwd_call(ops, c, lay, dev_in, pre, stats, zeroed, seed):
    """One backward on top of non-zero contents.  Returns (gradient dict with the base subtracted, raw buffers, base buffers)."""
    d = dev()
    B, T, Rr, S, H, V, P = (c[k] for k in ("B", "T", "R", "S", "H", "V", "P"))
    g = torch.Generator().manual_seed(77)
    base = {k: torch.randn(*s, generator=g).to(d) for k, s in
            (("word", (V, H)), ("pos", (P, H)), ("type", (3, H)), ("end", (1, H)), ("gamma", (H,)), ("beta", (H,)), ("table", (2, H)))}
    buf = {k: v.clone() for k, v in base.items()}
    buf["obj_vis"] = torch.full((B * Rr, H), SENT, device=d)
    pretrain = c["mode"] == "pretrain"
    if pretrain:
        buf["text_vis"] = torch.zeros((B, H), device=d) if zeroed else torch.full((B, H), SENT, device=d)
        dtv, d_ol, dol, sel = (H, 0), buf["table"], (0, 0), dev_in["sel"]
    else:
        buf["text_vis"] = torch.full((B * T, H), SENT, device=d)
        buf["obj_ling"] = torch.full((B * Rr, H), SENT, device=d)
        dtv, d_ol, dol, sel = (T * H, H), buf["obj_ling"], (Rr * H, H), None
    ops.embed_bwd(dev_in["dy"], pre, stats, dev_in["gamma"], lay, dev_in["ids"], dev_in["types"], sel, buf["word"], buf["pos"],
                  buf["type"], buf["end"], buf["gamma"], buf["beta"], buf["text_vis"], dtv, buf["obj_vis"], (Rr * H, H), d_ol, dol,
                  B, T, Rr, S, H, drop_p=c["p"], seed=seed, tag=TAG_EMBED, text_vis_zeroed=zeroed)
    torch.cuda.synchronize()
    un = R.embed_untouched(c)
    sub = lambda k: (buf[k].double() - base[k].double()).cpu()           # accumulate semantics: result = base + gradient
    grads = {k: sub(k) for k in ("word", "pos", "type", "end", "gamma", "beta")}
    keep_rows = lambda t, untouched: torch.where(untouched.reshape(-1, 1), torch.zeros((), dtype=torch.float64), t.double().cpu())
    grads["obj_vis"] = keep_rows(buf["obj_vis"], un["obj"]).reshape(B, Rr, H)
    if pretrain:
        grads["text_vis"] = buf["text_vis"].double().cpu()
        grads["obj_ling"] = sub("table")
    else:
        grads["text_vis"] = keep_rows(buf["text_vis"], un["text"]).reshape(B, T, H)
        grads["obj_ling"] = keep_rows(buf["obj_ling"], un["obj"]).reshape(B, Rr, H)
    return grads, buf, base


@pytest.mark.parametrize("name", list(R.EMBED_CASES))
def test_embedding_fwd_bwd_forms(ops, name):
    """embed_fwd / embed_bwd in the two forms the engine calls them (R.EMBED_CASES says which case covers which H / B / dropout /
    edge): forward pre, out, stats; every backward result, the small destinations on their own scale; untouched rows bit for bit;
    accumulation on top of non-zero contents; the broadcast d_text_vis written (sentinel overwritten) or added to zeroed memory."""
    c = R.embed_case(name, act_dtype())
    d = dev()
    B, T, Rr, S, H, V, P = (c[k] for k in ("B", "T", "R", "S", "H", "V", "P"))
    pretrain = c["mode"] == "pretrain"
    fwd_ref, g_ref = R.embed_ref(c)
    lay = ops.seq_layout(c["text_mask"].to(d), c["obj_mask"].to(d), S)
    code = lay["code"].cpu().long()
    assert torch.equal(code >> 16, c["kind"])
    named = (c["kind"] == R.KIND_TEXT) | (c["kind"] == R.KIND_OBJ)
    assert torch.equal((code & 0xffff)[named], c["idx"][named])
    assert torch.equal(lay["text_len"].cpu().long(), c["tl"]) and torch.equal(lay["nobj"].cpu().long(), c["no"])
    seed = torch.tensor([R.EMBED_SEED], dtype=torch.int32, device=d)
    dev_in = dict(ids=c["text_ids"].to(d), types=None if pretrain else c["text_type"].to(d), gamma=c["gamma"].to(d),
                  dy=to_gpu_bf16(c["dy"].reshape(B * S, H)), sel=None)
    obj_vis = to_gpu_bf16(c["obj_vis"].reshape(B * Rr, H))
    if pretrain:
        tv, tvs, ol, ols = to_gpu_bf16(c["text_vis"]), (H, 0), to_gpu_bf16(c["obj_ling"]), (0, 0)
        dev_in["sel"] = c["ling_idx"].to(d)
    else:       # dense linguistic rows read through a strided view of the [B*R, 2H] object embedding buffer
        ovl = to_gpu_bf16(torch.cat((torch.full((B * Rr, H), SENT), c["obj_ling"].reshape(B * Rr, H)), 1))
        tv, tvs, ol, ols = to_gpu_bf16(c["text_vis"].reshape(B * T, H)), (T * H, H), ovl[:, H:], (Rr * 2 * H, 2 * H)
    pre, out = a16(B * S, H, fill=SENT), a16(B * S, H, fill=SENT)
    stats = torch.full((B * S, 2), SENT, device=d)
    ops.embed_fwd(lay, dev_in["ids"], dev_in["types"], to_gpu_bf16(c["word"]), to_gpu_bf16(c["pos"]), to_gpu_bf16(c["type"]),
                  to_gpu_bf16(c["end"]), tv, tvs, obj_vis, (Rr * H, H), ol, ols, dev_in["sel"], dev_in["gamma"], c["beta"].to(d),
                  pre, stats, out, B, T, Rr, S, H, drop_p=c["p"], seed=seed, tag=TAG_EMBED)
    tag = "embed %s " % name
    report(tag + "fwd pre", pre.view(B, S, H), fwd_ref["pre"], *R.ACT16_TOL)
    report(tag + "fwd out", out.view(B, S, H), fwd_ref["out"], *R.ACT16_TOL)
    report(tag + "fwd stats mean", stats[:, 0], fwd_ref["mean"], *R.FP32_GRAD_TOL)
    report(tag + "fwd stats rstd", stats[:, 1], fwd_ref["rstd"], *R.FP32_GRAD_TOL)
    if c["keep"] is not None:      # the dropped elements are exactly the mask's
        o = out.view(B, S, H).float().cpu()
        assert bool((o[c["keep"] == 0] == 0).all()) and bool((o[(c["keep"] != 0) & (fwd_ref["out"].abs() > 0.05)] != 0).all())

    grads, buf, base = _embed_bwd_call(ops, c, lay, dev_in, pre, stats, c["zeroed"], seed)
    got, ref = R.embed_parts(c, grads), R.embed_parts(c, g_ref)
    assert got.keys() == ref.keys()
    for nm in ref:
        report(tag + "bwd " + nm, got[nm], ref[nm], *R.FP32_GRAD_TOL)
    # untouched memory, bit for bit
    un = R.embed_untouched(c)
    eq = lambda k, rows: torch.equal(buf[k].cpu()[rows], base[k].cpu()[rows])
    assert eq("word", un["word"]), "d_word rows of unused vocabulary ids were written"
    assert eq("pos", un["pos"]), "d_pos rows that no sample reaches were written"
    assert bool((buf["obj_vis"].cpu()[un["obj"].reshape(-1)] == SENT).all()), "d_obj_vis rows of padded boxes were written"
    assert bool((buf["obj_vis"].cpu()[~un["obj"].reshape(-1)] != SENT).all())
    if pretrain:
        assert eq("type", [1]), "d_type row 1 without a type-1 token"
        sel = set(c["ling_idx"][c["obj_mask"]].tolist())
        for row in (0, 1):
            if row not in sel:
                assert eq("table", [row]), "linguistic table row %d gradient must be exactly zero" % row
        assert bool((buf["text_vis"] != SENT).all()), "the per-sample text-visual sum must overwrite"
        # the other way of producing the per-sample sum gives the same values
        grads2, buf2, _ = _embed_bwd_call(ops, c, lay, dev_in, pre, stats, not c["zeroed"], seed)
        report(tag + "bwd d_text_vis (%s)" % ("written" if c["zeroed"] else "added to zeroed memory"), grads2["text_vis"],
               g_ref["text_vis"], *R.FP32_GRAD_TOL)
        report(tag + "bwd d_text_vis written vs added", buf2["text_vis"], buf["text_vis"].cpu(), 1e-4, 1e-4)
    else:
        assert bool((buf["obj_ling"].cpu()[un["obj"].reshape(-1)] == SENT).all()), "dense d_obj_ling rows of padded boxes were written"
        assert bool((buf["text_vis"].cpu()[un["text"].reshape(-1)] == SENT).all()), "d_text_vis rows of padded tokens were written"
        assert bool((buf["text_vis"].cpu()[~un["text"].reshape(-1)] != SENT).all())


# ------------------------------------------------------------------------------------------------------ B. MLM compaction
def _compact(ops, labels, src, n_split, V, cap):
    d = dev()
    out = dict(sel_pos=torch.full((cap,), 99, dtype=torch.int32, device=d), sel_src=torch.full((cap,), 99, dtype=torch.int32, device=d),
               labels_c=torch.full((cap,), 99, dtype=torch.int64, device=d), count0=torch.full((1,), 99.0, device=d),
               count1=torch.full((1,), 99.0, device=d), overflow=torch.zeros(1, dtype=torch.int32, device=d))
    ops.mlm_compact(labels.to(d), src.to(d), n_split, V, out["sel_pos"], out["sel_src"], out["labels_c"], out["count0"], out["count1"],
                    out["overflow"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,rate,n_split,capmode", [
    (1, 1.0, 0, "exact"), (1, 1.0, 1, "above"), (1, 0.0, 0, "above"),
    (640, 0.15, 300, "above"), (640, 0.15, 0, "exact"), (640, 0.0, 640, "above"),
    (1024, 1.0, 1024, "exact"), (1024, 0.15, 511, "below"),
    (1025, 0.15, 513, "below"), (1025, 1.0, 513, "above"),                        # two positions per thread, split inside a run
    (25600, 0.15, 12345, "above"), (25600, 0.15, 12345, "exact"), (25600, 0.15, 12345, "below"), (25600, 1.0, 12345, "exact"),
    (65537, 0.15, 40000, "exact"), (65537, 0.15, 65537, "below"), (65537, 1.0, 0, "above"), (65537, 0.0, 40000, "above"),
])
def test_mlm_compact(ops, n, rate, n_split, capmode):
    """The block scan that decides which rows are trained on, against the stable ascending list of positions with 0 <= label < V
    (labels -1, -7, V, V + 1000 are ignored; src_rows holds -1 entries).  cap = the count, one below it (overflow flag, first cap
    entries right, counts clipped to the kept entries) and far above it (tail filled with -1).  Everything is compared exactly."""
    V = 30522
    labels, src = R.mlm_case(n, rate, n_split, V, seed=n + n_split)
    total = int(((labels >= 0) & (labels < V)).sum())
    cap = {"exact": max(total, 1), "below": max(total - 1, 1), "above": total + 1000}[capmode]
    ref = R.mlm_compact_ref(labels, src, n_split, V, cap)
    assert ref["total"] == total and (capmode != "below" or total > cap)
    got = _compact(ops, labels, src, n_split, V, cap)
    for k in ("sel_pos", "sel_src", "labels_c", "count0", "count1", "overflow"):
        assert torch.equal(got[k].cpu(), ref[k]), "%s differs (n=%d rate=%.2f split=%d cap=%d total=%d)" % (k, n, rate, n_split, cap, total)


@pytest.mark.parametrize("n_split", [300, 640, 0])
def test_ce_compact_and_row_round_trip(ops, n_split):
    """ce_fwd_bwd_compact on mlm_compact's output (V = 30522, ld = 30528): both group losses and d(logits) against float64
    F.cross_entropy per group with its own mean; rows past the count: zero gradient; pad columns zero.  gather_rows -> scatter_rows
    through sel_src / sel_pos is exact and leaves rows that no index names alone."""
    d = dev()
    n, V, ld, cap, H = 640, 30522, 30528, 128, 768
    labels, src = R.mlm_case(n, 0.15, n_split, V, seed=5)
    ref = R.mlm_compact_ref(labels, src, n_split, V, cap)
    total, n0 = ref["total"], int(ref["count0"])
    assert 0 < total < cap - 8
    got = _compact(ops, labels, src, n_split, V, cap)
    x = rnd(cap, V, seed=40, scale=2.0)
    xr = x[:total].double().clone().requires_grad_(True)
    lab_c = ref["labels_c"][:total]
    losses = [F.cross_entropy(xr[a:b], lab_c[a:b]) if b > a else xr.sum() * 0 for a, b in ((0, n0), (n0, total))]
    (losses[0] + losses[1]).backward()
    buf = a16(cap, ld, fill=7.0)
    buf[:, :V] = to_gpu_bf16(x)
    l0, l1 = torch.zeros(1, device=d), torch.zeros(1, device=d)
    ops.ce_fwd_bwd_compact(buf, V, got["labels_c"], got["count0"], got["count1"], l0, l1)
    tag = "ce compact split=%d " % n_split
    report(tag + "loss group 0", l0, losses[0].detach().reshape(1), 1e-4, 1e-3)
    report(tag + "loss group 1", l1, losses[1].detach().reshape(1), 1e-4, 1e-3)
    if n0:
        report(tag + "dlogits group 0", buf[:n0, :V], xr.grad[:n0], 1e-5, 1e-2)
    if total > n0:
        report(tag + "dlogits group 1", buf[n0:total, :V], xr.grad[n0:], 1e-5, 1e-2)
    assert float(buf[total:].float().abs().max()) == 0.0, "rows past the count must get a zero gradient"
    assert float(buf[:, V:].float().abs().max()) == 0.0, "pad columns must be zero"
    # gather -> scatter round trip
    rows = rnd(n, H, seed=41)
    packed = a16(cap, H, fill=SENT)
    ops.gather_rows(to_gpu_bf16(rows), got["sel_src"], packed)
    exp_packed = torch.zeros(cap, H)
    ss = ref["sel_src"][:total].long()
    exp_packed[:total] = torch.where((ss >= 0)[:, None], rows[ss.clamp(min=0)], torch.zeros(()))
    assert torch.equal(packed.float().cpu(), exp_packed)
    dst = a16(n, H, fill=SENT)
    ops.scatter_rows(packed, got["sel_pos"], dst)
    exp = torch.full((n, H), SENT)
    exp[ref["sel_pos"][:total].long()] = exp_packed[:total]
    assert torch.equal(dst.float().cpu(), exp)


# ------------------------------------------------------------------------------------------------------ C. small kernels
@pytest.mark.parametrize("n", [4, 1020, 1024, 1028, 4 * 1024 * 3 + 4])
def test_dgelu_mul_and_tanh_bwd(ops, n):
    """out = dg * gelu'(u) (erf GELU) and out = dy * (1 - y^2) against float64 formulas; a sentinel behind the output stays."""
    dg, u = rnd(n, seed=1), rnd(n, seed=2, scale=2.0)
    out = a16(n + 8, fill=SENT)
    ops.dgelu_mul(to_gpu_bf16(dg), to_gpu_bf16(u), out[:n])
    ud = u.double()
    ref = dg.double() * (0.5 * (1 + torch.erf(ud / np.sqrt(2.0))) + ud * torch.exp(-0.5 * ud * ud) / np.sqrt(2 * np.pi))
    report("dgelu_mul n=%d" % n, out[:n], ref, *R.ACT16_TOL)
    assert bool((out[n:].float() == SENT).all())
    y = torch.tanh(rnd(n, seed=3, scale=1.5))
    y = R.rounder(act_dtype())(y)
    out = a16(n + 8, fill=SENT)
    ops.tanh_bwd(to_gpu_bf16(dg), to_gpu_bf16(y), out[:n])
    report("tanh_bwd n=%d" % n, out[:n], dg.double() * (1 - y.double() ** 2), *R.ACT16_TOL)
    assert bool((out[n:].float() == SENT).all())


def test_small_kernel_abi_rejections(ops):
    x, o = a16(16), a16(16)
    with pytest.raises(RuntimeError, match="vlb_dgelu_mul: n must be a multiple of 4"):
        ops.dgelu_mul(x[:6], x[:6], o[:6])
    with pytest.raises(RuntimeError, match="vlb_tanh_bwd: n must be a multiple of 4"):
        ops.tanh_bwd(x[:6], x[:6], o[:6])
    idx = torch.zeros(2, dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError, match="vlb_scatter_rows: bad argument"):
        ops.scatter_rows(a16(2, 12), idx, a16(2, 12))
    with pytest.raises(RuntimeError, match="vlb_gather_rows: H must be a multiple of 8"):
        ops.gather_rows(a16(2, 12), idx, a16(2, 12))
    boxes = torch.zeros((1, 2, 6), device=dev())
    with pytest.raises(RuntimeError, match="vlb_zero_padded_rows_bf16: bad argument"):
        ops.zero_padded_rows(a16(2, 16)[:, :12], boxes)


@pytest.mark.parametrize("H,ld", [(8, 8), (72, 96), (768, 1024)])
def test_zero_padded_rows(ops, H, ld):
    """rows of padded boxes (x1 <= -1.5) become zero in their first H columns -- box 0 of a sample included --; every other element
    of the strided buffer stays bit-identical."""
    B, Rr = 3, 7
    g = torch.Generator().manual_seed(H)
    boxes = torch.rand(B, Rr, 6, generator=g) * 10
    padded = torch.rand(B, Rr, generator=g) < 0.4
    padded[1, 0], padded[0, 0], padded[2, Rr - 1] = True, False, True
    boxes[..., 0] = torch.where(padded, torch.tensor(-2.0), boxes[..., 0])
    boxes[0, 1, 0] = -1.0                                   # a valid box left of the image origin is not padding
    padded[0, 1] = False
    x = rnd(B * Rr, ld, seed=9) + 3.0
    xg = to_gpu_bf16(x)
    before = xg.clone()
    ops.zero_padded_rows(xg[:, :H], boxes.to(dev()))
    exp = before.clone().cpu()
    exp[padded.reshape(-1), :H] = 0
    assert torch.equal(xg.cpu(), exp)


@pytest.mark.parametrize("rows,C,lds,p", [(5, 300, 304, 0.0), (5, 300, 304, 0.1), (1000, 300, 304, 0.1), (1000, 2048, 2048, 0.0),
                                          (63, 256, 512, 0.1), (1, 8, 8, 0.0)])
def test_masked_colsum(ops, rows, C, lds, p):
    """dst[c] += sum over rows with sel == 1 of src[r][c] * mask(r * 4096 + 2048 + c), on top of existing contents; sel values
    other than 1 (0, 2, -1) do not count."""
    g = torch.Generator().manual_seed(rows + C)
    src = rnd(rows, lds, seed=rows)
    sel = torch.tensor([1, 0, 1, 2, -1, 1, 1])[torch.randint(0, 7, (rows,), generator=g)]
    sel[0] = 1
    base = torch.randn(C + 8, generator=g)
    dst = base.clone().to(dev())
    seedv, tag = 991, 1001
    thr = drop_thr(p)
    w = (sel == 1).double()[:, None].expand(rows, C)
    if thr:
        idx = np.arange(rows, dtype=np.int64)[:, None] * 4096 + 2048 + np.arange(C)[None, :]
        w = w * torch.from_numpy(keep_mask(seedv, tag, idx.reshape(-1), thr).reshape(rows, C).astype(np.float64)) * drop_scale(thr)
    ref = (src[:, :C].double() * w).sum(0)
    ops.masked_colsum(to_gpu_bf16(src)[:, :C], sel.to(dev()), dst[:C], drop_p=p, seed=torch.tensor([seedv], dtype=torch.int32, device=dev()),
                      tag=tag, row_elems=4096, col_off=2048)
    report("masked_colsum rows=%d C=%d p=%.1f" % (rows, C, p), dst[:C].double().cpu() - base[:C].double(), ref, *R.FP32_GRAD_TOL)
    assert torch.equal(dst[C:].cpu(), base[C:])


# ------------------------------------------------------------------------------------------------------ D. attention edges
@pytest.mark.parametrize("B,S,nh,p", [(5, s, 2, 0.0) for s in (1, 2, 16, 17, 31, 32, 33, 64, 96, 97, 127, 130, 255)] +
                         [(8, 101, 12, 0.0), (3, 101, 16, 0.0), (5, 33, 2, 0.1), (5, 130, 2, 0.1), (8, 101, 12, 0.1)])
def test_attention_masks_and_short_sequences(ops, B, S, nh, p):
    """General 0/1 key masks (sample b, b % 5: full | holes | one key only | all zero | prefix of length 1) at short and ragged S,
    12 / 16 heads, dropout with a partial last key block.  lse on every (b, h, q); dq / dk / dv reported separately for live
    positions, masked positions (small in the reference), and the all-zero-mask samples (a plain softmax: -10000 on every score).

    Samples with ONE live key are reported on their own: there d(scores) = P (dP - D) is an exact cancellation, dq = dk = 0 in the
    reference, and with dropout the kernels cannot reproduce the zero for an arithmetic reason -- the saved ctx is 16-bit, so
    D = rowsum(dO * O) carries O's rounding (2^-9 of |dO . V| ~ 8 on bf16) while dP does not.  Their bar is therefore the class bar or,
    where that cannot be met, four times the error of R.attn_rounded_f32 (an fp32 CPU restatement that rounds where the kernels
    round) against the float64 reference on the same inputs, measured in the test and printed.  Measured for dk on the bf16 build:
    4.6e-2 (S = 33), 9.4e-2 (S = 130), 8.8e-2 (S = 101, 12 heads) -> bars 0.19 / 0.38 / 0.35; on the fp16 build 5.3e-3 / 1.0e-2 /
    1.4e-2; without dropout the restatement is exact (P = 1, O = V) and the class bar 2e-3 holds."""
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
    seed = torch.tensor([seedv], dtype=torch.int32, device=dev())
    qg, mg = to_gpu_bf16(qkv), mask.to(dev())
    ctx = a16(B * S, H, fill=SENT)
    lse = torch.full((B, nh, S), SENT, device=dev())
    ops.attention_fwd(qg, mg, ctx, lse, B, S, H, nh, drop_p=p, seed=seed, tag=tag)
    dqkv = a16(B * S, 3 * H, fill=SENT)
    ops.attention_bwd(qg, mg, ctx, lse, to_gpu_bf16(dctx), dqkv, B, S, H, nh, drop_p=p, seed=seed, tag=tag)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ctx.float()).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(dqkv.float()).all())
    name = "attn-edge B%d S%d h%d p%.1f " % (B, S, nh, p)
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
