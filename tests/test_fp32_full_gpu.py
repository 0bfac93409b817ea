"""GPU tests of pre-training in full fp32 (`fp32_full`): the kernels of vl-bert_amd/csrc/f32_pretrain.hip against float64 references
(tests/fp32_full_ref.py), the fp32 front end of vl-bert_amd/pretrain_f32.py, then the engine against the oracle beside the hybrid
(`encoder_fp32` alone), two optimizer steps, bit-identical results on the two builds of the library, the module mirror and the entry point.

Bars: 1e-6 relative for a row kernel's forward value (a loss), 1e-5 relative Frobenius for its gradient, 2e-5 for anything through the
split-operand GEMM (the bars tests/test_f32_encoder_gpu.py and tests/test_fp32_ends_gpu.py hold the fp32 kernels to); 1e-3, the project's
fp32 tolerance, for the engine, and 5x below the hybrid on the bf16 build."""
import math
import os
import subprocess
import sys

if __name__ == "__main__":          # the child of test_no_16bit_rounding_left_in_the_step
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import torch

from oracle import vlbert_oracle as O
from tests import fp32_full_ref as RF
from tests.gpu_util import TAG_DOWNSAMPLE, EngineDropoutMasks, dev, device_seed, drop_scale, drop_thr, keep_mask, pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
LD = {2: 4, 5: 8, 37: 40, 1601: 1604, 30522: 30528}      # leading dimensions of the logits: the smallest multiple of 4 (30528: the engine's)


def rel(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def check(name, got, ref, bar):
    e = rel(got, ref)
    print("  %-52s rel-fro %.3e  (bar %.0e)" % (name, e, bar))
    assert e <= bar, (name, e)


def padded(x, ld, fill=3.0):
    """x [rows, V] -> device fp32 [rows, ld] with junk in the pad columns (they must take no part)."""
    out = torch.full((x.shape[0], ld), fill, dtype=F32)
    out[:, :x.shape[1]] = x
    return out.to(dev())


def zf(*s):
    return torch.zeros(s, dtype=F32, device=dev())


# -------------------------------------------------------------------------------------------------------------------------------
# losses
# -------------------------------------------------------------------------------------------------------------------------------
def _run_ce(x, labels, V, gscale, copy):
    ops = pkg("ops")
    lg = padded(x, LD[V])
    cp = torch.full_like(lg, 9.0) if copy else None
    counts, loss = torch.full((1,), 77.0, device=dev()), zf(1)
    ops.ce_f32_fwd_bwd(lg, V, labels.to(dev()), counts, loss, gscale=gscale, logits_copy=cp)
    return lg, cp, float(counts), loss


@pytest.mark.parametrize("V", [2, 37, 30522])
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_ce_f32_fwd_bwd(rows, V):
    g = torch.Generator().manual_seed(100 * rows + V)
    x = torch.randn(rows, V, generator=g) * 3
    x[0] = torch.linspace(-1e4, 1e4, V)[torch.randperm(V, generator=g)]      # a row spanning +-1e4: the maximum must be subtracted
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[torch.rand(rows, generator=g) < 0.4] = -1
    labels[0] = int(x[0].argmin())                                           # the far end of the wide row
    labels[rows - 1] = V - 1                                                 # the last class
    for gscale, copy in ((0.37, True), (1.0, False)):
        ref_loss, ref_grad, n = RF.ce_ref(x, labels, gscale)
        lg, cp, count, loss = _run_ce(x, labels, V, gscale, copy)
        assert count == n and bool(torch.isfinite(lg).all())
        assert abs(float(loss) - float(ref_loss)) <= 1e-6 * abs(float(ref_loss)), (float(loss), float(ref_loss))
        check("ce_f32 d logits (rows %d, V %d, gscale %g)" % (rows, V, gscale), lg[:, :V], ref_grad, 1e-5)
        assert float(lg[:, V:].abs().max()) == 0.0                           # pad columns of the gradient: exactly zero
        if copy:
            assert torch.equal(cp[:, :V].cpu(), x) and float(cp[:, V:].abs().max()) == 0.0
        lg2, _, _, loss2 = _run_ce(x, labels, V, gscale, copy)              # the same inputs twice: the same bits
        assert torch.equal(lg, lg2) and torch.equal(loss, loss2)
    # no labelled row: loss 0, zero gradient, nothing non-finite
    lg, _, count, loss = _run_ce(x, torch.full((rows,), -1), V, 1.0, False)
    assert count == 0 and float(loss) == 0.0 and float(lg.abs().max()) == 0.0
    # exactly one labelled row
    one = torch.full((rows,), -1)
    one[rows // 2] = V // 2
    ref_loss, ref_grad, n = RF.ce_ref(x, one)
    lg, _, count, loss = _run_ce(x, one, V, 1.0, False)
    assert count == 1 and abs(float(loss) - float(ref_loss)) <= 1e-6 * abs(float(ref_loss))
    check("ce_f32 d logits, one labelled row", lg[:, :V], ref_grad, 1e-5)


@pytest.mark.parametrize("rows, V", [(70, 37), (5, 30522)])
@pytest.mark.parametrize("n0, n1", [(0, 3), (3, 0), (2, 2)])
def test_ce_f32_fwd_bwd_compact(n0, n1, rows, V):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(rows + V + 10 * n0 + n1)
    x = torch.randn(rows, V, generator=g) * 2
    labels = torch.full((rows,), -1)
    labels[:n0 + n1] = torch.randint(0, V, (n0 + n1,), generator=g)
    labels[n0 + n1 - 1] = V - 1
    r0, r1, ref_grad = RF.ce_compact_ref(x, labels, n0, n1, gscale=1.5)
    out = []
    for _ in range(2):
        lg, losses = padded(x, LD[V]), zf(4)
        c0, c1 = torch.tensor([float(n0)], device=dev()), torch.tensor([float(n1)], device=dev())
        ops.ce_f32_fwd_bwd_compact(lg, V, labels.to(dev()), c0, c1, losses[0:1], losses[2:3], gscale=1.5)
        out.append((lg, losses))
    lg, losses = out[0]
    assert torch.equal(lg, out[1][0]) and torch.equal(losses, out[1][1])
    for got, ref in ((float(losses[0]), float(r0)), (float(losses[2]), float(r1))):
        assert abs(got - ref) <= 1e-6 * abs(ref) and (ref != 0.0 or got == 0.0), (got, ref)
    check("ce_f32 compact d logits (%d + %d of %d rows, V %d)" % (n0, n1, rows, V), lg[:, :V], ref_grad, 1e-5)
    assert float(lg[:, V:].abs().max()) == 0.0 and float(lg[n0 + n1:].abs().max()) == 0.0 and bool(torch.isfinite(lg).all())


@pytest.mark.parametrize("C", [5, 1601])
@pytest.mark.parametrize("rows", [1, 7])
def test_soft_ce_f32_fwd_bwd(rows, C):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(rows * 7 + C)
    x = torch.randn(rows, C, generator=g) * 3
    t = torch.softmax(torch.randn(rows, C, generator=g) * 2, 1)
    if rows > 1:
        t[1] = 0.0              # invalid: no soft label
        t[4] *= 0.5             # invalid: sums to 0.5
        t[5] *= 1.05            # valid: within 0.1 of one
    for tgt, copy in ((t, True), (t, False), (torch.zeros_like(t), False)):
        ref_loss, ref_grad, tsum_ref, n = RF.soft_ce_ref(x, tgt, gscale=0.8)
        runs = []
        for _ in range(2):
            lg = padded(x, LD[C])
            cp = torch.full_like(lg, 9.0) if copy else None
            tsum, counts, loss = zf(rows), torch.full((1,), 55.0, device=dev()), zf(1)
            ops.soft_ce_f32_fwd_bwd(lg, C, tgt.to(dev()), tsum, counts, loss, gscale=0.8, logits_copy=cp)
            runs.append((lg, loss))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert float(counts) == n and rel(tsum, tsum_ref) <= 1e-6 if n else float(counts) == 0
        assert bool(torch.isfinite(lg).all()) and float(lg[:, C:].abs().max()) == 0.0
        if n == 0:
            assert float(loss) == 0.0 and float(lg.abs().max()) == 0.0
            continue
        assert abs(float(loss) - float(ref_loss)) <= 1e-6 * abs(float(ref_loss)), (float(loss), float(ref_loss))
        check("soft_ce_f32 d logits (rows %d, C %d)" % (rows, C), lg[:, :C], ref_grad, 1e-5)
        if copy:
            assert torch.equal(cp[:, :C].cpu(), x) and float(cp[:, C:].abs().max()) == 0.0
        if rows > 1:
            assert float(lg[1].abs().max()) == 0.0 and float(lg[4].abs().max()) == 0.0


# -------------------------------------------------------------------------------------------------------------------------------
# hand-over and the small reductions
# -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 768])
def test_gather_scatter_combine_f32(H):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(H)
    B, T, R = 3, 7, 5
    S = T + R + 1
    src = torch.randn(B * S, H, generator=g)
    idx = torch.tensor([5, -1, 0, B * S - 1, 17, -1, 9, 2, 30], dtype=torch.int32)
    out = torch.full((9, H), 4.0, device=dev())
    ops.gather_rows_f32(src.to(dev()), idx.to(dev()), out)
    assert torch.equal(out.cpu(), RF.gather_ref(src, idx))
    back = torch.full((B * S, H), -1.0, device=dev())
    ops.scatter_rows_f32(out, idx.to(dev()), back)                          # scatter(gather(x)) restores the selected rows exactly
    want = RF.scatter_ref(RF.gather_ref(src, idx), idx, torch.full((B * S, H), -1.0))
    assert torch.equal(back.cpu(), want) and torch.equal(back.cpu()[idx[idx >= 0].long()], src[idx[idx >= 0].long()])
    text_mask = torch.arange(T)[None, :] < torch.tensor([T, 3, 5])[:, None]
    obj_mask = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 0, 0], [1, 0, 1, 1, 0]], dtype=torch.bool)
    lay = ops.seq_layout(text_mask.to(dev()), obj_mask.to(dev()), S)
    d_text, d_obj = torch.randn(B, T, H, generator=g), torch.randn(B, R, H, generator=g)
    dx = torch.full((B * S, H), 8.0, device=dev())
    ops.head_grad_combine_f32(d_text.to(dev()).view(B * T, H), d_obj.to(dev()).view(B * R, H), lay["code"], dx, B, T, R, S, H)
    assert torch.equal(dx.cpu().view(B, S, H), RF.combine_ref(d_text, d_obj, text_mask, obj_mask, S))


@pytest.mark.parametrize("H", [64, 768])
def test_small_reductions_f32(H):
    """select_rows2 / table2_grad / group_rowsum / add_rows / mask_feature / masked_colsum: odd row counts, more rows than one pass of
    a workgroup's 16 waves takes, selectors outside {0, 1} ignored by the sums."""
    ops = pkg("ops")
    g = torch.Generator().manual_seed(H + 1)
    n = 70
    sel = torch.randint(0, 2, (n,), generator=g)
    table, src = torch.randn(2, H, generator=g), torch.randn(n, H, generator=g)
    out = zf(n, H)
    ops.select_rows2_f32(table.to(dev()), sel.to(dev()), out)
    assert torch.equal(out.cpu(), table[sel])
    dst = torch.ones(2, H, device=dev())
    ops.table2_grad_f32(src.to(dev()), sel.to(dev()), dst)
    ref = torch.stack((src[sel == 0].double().sum(0), src[sel == 1].double().sum(0))) + 1.0
    check("table2_grad_f32", dst, ref, 1e-6)
    for T in (5, 64):
        s = torch.randn(3 * T, H, generator=g)
        d = zf(3, H)
        ops.group_rowsum_f32(s.to(dev()), T, d)
        check("group_rowsum_f32 T=%d" % T, d, s.double().view(3, T, H).sum(1), 1e-6)
    a, b = torch.randn(3, 5 * H, generator=g), torch.randn(3, H, generator=g)
    ag = a.to(dev())
    ops.add_rows_f32(ag[:, :H], b.to(dev()))
    want = a.clone()
    want[:, :H] += b
    assert torch.equal(ag.cpu(), want)
    # mask substitution + the masked column sums through its dropout
    B, R, SEED, p = 7, 10, 4242, 0.1
    boxes = torch.rand(B, R, 4 + 2048, generator=g)
    boxes[2, 5:] = -2.0
    ops_sel = torch.randint(0, 2, (B, R), generator=g)
    emb = torch.randn(2048, generator=g)
    av = torch.randn(B * R, 4096, generator=g)
    ad = av.to(dev())
    seed = torch.tensor([SEED], dtype=torch.int32, device=dev())
    ops.mask_feature_f32(ad, boxes.to(dev()), ops_sel.to(dev()).view(-1), emb.to(dev()), drop_p=p, seed=seed, tag=TAG_DOWNSAMPLE)
    thr = drop_thr(p)
    keep = torch.from_numpy(keep_mask(SEED, TAG_DOWNSAMPLE, np.arange(B * R * 4096), thr).reshape(B * R, 4096)).double() * drop_scale(thr)
    hit = ((ops_sel == 1) & (boxes[:, :, 0] > -1.5)).view(-1)
    want = av.double().clone()
    want[hit, 2048:] = (emb.double()[None, :] * keep[:, 2048:])[hit]
    check("mask_feature_f32", ad, want, 1e-6)
    assert torch.equal(ad.cpu()[~hit], av[~hit]) and torch.equal(ad.cpu()[:, :2048], av[:, :2048])
    dfe = torch.randn(B * R, 2048, generator=g)
    dst = torch.ones(2048, device=dev())
    ops.masked_colsum_f32(dfe.to(dev()), ops_sel.to(dev()).view(-1), dst, drop_p=p, seed=seed, tag=TAG_DOWNSAMPLE, row_elems=4096, col_off=2048)
    check("masked_colsum_f32", dst, (dfe.double() * keep[:, 2048:])[ops_sel.view(-1) == 1].sum(0) + 1.0, 1e-6)


# -------------------------------------------------------------------------------------------------------------------------------
# front end of the engine
# -------------------------------------------------------------------------------------------------------------------------------
FRONT_PARAM_SEED = {(1, 64): 71, (1, 768): 73, (3, 64): 70, (3, 768): 102}      # chosen on the CPU: see the assertion of the test below


def _front_case(B, H):
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(hidden_size=H, num_hidden_layers=1, num_attention_heads=H // 64, intermediate_size=128, vocab_size=256,
                         max_position_embeddings=64, visual_region_classes=16)
    params = O.init_params(cfg, seed=FRONT_PARAM_SEED[(B, H)])
    batch = list(syn.make_batch(B, 32, 10, vocab_size=256, region_classes=16, seed=80 + B, ragged=True))
    boxes, mvrc_ops = batch[0], batch[5]
    if B == 3:
        mvrc_ops[0] = (boxes[0, :, 0] > -1.5).long()        # sample 0: every region masked
        mvrc_ops[1] = 0                                    # sample 1: none
        boxes[2] = -2.0                                    # sample 2: no valid box
        mvrc_ops[2] = 0
        batch[6][2] = 0
    return cfg, params, batch


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("B", [1, 3])
def test_front_end_f32_fwd_bwd(B, H, p):
    """pretrain_f32.front_fwd / front_bwd on an engine (T = 32, R = 10, S = 43, ragged): X[0], the projected regions and every gradient
    the front end produces -- d object_mask_visual_embedding, the per-sample d text_vis and the [2, H] table gradient among them --
    against float64 under the device's dropout masks."""
    E, ops = pkg("engine"), pkg("ops")
    cfg, params, batch = _front_case(B, H)
    T, R, S = 32, 10, 43
    mc = E.ModelConfig(hidden_size=H, num_hidden_layers=1, num_attention_heads=H // 64, intermediate_size=128, vocab_size=256,
                       max_position_embeddings=64, visual_region_classes=16, hidden_dropout_prob=p, attention_probs_dropout_prob=p,
                       obj_downsample_dropout=p)
    eng = E.PretrainEngine(mc, B, T, R, device="cuda:0", train=True, seed=11, encoder_fp32=True, fp32_full=True)
    eng.load_state_dict({k: v.to(dev()) for k, v in params.items()})
    eng.set_batch(*[t.to(dev()) for t in batch])
    eng.sync_weights()
    ops.seq_layout_into(eng.text_mask, eng.box_mask, S, eng.lay)
    g = torch.Generator().manual_seed(B + H)
    valid = RF.valid_rows(batch[2] > 0, batch[0][:, :, 0] > -1.5, S)
    dy = torch.randn(B, S, H, generator=g) * valid[..., None]
    ref = RF.front_ref(params, cfg, batch, S, dy, p_h=p, p_ds=p, seed=device_seed(eng), nh=H // 64)
    # a fair comparison: no pre-activation of the reference's ReLU within 1e-4 of zero (an fp32 product cannot flip it)
    cfg.obj_downsample_dropout = p
    hook = EngineDropoutMasks(device_seed(eng), S, R, H // 64) if p else None
    assert float(RF.obj_downsample_preact(params, cfg, batch, hook).abs().min()) > 1e-4
    eng.pre32.front_fwd(p, p)
    check("front end: projected regions", eng.pre32.obj_reps.view(B, R, H), ref["obj_reps"], 2e-5)
    check("front end: X[0]", eng.enc32.X[0].view(B, S, H) * valid[..., None].to(dev()), ref["out"] * valid[..., None], 2e-5)
    eng.P.grad.zero_()
    eng.pre32.front_bwd(dy.to(dev()).view(B * S, H).contiguous(), p, p)
    torch.cuda.synchronize()
    check("front end: d text_vis per sample", eng.pre32.d_textvis, ref["d_text_vis"], 2e-5)
    table = torch.cat((ref["grads"]["object_linguistic_embeddings.weight"], ref["grads"]["object_mask_word_embedding.weight"]))
    check("front end: d [2, H] linguistic table", eng.pre32.g_ling_table, table, 2e-5)
    if B == 3:      # sample 1 masks nothing, sample 2 has no box: the mask row's gradient comes from sample 0 alone
        assert float(ref["grads"]["object_mask_word_embedding.weight"].abs().max()) > 0
    for k in ("object_mask_visual_embedding.weight", "image_feature_extractor.obj_downsample.1.weight",
              "image_feature_extractor.obj_downsample.1.bias", "vlbert.visual_ln_text.weight", "vlbert.visual_ln_text.bias",
              "vlbert.visual_ln_object.weight", "vlbert.visual_ln_object.bias", "vlbert.word_embeddings.weight",
              "vlbert.position_embeddings.weight", "vlbert.token_type_embeddings.weight", "vlbert.end_embedding.weight",
              "vlbert.embedding_LayerNorm.weight", "vlbert.embedding_LayerNorm.bias"):
        check("front end: d " + k, eng.g32[k], ref["grads"][k], 2e-5)


# -------------------------------------------------------------------------------------------------------------------------------
# the engine against the oracle, beside the hybrid
# -------------------------------------------------------------------------------------------------------------------------------
BATCH_SEED = 347      # chosen on the CPU: no obj_downsample pre-activation of the oracle within 1e-4 of zero, eval and train (asserted below)


def _case():
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(num_hidden_layers=2)
    return cfg, O.init_params(cfg, seed=301), syn.make_batch(3, 32, 10, seed=BATCH_SEED, ragged=True)


def _errors(eng, oracle, cfg, batch):
    """{quantity: relative error} of an engine after forward + backward against the oracle's result."""
    from tests.test_engine_gpu import grad_errors, rel_fro
    outputs, _, grads, norm = oracle
    B, T, R = batch[2].shape[0], batch[2].shape[1], batch[0].shape[1]
    V, C = cfg.vocab_size, cfg.visual_region_classes
    max_len = int((batch[0][:, :, 0] > -1.5).sum(1).max())
    pairs = {"mlm": (eng.mlm_logits_copy[:, :V].view(B, T, V).float().cpu(), outputs["mlm_logits"].detach()),
             "mvrc": (eng.mvrc_logits_copy[:, :C].view(B, R, C)[:, :max_len].float().cpu(), outputs["mvrc_logits"].detach()[:, :max_len])}
    e = {}
    for k, (got, ref) in pairs.items():
        e["%s logits max-rel" % k] = float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
        e["%s logits rel-fro" % k] = rel_fro(got, ref)
    lv = eng.loss_values()
    for k in ("mlm_loss", "mvrc_loss"):
        if float(outputs[k]) != 0.0:
            e[k] = abs(lv[k] - float(outputs[k])) / abs(float(outputs[k]))
    e["grad norm"] = abs(eng.grad_norm() - norm) / norm
    for err, name in grad_errors(eng.grads(), grads, norm):
        e["d " + name] = err
    return e


def _full_beside_hybrid(tag, cfg, params, batch, train):
    from tests.test_engine_gpu import check_against_oracle, make_engine
    B, T, R = batch[2].shape[0], batch[2].shape[1], batch[0].shape[1]
    full = check_against_oracle(tag, cfg, params, batch, grad_tol=1e-3, logit_rtol=1e-3, logit_fro_tol=1e-3, loss_tol=1e-3, norm_tol=1e-3,
                                engine_kw=dict(encoder_fp32=True, fp32_full=True), train=train)
    assert full.mlm_logits_copy.dtype == F32 and full.X[-1].dtype == F32 and full.loss_scale == 1.0
    ef = _errors(full, full.oracle_result, cfg, batch)
    hyb = make_engine(cfg, B, T, R, train=train, encoder_fp32=True)
    hyb.load_state_dict({k: v.to(dev()) for k, v in params.items()})
    hyb.set_batch(*[t.to(dev()) for t in batch])
    assert device_seed(hyb) == device_seed(full)          # the same dropout masks: one oracle result serves both
    hyb.zero_grad()
    hyb.forward(train=train)
    hyb.backward(train=train)
    torch.cuda.synchronize()
    eh = _errors(hyb, full.oracle_result, cfg, batch)
    print("%s vs oracle: %-58s %-12s %-12s %s" % (tag, "quantity", "fp32_full", "hybrid", "ratio"))
    for k in ef:
        print("%s vs oracle: %-58s %.3e    %.3e    %s" % (tag, k, ef[k], eh[k], "%.1f" % (eh[k] / ef[k]) if ef[k] > 0 else "-"))
    print("%s vs oracle: worst fp32_full %.3e, worst hybrid %.3e" % (tag, max(ef.values()), max(eh.values())))
    for k, v in ef.items():
        assert v <= 1e-3, (k, v)                                             # (a): the fp32 gate, FRONT_TENSORS included
    if pkg("ops").BF16 == torch.bfloat16:
        for k in ef:
            assert ef[k] * 5 <= eh[k], (k, ef[k], eh[k])                     # (b)
    return full


@pytest.mark.parametrize("train", [False, True])
def test_engine_fp32_full_base_2_layers_vs_oracle(train):
    """The case of test_engine_fp32_encoder_base_2_layers_vs_oracle (2 base layers, B = 3, T = 32, R = 10, ragged, V = 30522, C = 1601),
    eval and train mode: (a) logits (max-relative and Frobenius), both losses, the gradient norm and every per-parameter gradient error
    <= 1e-3, with no exemption for the front-end tensors; (b) on the bf16 build each at least 5x below the hybrid's on the same case.
    The batch seed keeps every obj_downsample pre-activation of the oracle 1e-4 away from zero, so that no ReLU can flip."""
    cfg, params, batch = _case()
    assert float(RF.obj_downsample_preact(params, cfg, batch).abs().min()) > 1e-4
    hook = EngineDropoutMasks((1234 * 2 + 1) & 0x7FFFFFFF, 43, 10, 12, Sp=64)       # the engine's default seed (checked by the masks' test below)
    assert float(RF.obj_downsample_preact(params, cfg, batch, hook).abs().min()) > 1e-4
    eng = _full_beside_hybrid("fp32_full base 2-layer" + (" train" if train else ""), cfg, params, batch, train)
    assert device_seed(eng) == (1234 * 2 + 1) & 0x7FFFFFFF and eng.enc32.Sp == 64


def test_engine_fp32_full_no_valid_mvrc_rows_and_single_sample_vs_oracle():
    """The degenerate case of test_engine_no_valid_mvrc_rows_and_single_sample_vs_oracle: no valid soft label, B = 1."""
    from tests.test_engine_gpu import check_against_oracle
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(num_hidden_layers=1)
    params = O.init_params(cfg, seed=61)
    batch = list(syn.make_batch(1, 20, 7, seed=62, ragged=True))
    batch[5].zero_()
    batch[6].zero_()
    eng = check_against_oracle("fp32_full B=1, no MVRC labels", cfg, params, tuple(batch), grad_tol=1e-3, logit_rtol=1e-3, logit_fro_tol=1e-3,
                               loss_tol=1e-3, norm_tol=1e-3, engine_kw=dict(encoder_fp32=True, fp32_full=True))
    for k, v in _errors(eng, eng.oracle_result, cfg, batch).items():
        assert v <= 1e-3, (k, v)
    assert eng.loss_values()["mvrc_loss"] == 0.0 and bool(torch.isfinite(eng.P.grad).all())
    assert float(eng.g32["vlbert.mvrc_head.region_cls_pred.weight"].abs().max()) == 0.0


def test_engine_fp32_full_two_optimizer_steps():
    """train_step() twice with dropout on (labelled-row compaction off and on).  The first step's losses are the same bits under the same
    seed: nothing in a forward is summed in a run-dependent order.  The encoder's split-K weight gradients and the embedding backward add
    with float atomics (as in the hybrid), so the second step is held to the bounds test_engine_fp32_encoder_training_step_runs uses."""
    E, syn = pkg("engine"), pkg("synthetic")
    outs = []
    for _ in range(2):
        mc = E.ModelConfig(num_hidden_layers=2)
        eng = E.PretrainEngine(mc, 3, 32, 10, device="cuda:0", train=True, seed=5, encoder_fp32=True, fp32_full=True)
        eng.init_random(seed=1, visual_ln_init=1.0)
        eng.set_batch(*[t.to(dev()) for t in syn.make_batch(3, 32, 10, seed=9, ragged=True)])
        eng.train_step()
        first = eng.losses.clone()
        eng.train_step()
        torch.cuda.synchronize()
        lv = eng.loss_values()
        assert math.isfinite(lv["loss"]) and lv["mlm_loss"] > 0 and lv["mvrc_loss"] > 0 and bool(torch.isfinite(eng.P.master).all())
        outs.append((first, lv["loss"], eng.P.master.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and float(outs[0][0][0]) > 0 and float(outs[0][0][1]) > 0
    assert abs(outs[0][1] - outs[1][1]) <= 1e-4 * abs(outs[0][1])
    assert float((outs[0][2] - outs[1][2]).abs().max()) < 1e-4


def test_engine_fp32_full_step_graph_replays():
    """make_step_graph() on an fp32_full engine: the captured step replays (no allocation or host read on the fp32 path) and follows the
    eager engine within the bounds of the two-step test."""
    E, syn = pkg("engine"), pkg("synthetic")
    outs = []
    for graph in (False, True):
        eng = E.PretrainEngine(E.ModelConfig(num_hidden_layers=2), 3, 32, 10, device="cuda:0", train=True, seed=5, encoder_fp32=True, fp32_full=True)
        eng.init_random(seed=1, visual_ln_init=1.0)
        eng.set_batch(*[t.to(dev()) for t in syn.make_batch(3, 32, 10, seed=9, ragged=True)])
        eng.train_step()
        step = eng.make_step_graph() if graph else eng.train_step
        step()
        step()
        torch.cuda.synchronize()
        outs.append(eng.loss_values()["loss"])
        assert math.isfinite(outs[-1]) and float(eng.adam[5]) == 3.0      # (nothing runs during the capture itself)
    assert abs(outs[0] - outs[1]) <= 1e-4 * abs(outs[0])


def test_engine_fp32_full_compacted_mlm_rows_match_the_full_path(monkeypatch):
    """B x T = 2048 positions: the MLM head runs on the labelled rows only (capacity 512); losses and gradients equal the full path's."""
    E, syn = pkg("engine"), pkg("synthetic")
    res = []
    for compact in ("1", "0"):
        monkeypatch.setenv("VLB_MLM_COMPACT", compact)
        mc = E.ModelConfig(num_hidden_layers=1, vocab_size=1000, visual_region_classes=40)
        eng = E.PretrainEngine(mc, 32, 64, 4, device="cuda:0", train=False, seed=5, encoder_fp32=True, fp32_full=True)
        assert (eng.mlm_cap is not None) == (compact == "1")
        eng.init_random(seed=3, visual_ln_init=1.0)
        batch = syn.make_batch(32, 64, 4, vocab_size=1000, region_classes=40, seed=10, ragged=True)
        eng.set_batch(*[t.to(dev()) for t in batch])
        eng.zero_grad()
        eng.forward(train=False)
        eng.backward(train=False)
        torch.cuda.synchronize()
        res.append((eng.loss_values(), eng.P.grad.clone()))
    assert abs(res[0][0]["mlm_loss"] - res[1][0]["mlm_loss"]) <= 1e-6 * res[1][0]["mlm_loss"] and res[0][0]["mvrc_loss"] == res[1][0]["mvrc_loss"]
    check("compacted vs full path: flat gradient", res[0][1], res[1][1], 1e-5)


# -------------------------------------------------------------------------------------------------------------------------------
# no 16-bit tensor left: the two builds of the library give the same bits
# -------------------------------------------------------------------------------------------------------------------------------
def _dump_step(path):
    """Child: the 2-layer case forward (eval) + backward once; losses, logits and gradients into an .npz."""
    from tests.test_engine_gpu import make_engine
    cfg, params, batch = _case()
    eng = make_engine(cfg, 3, 32, 10, train=False, encoder_fp32=True, fp32_full=True)
    eng.load_state_dict({k: v.to(dev()) for k, v in params.items()})
    eng.set_batch(*[t.to(dev()) for t in batch])
    eng.zero_grad()
    eng.forward(train=False)
    eng.backward(train=False)
    torch.cuda.synchronize()
    g = eng.g32
    np.savez(path, losses=eng.losses.cpu().numpy(), mlm_logits=eng.mlm_logits_copy.cpu().numpy(), mvrc_logits=eng.mvrc_logits_copy.cpu().numpy(),
             g_cls=g["vlbert.mvrc_head.region_cls_pred.weight"].cpu().numpy(), g_mlm_dense=g["vlbert.mlm_head.predictions.transform.dense.weight"].cpu().numpy(),
             g_down=g["image_feature_extractor.obj_downsample.1.weight"].cpu().numpy(), g_mask=g["object_mask_visual_embedding.weight"].cpu().numpy(),
             g_ling=g["object_mask_word_embedding.weight"].cpu().numpy(), build=str(pkg("ops").BF16))


def test_no_16bit_rounding_left_in_the_step(tmp_path):
    """The 2-layer case on the two builds of the library (bf16 and fp16 as the 16-bit type), each in a fresh process: losses, logits and
    gradients are bit-identical -- a single 16-bit tensor between the inputs and the losses, or between the losses and the gradient,
    would round differently in the two.  (The gradients compared are ones whose summation order is fixed; those that float atomics
    feed -- the encoder's split-K weight gradients, the embedding tables', the bias column sums the weight-gradient GEMM takes on the
    side -- are not bit-reproducible from run to run.)"""
    dumps = []
    for prec in (None, "f16"):
        env = {k: v for k, v in os.environ.items() if k not in ("VLB_PRECISION", "VLB_LIB_PATH", "VLB_ENCODER_FP32", "VLB_FP32_FULL")}
        if prec:
            env["VLB_PRECISION"] = prec
        path = str(tmp_path / ("dump_%s.npz" % (prec or "bf16")))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        dumps.append(np.load(path))
    assert str(dumps[0]["build"]) == "torch.bfloat16" and str(dumps[1]["build"]) == "torch.float16"
    keys = [k for k in dumps[0].files if k != "build"]
    for k in keys:
        print("bf16 build vs fp16 build: %-12s max |difference| %.3e" % (k, float(np.abs(dumps[0][k].astype(np.float64) - dumps[1][k]).max())))
    for k in keys:
        a, b = dumps[0][k], dumps[1][k]
        assert a.dtype == np.float32 and np.isfinite(a).all() and float(np.abs(a).max()) > 0, k
        assert np.array_equal(a, b), (k, float(np.abs(a.astype(np.float64) - b).max()))


# -------------------------------------------------------------------------------------------------------------------------------
# module mirror and entry point
# -------------------------------------------------------------------------------------------------------------------------------
def test_module_mirror_fp32_full():
    """ResNetVLBERTForPretraining at tests/fixtures/pretrain_small.yaml with `fp32_encoder` + `fp32_full`: the loss is the engine's, the
    returned logits are fp32 and equal the engine's fp32 copies, loss.backward() leaves the gradients in param.grad (also with an upstream
    scale, which re-derives d(logits) from the kept fp32 logits), and all of it agrees with an engine built directly."""
    from tests.test_engine_gpu import make_engine
    tr, M = pkg("pretrain.train_end2end"), pkg("pretrain.modules")
    config = tr.load_config(os.path.join(ROOT, "tests", "fixtures", "pretrain_small.yaml"))
    config.NETWORK.VLBERT["fp32_encoder"] = True
    config.NETWORK.VLBERT["fp32_full"] = True
    cfg, params, batch = _case()
    net = M.ResNetVLBERTForPretraining(config)
    assert net.fp32_full
    net.load_state_dict({**params, "vlbert.mlm_head.predictions.decoder.weight": params["vlbert.word_embeddings.weight"]})
    net.eval()
    dbatch = tuple(t.to(dev()) for t in batch)
    outputs, loss = net(None, *dbatch)
    eng = next(iter(net._engines.values()))
    assert eng.fp32_full and eng.enc32 is not None and eng.mlm_logits_copy.dtype == F32
    B, T, R, V, C = 3, 32, 10, cfg.vocab_size, cfg.visual_region_classes
    assert float(loss.detach()) == float(eng.losses.sum()) and float(outputs["mlm_loss"]) == float(eng.losses[0])
    assert outputs["mlm_logits"].dtype == F32 and outputs["mvrc_logits"].dtype == F32
    assert torch.equal(outputs["mlm_logits"], eng.mlm_logits_copy[:, :V].view(B, eng.T, V)[:, :T])
    nobj = int((batch[0][:, :, 0] > -1.5).sum(1).max())
    assert torch.equal(outputs["mvrc_logits"][:, :nobj], eng.mvrc_logits_copy[:, :C].view(B, eng.R, C)[:, :nobj])
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    total = float(torch.nn.utils.clip_grad_norm_(net.parameters(), 1e9))
    direct = make_engine(cfg, B, T, R, train=False, encoder_fp32=True, fp32_full=True)
    direct.load_state_dict({k: v.to(dev()) for k, v in params.items()})
    direct.set_batch(*dbatch)
    direct.zero_grad()
    direct.forward(train=False)
    direct.backward(train=False)
    ref = direct.loss_values()["loss"]
    assert abs(float(loss.detach()) - ref) <= 1e-5 * ref and abs(total - direct.grad_norm()) <= 1e-4 * total
    net.zero_grad()
    _, loss2 = net(None, *dbatch)
    (loss2 / 2).backward()                                   # upstream scale, as with gradient accumulation
    half = float(torch.nn.utils.clip_grad_norm_(net.parameters(), 1e9))
    assert abs(half - 0.5 * total) <= 1e-4 * total


def test_train_end2end_fp32_full_trains_and_prints_its_mode():
    """python -m vl-bert_amd.pretrain.train_end2end --compute fp32-full (a fresh process: the mode switches the build of the library)."""
    env = {k: v for k, v in os.environ.items() if k not in ("VLB_PRECISION", "VLB_LIB_PATH")}
    cmd = [sys.executable, "-m", "vl-bert_amd.pretrain.train_end2end", "--cfg", os.path.join(ROOT, "tests", "fixtures", "pretrain_small.yaml"),
           "--compute", "fp32-full", "--steps", "2", "--steps-per-epoch", "20", "--text-len", "32", "--regions", "10"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "compute fp32-full" in r.stdout and "fp32_full: front end, encoder, heads and losses in fp32" in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    _dump_step(sys.argv[1])
