"""GPU tests of the fp32 front and back end of the VQA fine-tuning route (`fp32_ends`): the kernels of vl-bert_amd/csrc/f32_ends.hip and
the fp32 classifier head against float64 references (tests/fp32_ends_ref.py), then the route itself -- the VQA mirror against the
reference fixture and the oracle, the same at BASELINE config 4's widths, bit-identical results on the two builds of the library (no
16-bit tensor is left on the route), and two optimizer steps.

Bars: 1e-5 relative Frobenius for the LayerNorm-class kernels, 2e-5 for anything through the split-operand GEMM (the bars
tests/test_f32_encoder_gpu.py holds the fp32 kernels to); 1e-3, the project's fp32 tolerance, for the route."""
import os
import subprocess
import sys

if __name__ == "__main__":          # the child of test_no_16bit_rounding_left_on_the_route
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import torch

from tests.gpu_util import dev, drop_thr, keep_mask, pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32


def rel(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def check(name, got, ref, bar):
    e = rel(got, ref)
    print("  %-46s rel-fro %.3e  (bar %.0e)" % (name, e, bar))
    assert e <= bar, (name, e)


def seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int32, device=dev())


# -------------------------------------------------------------------------------------------------------------------------------
# kernels
# -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [13, 16])
@pytest.mark.parametrize("H", [64, 768, 1024])
def test_embed_f32_fwd_bwd(H, S, p):
    from tests.embed_attn_refs import EMBED_SEED, embed_ref, embed_untouched
    from tests.fp32_ends_ref import embed_case32
    from tests.gpu_util import TAG_EMBED
    ops = pkg("ops")
    c = embed_case32(H, S, p)
    fwd, grads = embed_ref(c)
    B, T, R, V, P = c["B"], c["T"], c["R"], c["V"], c["P"]
    d = dev()
    g = lambda k: c[k].to(d).contiguous()
    lay = ops.seq_layout(c["text_mask"].to(d), c["obj_mask"].to(d), S)
    z = lambda *s: torch.zeros(s, dtype=F32, device=d)
    pre, stats, out = z(B * S, H), z(B * S, 2), z(B * S, H)
    seed = seed_tensor(EMBED_SEED)
    text_vis, obj_vis, obj_ling = g("text_vis"), g("obj_vis"), g("obj_ling")
    ops.embed_f32_fwd(lay, g("text_ids"), g("text_type"), g("word"), g("pos"), g("type"), g("end"), text_vis, (T * H, H), obj_vis,
                      (R * H, H), obj_ling, (R * H, H), None, g("gamma"), g("beta"), pre, stats, out, B, T, R, S, H, drop_p=p, seed=seed,
                      tag=TAG_EMBED)
    check("embed_f32 out", out, fwd["out"], 1e-5)
    check("embed_f32 pre-LN sum", pre, fwd["pre"], 1e-5)
    check("embed_f32 mean", stats[:, 0], fwd["mean"], 1e-5)
    check("embed_f32 rstd", stats[:, 1], fwd["rstd"], 1e-5)
    G = dict(word=z(V, H), pos=z(P, H), type=z(3, H), end=z(1, H), gamma=z(H), beta=z(H), text_vis=z(B, T, H), obj_vis=z(B, R, H),
             obj_ling=z(B, R, H))
    ops.embed_f32_bwd(g("dy").view(B * S, H), pre, stats, g("gamma"), lay, g("text_ids"), g("text_type"), None, G["word"], G["pos"],
                      G["type"], G["end"], G["gamma"], G["beta"], G["text_vis"], (T * H, H), G["obj_vis"], (R * H, H), G["obj_ling"],
                      (R * H, H), B, T, R, S, H, drop_p=p, seed=seed, tag=TAG_EMBED)
    for k in ("text_vis", "obj_vis", "obj_ling", "word", "pos", "type", "end", "gamma", "beta"):
        check("embed_f32 d_" + k, G[k], grads[k], 1e-5)
    un = embed_untouched(c)
    assert float(G["word"][un["word"].to(d)].abs().max()) == 0.0 and int(un["word"].sum()) > 0
    if P > S:
        assert float(G["pos"][un["pos"].to(d)].abs().max()) == 0.0 and int(un["pos"].sum()) > 0
    else:
        assert not bool(un["pos"].any())              # P = 8: the object and end rows clamp to the last position row
    assert float(G["obj_vis"][un["obj"].to(d)].abs().max()) == 0.0 and float(G["obj_ling"][un["obj"].to(d)].abs().max()) == 0.0
    assert float(G["text_vis"][un["text"].to(d)].abs().max()) == 0.0


def test_embed_f32_rejects_the_table_form():
    ops = pkg("ops")
    d = dev()
    z = lambda *s: torch.zeros(s, dtype=F32, device=d)
    lay = ops.seq_layout(torch.ones(1, 2, dtype=torch.bool, device=d), torch.ones(1, 1, dtype=torch.bool, device=d), 4)
    ids = torch.zeros(1, 2, dtype=torch.int64, device=d)
    with pytest.raises(RuntimeError, match="obj_ling_idx"):
        ops.embed_f32_fwd(lay, ids, ids, z(4, 64), z(8, 64), z(3, 64), z(1, 64), z(1, 2, 64), (128, 64), z(1, 1, 64), (64, 64), z(2, 64),
                          (0, 0), torch.zeros(1, 1, dtype=torch.int64, device=d), z(64), z(64), z(4, 64), z(4, 2), z(4, 64), 1, 2, 1, 4, 64)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("ldinfo", [4, 5])
def test_obj_prep_f32_and_projection(ldinfo, p):
    """obj_prep_f32 -> the fp32 GEMM with bias + ReLU -> zero_padded_rows_f32: B = 2, R = 5, two padded boxes (a hole between valid
    boxes in one sample, the tail of the other).  The rows of padded boxes are exactly zero after the projection."""
    from tests.fp32_ends_ref import obj_prep_ref
    ops, syn = pkg("ops"), pkg("synthetic")
    d = dev()
    boxes, im_info, _, _ = syn.make_vqa_batch(2, 5, 4, 11, "cpu", answers=8)
    boxes[0, 2] = -2.0
    boxes[1, 4] = -2.0
    info = torch.zeros(2, ldinfo)
    info[:, :4] = im_info
    SEED, TAG = 777, 1001
    ref = obj_prep_ref(boxes, info, SEED, TAG, p)
    a = torch.full((10, 4096), 7.0, dtype=F32, device=d)
    ops.obj_prep_f32_fwd(boxes.to(d), info.to(d), a, drop_p=p, seed=seed_tensor(SEED), tag=TAG)
    check("obj_prep_f32", a, ref, 1e-5)
    assert float(a[2].abs().max()) == 0.0 and float(a[9].abs().max()) == 0.0
    if p > 0:      # the mask itself: zeros exactly where the host restatement of the keep bit says
        keep = keep_mask(SEED, TAG, np.arange(10 * 4096), drop_thr(p)).reshape(10, 4096)
        live = torch.from_numpy(keep) & (ref != 0)
        assert bool(((a.cpu() != 0) == live).all())
    Hd = 64
    g = torch.Generator().manual_seed(3)
    W, b = (torch.randn(Hd, 4096, generator=g) * 0.02).float(), (0.5 + torch.randn(Hd, generator=g)).float()      # relu(bias) != 0
    y = torch.full((10, Hd), 7.0, dtype=F32, device=d)
    ops.gemm_nt_f32(a, 4096, W.to(d), 4096, y, Hd, 10, Hd, 4096, bias=b.to(d), epi=2)
    assert float(y[2].abs().max()) > 0.0          # relu(bias) stands in a padded row before it is cleared
    ops.zero_padded_rows_f32(y, boxes.to(d))
    yr = torch.relu(ref @ W.double().t() + b.double()) * (boxes[..., 0] > -1.5).reshape(10, 1)
    check("projection of obj_prep_f32", y, yr, 2e-5)
    assert float(y[2].abs().max()) == 0.0 and float(y[9].abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 4099])
def test_dropout_f32_matches_the_16bit_mask(n):
    ops = pkg("ops")
    d = dev()
    SEED, TAG, p = 4321, 2002, 0.5
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).float()
    x[x == 0] = 1.0
    y = torch.full((n,), 7.0, dtype=F32, device=d)
    ops.dropout_f32(x.to(d), y, p, seed_tensor(SEED), TAG)
    keep = torch.from_numpy(keep_mask(SEED, TAG, np.arange(n), drop_thr(p)))
    scale = np.float32(65536.0) / np.float32(65536.0 - drop_thr(p))
    want = torch.where(keep, x * float(scale), torch.zeros_like(x))
    assert torch.equal(y.cpu(), want)                                   # bit-equal to x * scale where kept, 0 elsewhere
    ones = torch.ones(n, dtype=ops.BF16, device=d)
    y16 = torch.zeros(n, dtype=ops.BF16, device=d)
    ops.dropout_bf16(ones, y16, p, seed_tensor(SEED), TAG)
    assert torch.equal(y16.cpu() != 0, y.cpu() != 0)                    # the mask vlb_dropout_bf16 draws for the same (seed, tag)
    y0 = torch.zeros(n, dtype=F32, device=d)
    ops.dropout_f32(x.to(d), y0, 0.0, None, TAG)
    assert torch.equal(y0.cpu(), x)


@pytest.mark.parametrize("copy", [False, True])
@pytest.mark.parametrize("pw,gs", [(1.0, 1.0), (2.5, 0.25), (2.5, 1.0), (1.0, 0.25)])
@pytest.mark.parametrize("A", [7, 3129])
@pytest.mark.parametrize("rows", [1, 5])
def test_bce_logits_f32(rows, A, pw, gs, copy):
    from tests.fp32_ends_ref import bce_ref
    ops = pkg("ops")
    d = dev()
    ld = (A + 3) // 4 * 4
    g = torch.Generator().manual_seed(rows * 10000 + A)
    x = (torch.randn(rows, A, generator=g) * 3).float()
    y = torch.rand(rows, A, generator=g).float()                        # soft labels
    y[:, 0], y[:, -1] = 1.0, 0.0
    loss_ref, grad_ref = bce_ref(x, y, pw, gs)
    buf = torch.full((rows, ld), 5.0, dtype=F32, device=d)
    buf[:, :A] = x.to(d)
    cp = torch.full((rows, ld), 5.0, dtype=F32, device=d) if copy else None
    loss = torch.full((1,), 2.0, dtype=F32, device=d)                   # the loss is ACCUMULATED
    ops.bce_logits_f32_fwd_bwd(buf, A, y.to(d), loss, gscale=gs, logits_copy=cp, pos_weight=pw)
    assert abs(float(loss) - 2.0 - float(loss_ref)) <= 1e-5 * float(loss_ref), (float(loss) - 2.0, float(loss_ref))
    check("bce_logits_f32 d logits", buf[:, :A], grad_ref, 1e-5)
    assert ld > A and float(buf[:, A:].abs().max()) == 0.0              # padding columns exactly 0
    if copy:
        assert torch.equal(cp[:, :A].cpu(), x) and (ld == A or float(cp[:, A:].abs().max()) == 0.0)


def test_bce_logits_f32_loss_has_a_fixed_summation_order():
    """The rows' sums are added in a fixed order (no float atomic between the rows' workgroups): 37 rows x 3129 answers give the same
    bits on every call."""
    ops = pkg("ops")
    d = dev()
    rows, A, ld = 37, 3129, 3132
    g = torch.Generator().manual_seed(5)
    x = torch.zeros(rows, ld)
    x[:, :A] = torch.randn(rows, A, generator=g) * 3
    y = torch.rand(rows, A, generator=g).to(d)
    losses = []
    for _ in range(6):
        buf, loss = x.to(d), torch.zeros(1, dtype=F32, device=d)
        ops.bce_logits_f32_fwd_bwd(buf, A, y, loss)
        losses.append(loss)
    losses = torch.cat(losses).cpu()
    assert bool(torch.isfinite(losses).all()) and float(losses[0]) > 0
    assert torch.equal(losses, losses[0].expand(6)), losses.tolist()


def _lin(o, i, g):
    m = torch.nn.Module()
    bound = (6.0 / (o + i)) ** 0.5
    m.register_parameter("weight", torch.nn.Parameter(((torch.rand(o, i, generator=g) * 2 - 1) * bound).to(dev())))
    m.register_parameter("bias", torch.nn.Parameter((torch.randn(o, generator=g) * 0.1).to(dev())))
    return m


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("rows", [3, 37])
@pytest.mark.parametrize("classifier", ["2fc", "1fc", "mlm"])
def test_fp32_head_vs_float64(classifier, rows, p):
    """The three classifiers of the VQA module from the fp32 stages (hidden 768, 3129 answers, rows that are no multiple of 32), BCE,
    upstream factor 0.25 (d(logits) is re-derived from the kept logits): logits, loss, d x and every parameter gradient."""
    from tests.fp32_ends_ref import head_ref
    HD, ops = pkg("common.heads"), pkg("ops")
    H, A, hc, SEED, T0, T1 = 768, 3129, 1024, 991, 2001, 2002
    g = torch.Generator().manual_seed(17)
    lin32 = lambda m, act=None: HD.Linear32(HD.Weight32(m), act)
    if classifier == "2fc":
        mods = {"1": _lin(hc, H, g), "4": _lin(A, hc, g)}
        stages = [HD.Drop32(T0), lin32(mods["1"], "relu"), HD.Drop32(T1), lin32(mods["4"])]
        P = {"1.weight": mods["1"].weight, "1.bias": mods["1"].bias, "4.weight": mods["4"].weight, "4.bias": mods["4"].bias}
    elif classifier == "1fc":
        mods = {"1": _lin(A, H, g)}
        stages = [HD.Drop32(T0), lin32(mods["1"])]
        P = {"1.weight": mods["1"].weight, "1.bias": mods["1"].bias}
    else:
        ln = torch.nn.Module()
        ln.register_parameter("weight", torch.nn.Parameter((1.0 + 0.2 * torch.randn(H, generator=g)).to(dev())))
        ln.register_parameter("bias", torch.nn.Parameter((0.2 * torch.randn(H, generator=g)).to(dev())))
        mods = {"d": _lin(H, H, g), "2": _lin(A, H, g)}
        stages = [lin32(mods["d"], "gelu"), HD.LayerNorm32(ln), HD.Drop32(T1), lin32(mods["2"])]
        P = {"0.dense.weight": mods["d"].weight, "0.dense.bias": mods["d"].bias, "0.LayerNorm.weight": ln.weight,
             "0.LayerNorm.bias": ln.bias, "2.weight": mods["2"].weight, "2.bias": mods["2"].bias}
    head = HD.Head32(stages, seed_tensor(SEED))
    assert [id(q) for q in head.params()] == [id(q) for q in P.values()]
    x = torch.randn(rows, H, generator=g).float()
    label = torch.rand(rows, A, generator=g).float() * (torch.rand(rows, A, generator=g) < 0.01)
    if classifier == "2fc":
        # ReLU has no derivative at 0: a pre-activation within the fp32 GEMM's own error of 0 (~1e-6 here; one of 37 x 1024 was
        # 3.9e-7) takes either branch, and either is right.  The case is built without such units: their bias moves until every
        # pre-activation is at least 1e-4 (a hundred times that error) away from the kink.
        from tests.fp32_ends_ref import keep_scale
        xd = x.double() * keep_scale(SEED, T0, x.numel(), p).reshape(x.shape)
        for _ in range(50):
            pre = xd @ mods["1"].weight.detach().double().cpu().t() + mods["1"].bias.detach().double().cpu()
            near = (pre.abs() < 1e-4).any(0)
            if not bool(near.any()):
                break
            with torch.no_grad():
                mods["1"].bias[near.to(dev())] += 1e-3
        assert not bool(near.any())
    xg = x.to(dev()).requires_grad_(True)
    lab = label.to(dev())

    def bce(logits, logits_copy, loss, gs, fresh):
        ops.bce_logits_f32_fwd_bwd(logits, A, lab, loss, gscale=gs, logits_copy=logits_copy if fresh else None)
    logits, loss = HD.run_head(head, xg, p, bce)
    assert logits.dtype == F32 and loss.dtype == F32
    logits = logits[:, :A].clone()
    (0.25 * loss).backward()
    rl, rloss, rdx, rg = head_ref(classifier, {k: v.detach().cpu() for k, v in P.items()}, x, label, p, SEED, (T0, T1), g=0.25)
    check("head32 %s logits" % classifier, logits, rl, 2e-5)
    assert abs(float(loss.detach()) - float(rloss)) <= 2e-5 * float(rloss), (float(loss.detach()), float(rloss))
    check("head32 %s d x" % classifier, xg.grad, rdx, 2e-5)
    for k, q in P.items():
        check("head32 %s d %s" % (classifier, k), q.grad, rg[k], 2e-5)


# -------------------------------------------------------------------------------------------------------------------------------
# the route
# -------------------------------------------------------------------------------------------------------------------------------
def _vqa_net(cfg, classifier, A, hidden, params, ends):
    from tests.test_engine_gpu import _vqa_config
    M = pkg("vqa.modules.resnet_vlbert_for_vqa")
    conf = _vqa_config(cfg, classifier, A, hidden)
    conf["NETWORK"]["VLBERT"].update(fp32_encoder=True, fp32_ends=ends)
    net = M.ResNetVLBERT(conf, device="cuda:0")
    assert set(net.state_dict()) == set(params), set(net.state_dict()) ^ set(params)
    net.load_state_dict({k: v for k, v in params.items()})              # a reference-named state_dict in ...
    net.train()
    for m in (net.vlbert, net.image_feature_extractor):                 # every dropout off
        m.eval()
    net.cls_drop = 0.0
    return net


def _route_errors(net, batch, ref_logits, ref_loss, ref_grads, names):
    """{quantity: error} of one train_forward + backward against the reference values."""
    boxes, im_info, question, label = [t.to(dev()) for t in batch]
    net.zero_grad()
    outputs, loss = net.train_forward(None, boxes, im_info, question, label)
    loss.backward()
    lg, rl = outputs["label_logits"].detach().double().cpu(), ref_logits.double()
    e = {"logits max-rel": float((lg - rl).abs().max() / rl.abs().max()), "logits rel-fro": rel(lg, rl),
         "loss rel": abs(float(loss.detach()) - float(ref_loss)) / abs(float(ref_loss))}
    got = dict(net.named_parameters())
    for k in names:
        e["d " + k] = rel(got[k].grad, ref_grads[k])
    return e, outputs["label_logits"].detach().clone(), float(loss.detach())


_GRAD_NAMES = ["vlbert.encoder.layer.1.output.dense.weight", "image_feature_extractor.obj_downsample.1.weight", "vlbert.word_embeddings.weight",
               "object_linguistic_embeddings.weight"]
_HEAD_NAMES = {"2fc": ["final_mlp.1.weight", "final_mlp.4.weight", "final_mlp.4.bias"],
               "mlm": ["final_mlp.0.dense.weight", "final_mlp.0.LayerNorm.weight", "final_mlp.2.weight", "final_mlp.2.bias"]}


@pytest.mark.parametrize("classifier", ["2fc", "mlm"])
def test_vqa_fp32_ends_vs_reference_fixture_and_oracle(classifier):
    """The inputs and comparisons of test_vqa_module_mirror_vs_reference_fixture_and_oracle with fp32_encoder + fp32_ends: (a) every
    error <= 1e-3; (b) on the bf16 build each at least 5x below the same quantity of the hybrid (fp32_encoder alone), measured here.

    Measured on an MI355X (bf16 build), new route / hybrid -- see DESIGN.md section 3 for the table this test prints."""
    from oracle import vqa_oracle as VQ
    from tests.test_oracle_golden import load_vqa_case
    ops = pkg("ops")
    z, cfg, params, batch = load_vqa_case()
    A, hidden = int(z["answer_vocab"]), int(z["classifier_hidden"])
    if classifier != "2fc":
        params = VQ.init_vqa_params(cfg, int(z["pseed"]), A, classifier)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out, oloss = VQ.vqa_forward(leaves, cfg, *batch, classifier=classifier, classifier_dropout=0.0, train=False)
    oloss.backward()
    ref_grads = {k: v.grad for k, v in leaves.items()}
    names = _GRAD_NAMES + _HEAD_NAMES[classifier]
    net = _vqa_net(cfg, classifier, A, hidden, params, True)
    full, logits, loss = _route_errors(net, batch, out["label_logits"].detach(), oloss.detach(), ref_grads, names)
    hyb, _, _ = _route_errors(_vqa_net(cfg, classifier, A, hidden, params, False), batch, out["label_logits"].detach(), oloss.detach(),
                              ref_grads, names)
    print("vqa %s vs oracle: %-58s %-12s %-12s %s" % (classifier, "quantity", "fp32_ends", "hybrid", "ratio"))
    for k in full:
        print("vqa %s vs oracle: %-58s %.3e    %.3e    %.1f" % (classifier, k, full[k], hyb[k], hyb[k] / max(full[k], 1e-300)))
    if classifier == "2fc":      # the fixture of the reference's own module
        rl = torch.from_numpy(z["logits"]).double()
        fx = {"logits max-rel (fixture)": float((logits.double().cpu() - rl).abs().max() / rl.abs().max()),
              "logits rel-fro (fixture)": rel(logits, rl), "loss rel (fixture)": abs(loss - float(z["loss"])) / float(z["loss"])}
        for k, v in fx.items():
            print("vqa 2fc vs reference fixture: %-46s %.3e" % (k, v))
        full.update(fx)
    for k, v in full.items():
        assert v <= 1e-3, (k, v)                                         # (a)
    if ops.BF16 == torch.bfloat16:
        for k in hyb:
            assert full[k] * 5 <= hyb[k], (k, full[k], hyb[k])           # (b)
    boxes, im_info, question, label = [t.to(dev()) for t in batch]
    net.eval()
    inf = net(None, boxes, im_info, question)["label_logits"]
    assert inf.dtype == F32 and rel(inf, out["label_logits"].detach()) <= 1e-3
    sd = net.state_dict()                                                # ... and out again
    assert set(sd) == set(params)
    assert all(torch.equal(sd[k].cpu(), params[k]) for k in ("final_mlp.%s.weight" % ("4" if classifier == "2fc" else "2"),
                                                              "vlbert.word_embeddings.weight"))
    net.train()                                                          # classifier dropout on: runs, finite, another loss
    net.cls_drop = 0.5
    _, l2 = net.train_forward(None, boxes, im_info, question, label)
    l2.backward()
    assert torch.isfinite(l2) and abs(float(l2.detach()) - loss) > 0


def test_vqa_fp32_ends_at_config4_widths_vs_oracle():
    """hidden 1024, 16 heads, intermediate 4096 (VL-BERT-large, cfgs/vqa/large_4x16G_fp32.yaml) at 2 layers: B = 2, 20 question tokens,
    11 boxes, the shipped "mlm" classifier with 3129 answers, against the oracle; the bars of (a)."""
    from oracle import vlbert_oracle as O
    from oracle import vqa_oracle as VQ
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096, vocab_size=2048,
                         max_position_embeddings=64, visual_region_classes=50, hidden_dropout_prob=0.0,
                         attention_probs_dropout_prob=0.0, obj_downsample_dropout=0.0)
    A = 3129
    params = VQ.init_vqa_params(cfg, 23, A, "mlm")
    batch = syn.make_vqa_batch(2, 11, 20, 29, "cpu", answers=A)
    batch[2] = batch[2] % 2000 + 5                                      # question ids inside the small vocabulary
    batch[2][1, 13:] = 0                                                # ragged questions
    batch[0][1, 8:] = -2.0                                              # ragged boxes
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out, oloss = VQ.vqa_forward(leaves, cfg, *batch, classifier="mlm", classifier_dropout=0.0, train=False)
    oloss.backward()
    names = _GRAD_NAMES + _HEAD_NAMES["mlm"]
    net = _vqa_net(cfg, "mlm", A, 1024, params, True)
    full, _, _ = _route_errors(net, batch, out["label_logits"].detach(), oloss.detach(), {k: v.grad for k, v in leaves.items()}, names)
    for k, v in full.items():
        print("vqa mlm (large widths) vs oracle: %-58s %.3e" % (k, v))
    for k, v in full.items():
        assert v <= 1e-3, (k, v)


def _dump_route(path):
    """Child: the VQA case forward (eval) and backward once; logits, loss and two gradients into an .npz."""
    from oracle import vqa_oracle as VQ
    from tests.test_oracle_golden import load_vqa_case
    z, cfg, params, batch = load_vqa_case()
    A = int(z["answer_vocab"])
    params = VQ.init_vqa_params(cfg, int(z["pseed"]), A, "mlm")
    net = _vqa_net(cfg, "mlm", A, int(z["classifier_hidden"]), params, True)
    boxes, im_info, question, label = [t.to(dev()) for t in batch]
    outputs, loss = net.train_forward(None, boxes, im_info, question, label)
    loss.backward()
    got = dict(net.named_parameters())
    np.savez(path, logits=outputs["label_logits"].detach().cpu().numpy(), loss=loss.detach().cpu().numpy(),
             g_head=got["final_mlp.2.weight"].grad.cpu().numpy(),
             g_down=got["image_feature_extractor.obj_downsample.1.weight"].grad.cpu().numpy(), build=str(pkg("ops").BF16))


def test_no_16bit_rounding_left_on_the_route(tmp_path):
    """The same case on the two builds of the library (bf16 and fp16 as the 16-bit type), each in a fresh process: logits, loss and two
    gradients are bit-identical -- a single 16-bit tensor on the route would round differently in the two.  (The two gradients are ones
    whose summation order is fixed: no atomics between several K slices or workgroups feed them.)"""
    dumps = []
    for prec in (None, "f16"):
        env = {k: v for k, v in os.environ.items() if k not in ("VLB_PRECISION", "VLB_LIB_PATH", "VLB_ENCODER_FP32", "VLB_FP32_ENDS")}
        if prec:
            env["VLB_PRECISION"] = prec
        path = str(tmp_path / ("dump_%s.npz" % (prec or "bf16")))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        dumps.append(np.load(path))
    assert str(dumps[0]["build"]) == "torch.bfloat16" and str(dumps[1]["build"]) == "torch.float16"
    for k in ("logits", "loss", "g_head", "g_down"):
        print("bf16 build vs fp16 build: %-8s max |difference| %.3e" % (k, float(np.abs(dumps[0][k].astype(np.float64) - dumps[1][k]).max())))
    for k in ("logits", "loss", "g_head", "g_down"):
        a, b = dumps[0][k], dumps[1][k]
        assert a.dtype == np.float32 and np.isfinite(a).all() and float(np.abs(a).max()) > 0
        assert np.array_equal(a, b), (k, float(np.abs(a.astype(np.float64) - b).max()))


def test_vqa_fp32_ends_two_optimizer_steps():
    """FusedAdamW on the flagged mirror with every dropout on: finite, and the same under the same seed within the bounds
    test_engine_fp32_encoder_training_step_runs uses (atomics reorder a few fp32 sums)."""
    from oracle import vqa_oracle as VQ
    from tests.test_engine_gpu import _vqa_config
    from tests.test_oracle_golden import load_vqa_case
    M, OPT = pkg("vqa.modules.resnet_vlbert_for_vqa"), pkg("optim")
    z, cfg, params, batch = load_vqa_case()
    A = int(z["answer_vocab"])
    params = VQ.init_vqa_params(cfg, int(z["pseed"]), A, "mlm")
    boxes, im_info, question, label = [t.to(dev()) for t in batch]
    outs = []
    for _ in range(2):
        conf = _vqa_config(cfg, "mlm", A, int(z["classifier_hidden"]))
        conf["NETWORK"]["VLBERT"].update(fp32_encoder=True, fp32_ends=True)
        net = M.ResNetVLBERT(conf, device="cuda:0")
        net.load_state_dict({k: v for k, v in params.items()})
        net.train()
        opt = OPT.FusedAdamW(net.parameters(), lr=1e-4, weight_decay=1e-4)
        for _ in range(2):
            opt.zero_grad()
            _, loss = net.train_forward(None, boxes, im_info, question, label)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        outs.append((float(loss.detach()), torch.cat([q.detach().reshape(-1) for q in net.parameters()]).clone()))
        assert bool(torch.isfinite(outs[-1][1]).all())
    assert abs(outs[0][0] - outs[1][0]) <= 1e-4 * abs(outs[0][0])
    assert float((outs[0][1] - outs[1][1]).abs().max()) < 1e-4


if __name__ == "__main__":
    _dump_route(sys.argv[1])
