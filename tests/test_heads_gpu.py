"""The shared hand-scheduled head (common/heads.py) on the MI355X, driven directly -- forward, loss, backward with an upstream factor --
against fp32 torch autograd on the same 16-bit-rounded inputs and weights.  The dropout masks are the device's own: vlb_dropout_bf16 on
ones under the head's seed and each site's tag, read before the step (the backward advances the seed), so a backward that replays a
site under the wrong tag shows up as a gradient error.  Bars: the ones the module tests of these heads use (logits 2e-2 abs/rel, loss
1e-2 relative, gradients rel-Frobenius 5e-2)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.gpu_util import act_dtype, dev, pkg, report

pytestmark = pytest.mark.gpu
P_DROP, FACTORS = (0.0, 0.3), (1.0, 0.37)


def rel_fro(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-12))


def _r16(t):
    return t.to(act_dtype()).float()


def _lin(o, i, g, scale=1.0):
    m = nn.Module()
    m.weight = nn.Parameter(_r16(torch.randn(o, i, generator=g) * scale / i ** 0.5).to(dev()))
    m.bias = nn.Parameter(_r16(torch.randn(o, generator=g) * 0.1).to(dev()))
    return m


def _ln(n, g):
    m = nn.Module()
    m.weight = nn.Parameter(_r16(1.0 + 0.2 * torch.randn(n, generator=g)).to(dev()))
    m.bias = nn.Parameter(_r16(0.1 * torch.randn(n, generator=g)).to(dev()))
    return m


def _keep_mask(rows, width, p, seed, tag):
    """the 0/1 mask of vlb_dropout_bf16 on a contiguous [rows, width padded to 64] buffer (what a site sees) under (seed, tag)"""
    ops = pkg("ops")
    ones = torch.ones(rows, (width + 63) // 64 * 64, dtype=ops.BF16, device=dev())
    return (ops.dropout_bf16(ones, torch.empty_like(ones), p, seed, tag) != 0).float()


def _build(case, g):
    """-> (head, x [rows, 128] fp32, torch stages [(kind, ...)], loss_fn of the head, torch loss(logits [rows, N]), N, logits view)"""
    Hd, ops = pkg("common.heads"), pkg("ops")
    seed = torch.tensor([ops.rank_seed(12345)], dtype=torch.int32, device=dev())
    H = 128
    full = lambda z, N: z[:, :N].float()
    if case in ("2fc", "mlm", "reg"):
        rows, N = (37, 81) if case == "reg" else (5, 70)
        if case == "2fc":
            a, b = _lin(100, H, g), _lin(N, 100, g)
            stages = [Hd.Drop(2001), Hd.Linear(Hd.Linear16(a), "relu"), Hd.Drop(2002), Hd.Linear(Hd.Linear16(b, pad_k=True))]
            ref = [("drop", 2001), ("lin", a, "relu"), ("drop", 2002), ("lin", b, None)]
        elif case == "mlm":
            a, n, b = _lin(H, H, g), _ln(H, g), _lin(N, H, g)
            stages = [Hd.Linear(Hd.Linear16(a), "gelu"), Hd.LayerNorm(n), Hd.Drop(2002), Hd.Linear(Hd.Linear16(b, pad_k=True))]
            ref = [("lin", a, "gelu"), ("ln", n), ("drop", 2002), ("lin", b, None)]
        else:
            a, b = _lin(H, H, g), _lin(N, H, g)
            stages = [Hd.Linear(Hd.Linear16(a), "gelu"), Hd.Drop(3001), Hd.Linear(Hd.Linear16(b))]
            ref = [("lin", a, "gelu"), ("drop", 3001), ("lin", b, None)]
        head = Hd.Head(stages, seed, row_cap=64 if case == "reg" else 1)
        if case == "reg":       # CE over the 81 classes, mean over the rows
            labels = torch.randint(0, N, (rows,), generator=g).to(dev())
            count = torch.zeros(1, device=dev())

            def loss_fn(logits, copy, loss, gs, fresh):
                ops.ce_fwd_bwd(logits, N, labels, count, loss, gscale=gs, logits_copy=copy if fresh else None)
            tloss = lambda z: F.cross_entropy(z, labels)
        else:                   # BCE-with-logits, mean over the rows of the sum over the answers (the reference's `* answers`)
            label = _r16(torch.rand(rows, N, generator=g)).to(dev())

            def loss_fn(logits, copy, loss, gs, fresh):
                ops.bce_logits_fwd_bwd(logits, N, label, loss, gscale=gs, logits_copy=copy if fresh else None)
            tloss = lambda z: F.binary_cross_entropy_with_logits(z, label) * N
        view = lambda z: full(z, N)
    else:                       # VCR's answer classifier: Linear(H, 1) on B x C rows, one live column of 64
        V = pkg("vcr.modules.resnet_vlbert_for_vcr")
        B, C, N = 2, 4, 1
        rows = B * C
        a = _lin(1, H, g, scale=4.0)
        head = Hd.Head([Hd.Drop(3002), Hd.Linear(Hd.Linear16(a), wgrad=V.one_column_wgrad(H, dev()))], seed)
        ref = [("drop", 3002), ("lin", a, None)]
        answer = torch.randint(0, C, (B,), generator=g).to(dev())
        w = 4.0
        loss_fn = V.answer_loss(answer, B, C, case == "1fc_sigmoid", w, torch.zeros(1, device=dev()))
        if case == "1fc_sigmoid":
            onehot = F.one_hot(answer, C).float().view(-1)
            tloss = lambda z: F.binary_cross_entropy_with_logits(z.view(-1), onehot, pos_weight=torch.tensor(w, device=dev())) * (w + 1) / (2 * w)
        else:
            tloss = lambda z: F.cross_entropy(z.view(B, C), answer)
        view = lambda z: full(z, 1)
    x = _r16(torch.randn(rows, H, generator=g) * 0.7).to(dev())
    return head, x, ref, loss_fn, tloss, view


def _masks(head, ref, x, p):
    """per dropout site: the scaled keep mask over the padded width the site sees, taken from the device before the step"""
    if p <= 0:
        return {}
    thr = min(int(p * 65536.0 + 0.5), 65535)
    out, w = {}, x.shape[1]
    for st in ref:
        if st[0] == "drop":
            out[st[1]] = _keep_mask(x.shape[0], w, p, head.seed, st[1]) * (65536.0 / (65536.0 - thr))
        elif st[0] == "lin":
            w = st[1].weight.shape[0]
    return out


def _torch_ref(ref, x, masks, tloss, factor):
    """-> (logits, loss, [d params in head.params() order], d x, sum |d logits|) of fp32 autograd"""
    xr = x.clone().requires_grad_(True)
    h, params = xr, []
    for st in ref:
        if st[0] == "drop":
            h = h * masks[st[1]][:, :h.shape[1]] if masks else h
        elif st[0] == "lin":
            h = F.linear(h, st[1].weight, st[1].bias)
            h = F.relu(h) if st[2] == "relu" else (F.gelu(h) if st[2] == "gelu" else h)
            params += [st[1].weight, st[1].bias]
        else:
            h = F.layer_norm(h, h.shape[1:], st[1].weight, st[1].bias, eps=1e-12)
            params += [st[1].weight, st[1].bias]
    loss = tloss(h)
    grads = torch.autograd.grad(factor * loss, params + [xr, h])
    return h.detach(), float(loss.detach()), list(grads[:-2]), grads[-2], float(grads[-1].abs().sum())


def _step(case, p, factor):
    g = torch.Generator().manual_seed(11)
    head, x, ref, loss_fn, tloss, view = _build(case, g)
    masks = _masks(head, ref, x, p)
    st = head.forward(x, p, loss_fn)
    got = dict(logits=view(st["copy"]).clone(), loss=float(st["loss"][0]))
    got["dx"], got["grads"] = head.backward(st, factor)
    torch.cuda.synchronize()
    return head, x, ref, tloss, masks, got


def _errors(name, got, want, zero_sum_bias=False):
    """prints every figure, returns the names of the checks that miss their bar.  zero_sum_bias: the last bias gradient is a sum of
    d(logits) that cancels exactly (softmax over the choices of a sample: the reference is 0 up to rounding), so its error is taken
    relative to the sum of the magnitudes of its terms"""
    logits, loss, grads, dx, dl1 = want
    bad = []
    try:
        report(name + " logits", got["logits"], logits, 2e-2, 2e-2)
    except AssertionError:
        bad.append("logits")
    e = abs(got["loss"] - loss) / abs(loss)
    print("  %s loss %.6f vs %.6f rel %.3e" % (name, got["loss"], loss, e))
    bad += ["loss"] * (not e < 1e-2)
    for k, (a, b) in enumerate(zip(got["grads"] + [got["dx"]], grads + [dx])):
        e = rel_fro(a, b) if not (zero_sum_bias and k == len(grads) - 1) else float((a - b).norm()) / dl1
        print("  %s d %s rel-fro %.3e" % (name, "x" if k == len(grads) else "param %d" % k, e))
        bad += ["d%d" % k] * (not e < 5e-2)
    return bad


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("p", P_DROP)
@pytest.mark.parametrize("case", ["2fc", "1fc_sigmoid", "1fc_softmax", "mlm", "reg"])
def test_head_matches_torch_autograd(case, p, factor):
    """2fc: K padded 100 -> 128, outputs 70 -> 128, two dropout sites.  1fc_*: 8 = 2 x 4 rows, one live column of 64, the weighted BCE
    (pos_weight 4) / the softmax CE through the [B, 64] staging buffer.  mlm: dense + GELU + LayerNorm -> drop -> linear.  reg: 37 rows
    in a row capacity of 64, 81 classes padded to 128, CE.  factor 0.37 takes the re-derive-d(logits)-from-the-kept-copy branch."""
    head, x, ref, tloss, masks, got = _step(case, p, factor)
    assert len(got["grads"]) == len(head.params()) and got["dx"].shape == x.shape
    bad = _errors("head %s p=%g g=%g" % (case, p, factor), got, _torch_ref(ref, x, masks, tloss, factor), zero_sum_bias=case == "1fc_softmax")
    assert not bad, bad


def test_head_test_sees_a_swapped_dropout_tag():
    """the 2fc case at p = 0.3 against the torch reference with the two sites' masks swapped: it must miss the bar, or a backward
    replaying the wrong tag would pass the test above"""
    head, x, ref, tloss, masks, got = _step("2fc", 0.3, 1.0)
    assert masks[2001].shape == masks[2002].shape == (5, 128) and not torch.equal(masks[2001], masks[2002])
    swapped = {2001: masks[2002], 2002: masks[2001]}
    bad = _errors("head 2fc swapped masks", got, _torch_ref(ref, x, swapped, tloss, 1.0))
    assert any(k.startswith("d") for k in bad), bad
