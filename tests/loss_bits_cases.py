"""Inputs and launches of the loss-kernel bit fixture (tests/golden/loss_bits/loss_bits_small.npz): every entry point of csrc/loss.hip
that a row kernel stands behind, in every DS (device loss scale) x ACC (training-time counters) x logits_copy form, on inputs made here
from a numpy seed.  tools/make_loss_bits_golden.py runs the cases on a build of the library and stores what it wrote;
tests/test_loss_bits_gpu.py runs them again and compares bit patterns.  No reference arithmetic in here: the only assertions are the
ones that need none (a kept copy is the input, a row without a label is zero, a forward-only launch leaves the logits alone).

run(name) -> {key: numpy array}.  Gradients are int16 bit patterns of the library's 16-bit type -- the whole d(logits), padding
included, at the small shapes, the labelled rows alone at the wide ones --, counters int64, counts float32, a
loss slot the int32 bit pattern of its float -- stored only where exactly ONE row adds to it (elsewhere the float atomicAdd order is
free).  A DS form gets gscale = G and the device scalar D, its static twin the host product G * D (exact: both are powers of two times
3), so the two are the same request.
"""
import itertools

import numpy as np
import torch

from tests.gpu_util import act_dtype, dev, pkg

SEED = 20240611
G, D = 0.75, 1024.0
PAD = 64.0            # pad columns of the logits: would win every argmax and swamp every sum if they were read
SENTINEL = -3.0       # what a kept-copy buffer holds before the launch
V_S, LD_S = 37, 40                      # ragged 8-wide tail
V_W, LD_W = 30522, 30528
C_S, LDC_S = 5, 8
C_W, LDC_W = 1601, 1664                 # the engine's Cp: visual_region_classes rounded up to 64


def rng(case):
    return np.random.default_rng([SEED, sum(map(ord, case))])


def logits16(r, rows, V, ld, scale=3.0):
    """Rounded to the 16-bit type under test, off any coarse grid; pad columns hold PAD."""
    x = (r.standard_normal((rows, ld)) * scale).astype(np.float32)
    x[:, V:] = PAD
    return torch.from_numpy(x).to(act_dtype())


def bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy()


def fbits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def zf(n=1):
    return torch.zeros(n, dtype=torch.float32, device=dev())


def counters():
    return torch.tensor([7, 11], dtype=torch.int64, device=dev())


def scale_args(ds):
    return dict(gscale=G, dscale=torch.tensor([D], dtype=torch.float32, device=dev())) if ds else dict(gscale=G * D, dscale=None)


def copy_buf(x, copy):
    return torch.full_like(x, SENTINEL) if copy else None


def check_copy(cp, x0, V):
    if cp is not None:
        assert torch.equal(cp[:, :V].view(torch.int16), x0[:, :V].view(torch.int16)) and bool((cp[:, V:] == SENTINEL).all())


def form(ds, acc, copy=None):
    return "ds%d_acc%d" % (ds, acc) + ("" if copy is None else "_copy%d" % copy)


# ---- hard labels ------------------------------------------------------------------------------------------------------------------
def hard_plain(case, V, ld, labels, tie_rows=()):
    ops, r = pkg("ops"), rng(case)
    x0 = logits16(r, len(labels), V, ld)
    for row, cols in tie_rows:                  # a tie at the maximum: the lowest column is the argmax
        x0[row, list(cols)] = 9.0
    x0 = x0.to(dev())
    lab = torch.tensor(labels, dtype=torch.int64, device=dev())
    valid = [i for i, l in enumerate(labels) if 0 <= l < V]
    out = {}
    for ds, acc, copy in itertools.product((0, 1), repeat=3):
        x, counts, loss, a, cp = x0.clone(), zf(), zf(), counters(), copy_buf(x0, copy)
        ops.ce_fwd_bwd(x, V, lab, counts, loss, logits_copy=cp, acc=a if acc else None, **scale_args(ds))
        check_copy(cp, x0, V)
        rest = [i for i in range(len(labels)) if i not in valid]
        assert not bits(x[rest]).any()
        k = "%s/%s/" % (case, form(ds, acc, copy))
        out[k + "grad"] = bits(x[valid] if V == V_W else x)
        out[k + "counts"] = counts.cpu().numpy()
        if acc:
            out[k + "acc"] = a.cpu().numpy()
        if len(valid) == 1:
            out[k + "loss"] = fbits(loss)
    return out


def hard_small():
    # labels: ignore_index, out of range, first and last column, a tie won by the label (columns 5, 20), a tie lost (label 30 > 12)
    return hard_plain("hard_small", V_S, LD_S, [-1, V_S, 0, V_S - 1, 5, 30], tie_rows=((4, (5, 20)), (5, (12, 30))))


def hard_wide():
    # the out-of-range label counts in the divisor (label >= 0) and adds no loss: n_valid = 2, one row writes the loss slot
    return hard_plain("hard_wide", V_W, LD_W, [V_W, -1, V_W - 1])


def hard_compact():
    ops, case, r = pkg("ops"), "hard_compact", rng("hard_compact")
    x0 = logits16(r, 6, V_S, LD_S).to(dev())
    lab = torch.tensor([3, V_S - 1, 0, -1, -1, -1], dtype=torch.int64, device=dev())      # count0 = 2, count1 = 1, padding behind
    c0, c1 = torch.tensor([2.0], device=dev()), torch.tensor([1.0], device=dev())
    out = {}
    for ds, acc in itertools.product((0, 1), repeat=2):
        x, l0, l1, a0, a1 = x0.clone(), zf(), zf(), counters(), counters()
        ops.ce_fwd_bwd_compact(x, V_S, lab, c0, c1, l0, l1, acc=a0 if acc else None, acc1=a1 if acc else None, **scale_args(ds))
        assert not bits(x[3:]).any()
        k = "%s/%s/" % (case, form(ds, acc))
        out[k + "grad"] = bits(x)
        out[k + "loss1"] = fbits(l1)            # group 1 has one row
        if acc:
            out[k + "acc"] = torch.stack([a0, a1]).cpu().numpy()
    return out


B_RW, T_RW, SPLIT_RW = 3, 5, 2


def rowweight_inputs(case):
    """B=3 samples of T=5 rows: sample 0 one label (alone in group 0: its loss slot has one writer), sample 1 none (and an out-of-range
    label, which no count takes), sample 2 three (group 1).  -> logits, labels, weights of vlb_sample_norm_weights."""
    ops, r = pkg("ops"), rng(case)
    x0 = logits16(r, B_RW * T_RW, V_S, LD_S).to(dev())
    labels = [-1, -1, 7, -1, -1] + [-1, V_S, -1, -1, -1] + [0, -1, V_S - 1, -1, 21]
    lab = torch.tensor(labels, dtype=torch.int64, device=dev())
    w, c0, c1 = zf(B_RW), zf(), zf()
    ops.sample_norm_weights(w, T_RW, labels=lab, V=V_S, B_split=SPLIT_RW, count0=c0, count1=c1)
    return x0, lab, labels, w, {"w": fbits(w), "counts": torch.cat([c0, c1]).cpu().numpy()}


def hard_rowweight_full():
    ops, case = pkg("ops"), "hard_rowweight_full"
    x0, lab, labels, w, out = rowweight_inputs(case)
    out = {case + "/" + k: v for k, v in out.items()}
    valid = [i for i, l in enumerate(labels) if 0 <= l < V_S]
    rest = [i for i in range(len(labels)) if i not in valid]
    for ds, acc, copy in itertools.product((0, 1), repeat=3):
        x, l0, l1, a0, a1, cp = x0.clone(), zf(), zf(), counters(), counters(), copy_buf(x0, copy)
        ops.ce_rowweight_fwd_bwd(x, V_S, lab, w, T_RW, l0, B_split=SPLIT_RW, loss_out1=l1, logits_copy=cp, acc=a0 if acc else None,
                                 acc1=a1 if acc else None, **scale_args(ds))
        check_copy(cp, x0, V_S)
        assert not bits(x[rest]).any()
        k = "%s/%s/" % (case, form(ds, acc, copy))
        out[k + "grad"] = bits(x)
        out[k + "loss0"] = fbits(l0)
        if acc:
            out[k + "acc"] = torch.stack([a0, a1]).cpu().numpy()
    x, l0, l1, a0, a1 = x0.clone(), zf(), zf(), counters(), counters()
    ops.ce_rowweight_eval(x, V_S, lab, w, T_RW, l0, a0, B_split=SPLIT_RW, loss_out1=l1, acc1=a1)
    assert torch.equal(x.view(torch.int16), x0.view(torch.int16))          # BWD = false: the logits are only read
    out[case + "/eval/loss0"], out[case + "/eval/acc"] = fbits(l0), torch.stack([a0, a1]).cpu().numpy()
    return out


def hard_rowweight_compact():
    ops, case, cap = pkg("ops"), "hard_rowweight_compact", 8
    xf, lab, labels, w, out = rowweight_inputs(case)
    out = {case + "/" + k: v for k, v in out.items()}
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev())
    sel_pos, sel_src, labels_c, over = i32(cap, -7), i32(cap, -7), torch.full((cap,), -7, dtype=torch.int64, device=dev()), i32(1)
    ops.mlm_compact(lab, torch.arange(B_RW * T_RW, dtype=torch.int32, device=dev()), SPLIT_RW * T_RW, V_S, sel_pos, sel_src, labels_c, zf(),
                    zf(), over)
    n = sum(0 <= l < V_S for l in labels)
    assert sel_pos[n:].tolist() == [-1] * (cap - n) and int(over) == 0
    x0 = logits16(rng(case + "/pad"), cap, V_S, LD_S).to(dev())               # the rows behind the list hold logits too: none may be read
    x0[:n] = xf[sel_pos[:n].long()]
    out[case + "/sel_pos"] = sel_pos.cpu().numpy()
    for ds, acc in itertools.product((0, 1), repeat=2):
        x, l0, l1, a0, a1 = x0.clone(), zf(), zf(), counters(), counters()
        ops.ce_rowweight_fwd_bwd(x, V_S, labels_c, w, T_RW, l0, B_split=SPLIT_RW, loss_out1=l1, sel_pos=sel_pos, acc=a0 if acc else None,
                                 acc1=a1 if acc else None, **scale_args(ds))
        assert not bits(x[n:]).any()
        k = "%s/%s/" % (case, form(ds, acc))
        out[k + "grad"] = bits(x)
        out[k + "loss0"] = fbits(l0)
        if acc:
            out[k + "acc"] = torch.stack([a0, a1]).cpu().numpy()
    x, l0, l1, a0, a1 = x0.clone(), zf(), zf(), counters(), counters()
    ops.ce_rowweight_eval(x, V_S, labels_c, w, T_RW, l0, a0, B_split=SPLIT_RW, loss_out1=l1, acc1=a1, sel_pos=sel_pos)
    assert torch.equal(x.view(torch.int16), x0.view(torch.int16))
    out[case + "/eval/loss0"], out[case + "/eval/acc"] = fbits(l0), torch.stack([a0, a1]).cpu().numpy()
    return out


# ---- soft labels ------------------------------------------------------------------------------------------------------------------
def soft(case, C, ld, B, R, invalid):
    """B * R rows; the rows of `invalid` carry half a distribution (sum 0.5: off by more than 0.1), the others a full one."""
    ops, r = pkg("ops"), rng(case)
    rows = B * R
    x0 = logits16(r, rows, C, ld).to(dev())
    t = r.standard_normal((rows, C)).astype(np.float64) * 2
    t = np.exp(t - t.max(1, keepdims=True))
    t = (t / t.sum(1, keepdims=True)).astype(np.float32)
    t[list(invalid)] *= 0.5
    tgt = torch.from_numpy(t).to(dev())
    valid = [i for i in range(rows) if i not in invalid]
    out = {}
    for weighted, (ds, acc, copy) in itertools.product((0, 1), itertools.product((0, 1), repeat=3)):
        x, tsum, counts, loss, a, cp = x0.clone(), zf(rows), zf(), zf(), counters(), copy_buf(x0, copy)
        kw = dict(logits_copy=cp, acc=a if acc else None, **scale_args(ds))
        if weighted:
            w = zf(B)
            ops.soft_ce_rowweight_fwd_bwd(x, C, tgt, tsum, w, R, counts, loss, **kw)
        else:
            ops.soft_ce_fwd_bwd(x, C, tgt, tsum, counts, loss, **kw)
        check_copy(cp, x0, C)
        assert not bits(x[list(invalid)]).any() and not bits(x[:, C:]).any()
        k = "%s/%s/%s/" % (case, "rowweight" if weighted else "plain", form(ds, acc, copy))
        out[k + "grad"] = bits(x[valid][:, :C] if C == C_W else x)
        out[k + "counts"] = counts.cpu().numpy()
        if weighted:
            out[k + "w"] = fbits(w)
        if len(valid) == 1:
            out[k + "loss"] = fbits(loss)
        if acc:
            out[k + "acc"] = a.cpu().numpy()
    x, tsum, w, counts, loss, a = x0.clone(), zf(rows), zf(B), zf(), zf(), counters()
    ops.soft_ce_rowweight_eval(x, C, tgt, tsum, w, R, counts, loss, a)
    assert torch.equal(x.view(torch.int16), x0.view(torch.int16))
    out[case + "/rowweight/eval/acc"], out[case + "/rowweight/eval/counts"] = a.cpu().numpy(), counts.cpu().numpy()
    if len(valid) == 1:
        out[case + "/rowweight/eval/loss"] = fbits(loss)
    return out


def soft_small():
    return soft("soft_small", C_S, LDC_S, 2, 4, invalid=(1, 5, 6, 7))      # sample 0: three valid regions, sample 1: one


def soft_wide():
    return soft("soft_wide", C_W, LDC_W, 1, 4, invalid=(2,))


def soft_single():
    return soft("soft_single", C_W, LDC_W, 1, 4, invalid=(0, 1, 3))      # one valid row: the loss slot has one writer and is compared


CASES = {f.__name__: f for f in (hard_small, hard_wide, hard_compact, hard_rowweight_full, hard_rowweight_compact, soft_small, soft_wide,
                                 soft_single)}


def run(name):
    out = CASES[name]()
    torch.cuda.synchronize()
    return out


def precision():
    return "f16" if act_dtype() == torch.float16 else "bf16"
