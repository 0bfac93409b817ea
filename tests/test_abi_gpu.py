"""The branches of the one-symbol-per-operation C ABI that no training path takes (-m gpu): the combinations of the optional arguments
that the library refuses, and the empty run of the optimizer step with and without a loss scaler."""
import pytest
import torch

from tests.gpu_util import dev, pkg

pytestmark = pytest.mark.gpu
VLB_ERR_ARG = -1
GROWTH_INTERVAL, UNSKIPPED = 3, 4      # VLB_SCALER_* slots (include/vlbert_hip.h)


def bits(t):
    return t.clone().view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_refused_combinations_of_the_optional_loss_arguments():
    """The fp32 losses take a device scale only with the counters (the kernels without them have no such argument), and the two-group
    loss takes its counter pair whole.  The library answers VLB_ERR_ARG, names the entry point and launches nothing: the logits and
    every output keep their bits.  The ops wrappers refuse the same calls before they reach the library."""
    ops, L = pkg("ops"), pkg("_lib")
    h, d = L.load(), dev()
    rows, ld, V = 2, 8, 5
    x = torch.randn(rows, ld, device=d)
    x16 = x.to(ops.BF16)
    labels = torch.tensor([1, 3], dtype=torch.int64, device=d)
    target = torch.full((rows, ld), 1.0 / V, device=d)
    out = torch.full((8,), 7.0, device=d)      # counts | loss | loss1 | tsum[2] | row_loss[2], all expected to stay 7
    counts, loss, loss1, tsum, row_loss = out[0:1], out[1:2], out[2:3], out[3:5], out[5:7]
    dscale = torch.full((1,), 2.0, device=d)
    acc = torch.zeros(2, dtype=torch.int64, device=d)
    x0, x16_0, s = bits(x), bits(x16), ops._stream()
    p = lambda t: t.data_ptr()

    refused = {
        "vlb_ce_f32_fwd_bwd": lambda: h.vlb_ce_f32_fwd_bwd(p(x), ld, rows, V, p(labels), p(counts), 1.0, p(dscale), p(loss), p(row_loss), None,
                                                           0, None, s),
        "vlb_ce_f32_fwd_bwd_compact": lambda: h.vlb_ce_f32_fwd_bwd_compact(p(x), ld, rows, V, p(labels), p(counts), p(counts), 1.0, p(dscale),
                                                                           p(loss), p(loss1), p(row_loss), None, None, s),
        "vlb_soft_ce_f32_fwd_bwd": lambda: h.vlb_soft_ce_f32_fwd_bwd(p(x), ld, rows, V, p(target), ld, p(tsum), p(counts), 1.0, p(dscale),
                                                                     p(loss), p(row_loss), None, 0, None, s),
        "vlb_ce_fwd_bwd_compact": lambda: h.vlb_ce_fwd_bwd_compact(p(x16), ld, rows, V, p(labels), p(counts), p(counts), 1.0, None, p(loss),
                                                                   p(loss1), p(acc), None, s),
    }
    for name, call in refused.items():
        assert call() == VLB_ERR_ARG, name
        assert name + ":" in h.vlb_last_error().decode(), (name, h.vlb_last_error())

    for call in (lambda: ops.ce_f32_fwd_bwd(x, V, labels, counts, loss, row_loss=row_loss, dscale=dscale),
                 lambda: ops.ce_f32_fwd_bwd_compact(x, V, labels, counts, counts, loss, loss1, row_loss=row_loss, dscale=dscale),
                 lambda: ops.soft_ce_f32_fwd_bwd(x, V, target, tsum, counts, loss, row_loss=row_loss, dscale=dscale),
                 lambda: ops.ce_fwd_bwd_compact(x16, V, labels, counts, counts, loss, loss1, acc=acc)):
        with pytest.raises(ValueError):
            call()

    torch.cuda.synchronize()
    assert torch.equal(bits(x), x0) and torch.equal(bits(x16), x16_0)
    assert torch.equal(out, torch.full_like(out, 7.0)) and not acc.any()


@pytest.mark.parametrize("g16", [False, True])
def test_adamw_step_over_an_empty_run(g16):
    """p.numel() == 0.  Without a scaler the call is no step: it returns before adam_advance_kernel, so the step count and the pending
    sum of squares stay.  With one, scaler_advance_kernel runs all the same: a finite sumsq counts the step (state[5] + 1), sumsq = 0,
    and -- only when asked to apply the scaler's rule -- one more clean step is counted (unskipped + 1, below the growth interval)."""
    ops, Ls = pkg("ops"), pkg("loss_scale")
    d = dev()
    e32 = torch.empty(0, device=d)
    g = torch.empty(0, dtype=ops.BF16 if g16 else torch.float32, device=d)

    def state():
        return torch.tensor([1e-3, 0.9, 0.999, 1e-6, 1e-2, 5.0, 1.0, 3.0], device=d)

    st = state()
    ops.adamw_step(e32, g, e32, e32, None, st)
    assert torch.equal(bits(st), bits(state()))

    for update in (True, False):
        st, sc = state(), Ls.LossScaler(Ls.DynamicLossScale(init_scale=1024.0), d)
        before = sc.state.clone()
        ops.adamw_step(e32, g, e32, e32, None, st, scaler=sc.state, update_scaler=update)
        want = state()
        want[5], want[7] = 6.0, 0.0
        assert torch.equal(bits(st), bits(want))
        if update:
            assert before[UNSKIPPED] + 1 < before[GROWTH_INTERVAL]
            before[UNSKIPPED] += 1
        assert torch.equal(bits(sc.state), bits(before))
