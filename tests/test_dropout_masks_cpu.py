"""The oracle's dropout-mask hook (oracle/vlbert_oracle.py `dropout`) and the test-side restatement of the engine's dropout layout
(tests/gpu_util.EngineDropoutMasks) that the train-mode GPU parity tests hand to it -- no GPU needed."""
import numpy as np
import pytest
import torch

from oracle import vlbert_oracle as O
from tests.gpu_util import EngineDropoutMasks, TAG_DOWNSAMPLE, TAG_EMBED, drop_scale, drop_thr, keep_mask, pkg, rng_advance


def _small(p, multitask=False):
    """A small model (H = 64, 2 layers) and a ragged batch with masked regions and one sample without any valid box."""
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, vocab_size=1024,
                         visual_region_classes=40, max_position_embeddings=64, hidden_dropout_prob=p, attention_probs_dropout_prob=p,
                         obj_downsample_dropout=p, multitask=multitask)
    params = O.init_params(cfg, seed=3)
    batch = list(syn.make_batch(3, 12, 6, vocab_size=1024, region_classes=40, seed=4, ragged=True))
    batch[0][1] = -2.0
    batch[5][1] = 0
    batch[6][1] = 0
    if multitask:
        batch += list(syn.make_aux_text(2, 9, vocab_size=1024, seed=5))
    return cfg, params, tuple(batch)


class _Ones:
    def __init__(self):
        self.sites = []

    def __call__(self, site, prob, shape, layer=None, inds=None):
        self.sites.append((site, layer))
        return torch.ones(shape)


@pytest.mark.parametrize("multitask", [False, True])
def test_all_ones_masks_reproduce_eval_mode_bit_for_bit(multitask):
    """train=True with a hook that keeps everything (scale 1) is train=False exactly: the hook replaces torch's RNG and nothing
    else; every dropout site of the reference asks the hook once."""
    cfg, params, batch = _small(0.3, multitask)
    ones = _Ones()
    _, loss_t, g_t, n_t = O.loss_and_grads(params, cfg, batch, train=True, drop_hook=ones)
    _, loss_e, g_e, n_e = O.loss_and_grads(params, cfg, batch, train=False)
    assert torch.equal(loss_t, loss_e) and n_t == n_e
    for k in g_e:
        assert torch.equal(g_t[k], g_e[k]), k
    want = [("obj_downsample", None), ("embedding", None)]
    for l in range(cfg.num_hidden_layers):
        want += [("attention_probs", l), ("attention_output", l), ("ffn_output", l)]
    assert ones.sites == want


def test_default_train_mode_still_uses_torch_dropout():
    """Without a hook, train=True draws torch's masks as before (two draws differ, a re-seeded draw repeats)."""
    cfg, params, batch = _small(0.1)
    torch.manual_seed(0)
    a = O.loss_and_grads(params, cfg, batch, train=True)[1]
    b = O.loss_and_grads(params, cfg, batch, train=True)[1]
    torch.manual_seed(0)
    c = O.loss_and_grads(params, cfg, batch, train=True)[1]
    assert not torch.equal(a, b) and torch.equal(a, c)


def test_engine_layout_masks_at_chosen_indices():
    """Each site's mask at a few hand-placed elements is keep_mask(seed, tag, index, thr) x the device scale, with the index
    formulas of the engine's kernels (S = T + R + 1 of the engine, not the oracle's max_length)."""
    seed, S, R, nh, H, p = 0x1234567, 43, 10, 12, 768, 0.1
    thr = drop_thr(p)
    sc = np.float32(65536.0) / np.float32(65536.0 - thr)
    assert abs(sc - drop_scale(thr)) < 1e-6
    m = EngineDropoutMasks(seed, S, R, nh)
    Sp = 64
    mf = EngineDropoutMasks(seed, S, R, nh, Sp=Sp)

    def want(tag, idx):
        return float(keep_mask(seed, tag, np.array([idx]), thr)[0]) * float(sc)

    emb = m("embedding", p, (5, 40, H))                                  # b over B + B_aux, s < max_length = 40
    for b, s, c in ((0, 0, 0), (4, 39, 767), (2, 17, 333)):
        assert float(emb[b, s, c]) == want(TAG_EMBED, (b * S + s) * H + c)
    att = m("attention_probs", p, (5, nh, 40, 40), layer=3)
    fatt = mf("attention_probs", p, (5, nh, 40, 40), layer=3)
    for b, h, q, k in ((0, 0, 0, 1), (4, 11, 39, 38), (1, 5, 7, 22)):
        assert float(att[b, h, q, k]) == want(3 * 8 + 0, ((b * nh + h) * S + q) * S + k)
        assert float(fatt[b, h, q, k]) == want(3 * 8 + 0, ((b * nh + h) * S + q) * Sp + k)
    for site, off in (("attention_output", 1), ("ffn_output", 2)):
        t = m(site, p, (5, 40, H), layer=11)
        for b, s, c in ((0, 0, 1), (4, 39, 700), (3, 1, 64)):
            assert float(t[b, s, c]) == want(11 * 8 + off, (b * S + s) * H + c)
    inds = torch.tensor([[0, 0], [0, 3], [2, 0], [4, 9]])
    ds = m("obj_downsample", p, (4, 4096), inds=inds)
    for k, e in ((0, 0), (1, 2047), (2, 2048), (3, 4095)):
        b, r = inds[k].tolist()
        assert float(ds[k, e]) == want(TAG_DOWNSAMPLE, (b * R + r) * 4096 + e)
    # masked_colsum reads the feature half: row_elems 4096, col_off 2048 -- the same draws as the forward's columns 2048..4095
    col = 17
    assert float(ds[3, 2048 + col]) == want(TAG_DOWNSAMPLE, (9 + 4 * R) * 4096 + 2048 + col)


def test_rng_advance_restatement():
    """rng_advance: hash32(seed + 0x9E3779B9) | 1 in uint32 arithmetic (vl-bert_amd/csrc/optim.hip:255)."""
    def hash32(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    for s in (0, 1, 2469, 0x7FFFFFFF, 0xFFFFFFFF, 0x9E3779B9):
        assert rng_advance(s) == hash32((s + 0x9E3779B9) & 0xFFFFFFFF) | 1
        assert rng_advance(s) & 1 and 0 <= rng_advance(s) <= 0xFFFFFFFF
    assert rng_advance(2469) != rng_advance(rng_advance(2469))


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_kept_fraction_and_mean(p):
    """About 1 - p of the elements survive, scaled so the mask's mean is ~1 (inverted dropout)."""
    m = EngineDropoutMasks(99 * 2 + 1, 101, 36, 12)
    t = m("attention_probs", p, (6, 12, 101, 101), layer=5).numpy()
    kept = float((t > 0).mean())
    assert abs(kept - (1.0 - p)) < 2e-3, kept
    assert abs(float(t.mean()) - 1.0) < 3e-3
    assert np.all((t == 0) | (t == np.float32(m.scale(m.thr(p)))))


def test_wrong_seed_masks_miss_the_bar_on_the_oracle_alone():
    """The margin the train-mode GPU tests assert (tests/test_engine_gpu.py WRONG_SEED_FACTOR): for config a, the oracle under the
    masks of seed s and of advance(s) differ on the worst gradient tensor by far more than 5 x the per-tensor bar of that test, at
    the smaller p.  A test whose two mask sets were this close could not tell a wrong mask from rounding."""
    from tests.test_engine_gpu import WRONG_SEED_FACTOR, dropout_case_a, grad_errors
    cfg, params, batch = dropout_case_a(0.1)
    s = 1234 * 2 + 1                                    # PretrainEngine's initial seed for seed=1234
    S, R = batch[2].shape[1] + batch[0].shape[1] + 1, batch[0].shape[1]
    _, _, ga, na = O.loss_and_grads(params, cfg, batch, train=True, drop_hook=EngineDropoutMasks(s, S, R, cfg.num_attention_heads))
    _, _, gb, _ = O.loss_and_grads(params, cfg, batch, train=True,
                                   drop_hook=EngineDropoutMasks(rng_advance(s), S, R, cfg.num_attention_heads))
    worst = grad_errors(gb, ga, na)
    print("oracle vs oracle, masks of s and advance(s): worst %.3e (%s)" % worst[0])
    assert worst[0][0] >= WRONG_SEED_FACTOR * 0.12
