"""Sequences of 257..512 positions through the engine and the module mirror (-m gpu): PretrainEngine(max_seq=512) runs attention on the
streaming kernels of vl-bert_amd/csrc/attention_long.hip; seq_layout, the embedding forward / backward, the lse and mask buffers see
more than 256 rows per sample.  Oracle parity with the bars of tests/test_engine_gpu.py::check_against_oracle, a replayed step graph
against the eager step, and the VisualLinguisticBert mirror (packed-sequence call form) against the oracle."""
import pytest
import torch

from oracle import vlbert_oracle as O
from tests.gpu_util import dev, pkg, report
from tests.test_engine_gpu import _module_config, check_against_oracle, make_engine, rel_fro

pytestmark = pytest.mark.gpu
LONG = {"max_seq": 512}


def test_sequence_length_limits_of_the_engine():
    E = pkg("engine")
    mc = E.ModelConfig(num_hidden_layers=1)
    with pytest.raises(ValueError, match="max_seq"):                      # a default engine stops at 256 and says how to go further
        E.PretrainEngine(mc, 1, 156, 100, device="cuda:0")
    with pytest.raises(ValueError, match="max_seq"):
        E.PretrainEngine(mc, 1, 16, 4, device="cuda:0", max_seq=600)
    with pytest.raises(ValueError, match="max_seq"):
        E.PretrainEngine(mc, 1, 16, 4, device="cuda:0", max_seq=128)
    with pytest.raises(ValueError, match="512"):                          # T + R + 1 = 513
        E.PretrainEngine(mc, 1, 412, 100, device="cuda:0", max_seq=512)
    with pytest.raises(ValueError, match="fp32 encoder"):                 # the fp32 softmax kernels stay at 256 keys
        E.PretrainEngine(mc, 1, 200, 100, device="cuda:0", max_seq=512, encoder_fp32=True)


def test_engine_s301_vs_oracle():
    """S = 200 + 100 + 1 = 301: three key / query blocks, the last one of 45 rows; ragged batch, 2 layers, eval."""
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(num_hidden_layers=2, max_position_embeddings=512)
    params = O.init_params(cfg, seed=41)
    batch = syn.make_batch(2, 200, 100, seed=42, ragged=True)
    check_against_oracle("S=301", cfg, params, batch, engine_kw=LONG)


def test_engine_s385_train_mode_vs_oracle():
    """S = 284 + 100 + 1 = 385 (one row in the fourth block) with every dropout on: the forward and both backward roles regenerate the
    attention masks the oracle is handed; the oracle under another seed's masks must miss the bars (check_against_oracle)."""
    syn = pkg("synthetic")
    p = 0.1
    cfg = O.VLBertConfig(num_hidden_layers=2, max_position_embeddings=512, hidden_dropout_prob=p, attention_probs_dropout_prob=p,
                         obj_downsample_dropout=p)
    params = O.init_params(cfg, seed=43)
    batch = syn.make_batch(2, 284, 100, seed=44, ragged=True)
    check_against_oracle("S=385 train", cfg, params, batch, engine_kw=LONG, train=True)


def test_engine_s512_vs_oracle():
    """S = 411 + 100 + 1 = 512: the longest sequence (every position row of a 512-row table is reachable), 1 layer, ragged batch."""
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(num_hidden_layers=1, max_position_embeddings=512)
    params = O.init_params(cfg, seed=45)
    batch = syn.make_batch(2, 411, 100, seed=46, ragged=True)
    check_against_oracle("S=512", cfg, params, batch, engine_kw=LONG)


def test_step_graph_replay_equals_the_eager_step_at_s301():
    """One optimizer step replayed from make_step_graph() against an eager shadow step from the same state (the pattern of
    tests/test_loss_scale_f16_gpu.py): d(logits), the reproducible gradients, and -- with the atomically accumulated gradients
    copied over -- weights and optimizer state, bit for bit; the loss scalars up to the order of their atomic row sums (see below).
    The attention launchers allocate nothing and never synchronise."""
    E, syn = pkg("engine"), pkg("synthetic")
    B, T, Rg = 2, 200, 100
    batch = [t.to(dev()) for t in syn.make_batch(B, T, Rg, seed=47, ragged=True)]

    def engine():
        eng = E.PretrainEngine(E.ModelConfig(num_hidden_layers=2), B, T, Rg, device="cuda:0", train=True, lr=1e-4, weight_decay=1e-2,
                               max_grad_norm=1.0, seed=5, max_seq=512)
        eng.init_random(seed=3)
        eng.set_batch(*batch)
        return eng

    def bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.element_size() == 2 else t)

    def carried(e):
        return [e.P.master, e.P.m, e.P.v, e.adam, e.seed]

    eng, shadow = engine(), engine()
    assert eng.S == 301
    eng.train_step()                                          # (make_step_graph wants one eager step first)
    torch.cuda.synchronize()
    step = eng.make_step_graph()
    # the tied word-embedding table takes the embedding backward's atomic scatter, the obj_downsample weight gradient is computed from
    # d(obj_reps), which that backward sums with atomics: not reproducible run to run
    exact = set(eng._gemm_weight_names()) - {"vlbert.word_embeddings.weight", "image_feature_extractor.obj_downsample.1.weight"}
    for i in range(2):
        for dst, src in zip(carried(shadow), carried(eng)):
            dst.copy_(src)
        shadow._weights_dirty = True
        step()
        shadow.zero_grad(); shadow.forward(True); shadow.backward(True)
        torch.cuda.synchronize()
        # The loss kernels add one term per labelled row to the loss scalar with a float atomic (csrc/loss.hip), so the SUM depends on
        # the order the rows retire in, run to run, eager or replayed (measured here: 3 ulp on the MVRC loss of 200 rows).  What the
        # terms are computed from -- the logits -- must be equal bit for bit; the sums may differ by the reordering of n fp32 adds:
        # |diff| <= n * 2^-24 * sum |term| = n * 2^-24 * loss (every term is a non-negative cross-entropy).
        n_rows = max(eng.BT, eng.BR)
        for k in range(4):
            a, b = float(eng.losses[k]), float(shadow.losses[k])
            assert abs(a - b) <= n_rows * 2.0 ** -24 * abs(b), "replay %d: loss %d differs: %r vs %r" % (i, k, a, b)
        for a, b in ((eng.mlm_logits, shadow.mlm_logits), (eng.mvrc_logits, shadow.mvrc_logits)):
            assert torch.equal(bits(a), bits(b)), "replay %d: d(logits) differ from the eager step's" % i
        for (n, a), b in zip(eng.g32.items(), shadow.g32.values()):
            if n in exact:
                assert torch.equal(bits(a), bits(b)), "replay %d: gradient of %s differs from the eager step's" % (i, n)
        shadow.P.grad.copy_(eng.P.grad)
        shadow.optimizer_step()
        torch.cuda.synchronize()
        for name, a, b in zip(("master", "m", "v", "adam", "seed"), carried(eng), carried(shadow)):
            assert torch.equal(bits(a), bits(b)), "replay %d: %s differs" % (i, name)
        assert torch.equal(bits(eng.P.w16), bits(shadow.P.w16)), "replay %d: the 16-bit weights differ" % i
    assert step.n_graphs == 1 and step.n_calls == 0
    lv = eng.loss_values()
    assert all(v == v and abs(v) < 1e30 for v in lv.values()), lv


def test_module_mirror_packed_sequence_at_s281_vs_oracle():
    """VisualLinguisticBert (no heads), T = 180, R = 100 -> S = 281, the call form that returns the packed sequence: values and the
    gradients of both embedding inputs and of an encoder weight against the oracle, with the bars of
    test_module_api_hidden_states_match_oracle."""
    VL = pkg("common.visual_linguistic_bert")
    cfg = O.VLBertConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=512,
                         max_position_embeddings=512, visual_region_classes=50)
    B, T, Rg, H = 2, 180, 100, cfg.hidden_size
    full = O.init_params(cfg, seed=51)
    g = torch.Generator().manual_seed(52)
    ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g)
    tlen, nobj = torch.tensor([T, 131]), torch.tensor([77, Rg])            # ragged: neither sample fills both parts
    text_mask = torch.arange(T)[None, :] < tlen[:, None]
    obj_mask = torch.arange(Rg)[None, :] < nobj[:, None]
    ids = ids * text_mask
    types = torch.zeros_like(ids)
    text_vis = torch.randn((B, T, H), generator=g)
    obj_vl = torch.randn((B, Rg, 2 * H), generator=g)
    net = VL.VisualLinguisticBert(_module_config(cfg)["NETWORK"]["VLBERT"])
    net.load_state_dict({k[len("vlbert."):]: v for k, v in full.items()
                         if k.startswith("vlbert.") and not k.startswith(("vlbert.mlm_head.", "vlbert.mvrc_head."))})
    net.eval()
    to = lambda t: t.to(dev())
    tv, ovl = to(text_vis).requires_grad_(True), to(obj_vl).requires_grad_(True)
    seq, pooled = net(to(ids), to(types), tv, to(text_mask), ovl, to(obj_mask), output_all_encoded_layers=False)
    assert pooled is None
    eng = next(iter(net._engines.values()))
    assert eng.S > 256 and eng.max_seq == 512, (eng.S, eng.max_seq)
    p = {k: v.clone().requires_grad_(True) for k, v in full.items()}
    tvc, ovlc = text_vis.clone().requires_grad_(True), obj_vl.clone().requires_grad_(True)
    ref = O.vlbert_forward(p, cfg, ids, types, tvc, text_mask, ovlc, obj_mask, False)[3]
    assert seq.shape == ref.shape, (seq.shape, ref.shape)
    live = (torch.arange(ref.shape[1])[None, :] < (tlen + nobj + 1)[:, None]).unsqueeze(-1).float()      # packed rows of each sample
    report("module-API packed sequence S=281 vs oracle (live rows)", seq.cpu() * live, ref * live, 2e-3, 1.5e-2)
    cot = torch.randn(ref.shape, generator=g) * live
    (ref * cot).sum().backward()
    (seq * to(cot)).sum().backward()
    e_tv, e_ovl = rel_fro(tv.grad, tvc.grad), rel_fro(ovl.grad, ovlc.grad)
    print("module-API (packed sequence, S=281) input gradients: rel-fro err text_visual %.3e object_vl %.3e" % (e_tv, e_ovl))
    assert e_tv <= 3e-2 and e_ovl <= 3e-2
    gw = dict(net.named_parameters())["encoder.layer.0.intermediate.dense.weight"].grad
    assert rel_fro(gw, p["vlbert.encoder.layer.0.intermediate.dense.weight"].grad) <= 5e-2
