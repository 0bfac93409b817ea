"""Attention-map visualisation on the fused 16-bit path (-m gpu), layer by layer above the kernel test (test_attention_probs_gpu.py):
PretrainEngine.attention_probs() / encoded_layers(), the inspection call forms of the VisualLinguisticBert mirror on that path
(257..512 positions, or `inspect_fused`), the ResNetVLBERTForAttentionVis mirror and the vis_attention_maps entry point.

Bars.  Hidden states: the project's hidden-state class report(.., 2e-3, 1.5e-2), the bar of the fp32-path inspection test.  Attention
probabilities against the oracle's fp32 probabilities: not derivable (the 16-bit rounding of x_l, Q and K enters), so measured --
max abs error per layer on the bf16 build, 2 layers:
    S = 101 (T 64, R 36):    layer 0 1.597e-04, layer 1 2.259e-04   (against the oracle's OTHER layer: 3.2e-02)
    S = 301 (T 200, R 100):  layer 0 5.916e-05, layer 1 6.298e-05   (against the oracle's OTHER layer: 8.8e-03)
PROBS_BAR = 5e-4 = twice the largest of these (4.5e-4) rounded up to one significant digit (the factor 2 for other seeds: the
arithmetic is deterministic).  Layer l against the oracle's layer 1 - l must miss it.  The same bar holds the module-level comparisons
(281 positions against the oracle: 8.2e-05; inspect_fused against the fp32-encoder path at 101 positions: 1.3e-04).
"""
import os

import numpy as np
import pytest
import torch

from oracle import vlbert_oracle as O
from tests import attention_probs_ref as AR
from tests.gpu_util import dev, device_seed, pkg, report
from tests.test_engine_gpu import _module_config, make_engine

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "fixtures", "attention_vis_small.yaml")
PROBS_BAR = 5e-4
HID = (2e-3, 1.5e-2)


def valid_rows(t, mask):
    """[B, (nh,) n, ...] -> the rows of valid queries only (padded positions hold whatever the front end put there)."""
    return t[mask] if t.dim() == 3 else t.permute(0, 2, 1, 3)[mask]


# ------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("T,R", [(64, 36), (200, 100)])
def test_engine_attention_probs_and_encoded_layers_vs_oracle(T, R):
    syn = pkg("synthetic")
    cfg = O.VLBertConfig(num_hidden_layers=2, max_position_embeddings=512)
    params = O.init_params(cfg, seed=71)
    batch = syn.make_batch(2, T, R, seed=72 + T, ragged=True)
    eng = make_engine(cfg, 2, T, R, train=False, max_seq=512)
    eng.load_state_dict({k: v.to(dev()) for k, v in params.items()})
    eng.set_batch(*[t.to(dev()) for t in batch])
    eng.forward(train=False)
    layers, probs = eng.encoded_layers(), eng.attention_probs()
    want_x, want_p, mask = AR.oracle_layers_and_probs(params, cfg, AR.oracle_core_inputs(params, cfg, batch))
    L, nh, n = cfg.num_hidden_layers, cfg.num_attention_heads, mask.shape[1]
    assert len(layers) == L and len(probs) == L and eng.longest_sequence() == n
    assert probs[0].shape == (2, nh, n, n) and probs[0].dtype == torch.float32 and layers[0].shape == (2, n, cfg.hidden_size)
    errs, other = [], []
    for l in range(L):
        got = valid_rows(probs[l].cpu(), mask)
        errs.append(float((got - valid_rows(want_p[l], mask)).abs().max()))
        other.append(float((got - valid_rows(want_p[1 - l], mask)).abs().max()))
        print("engine S%d attention_probs layer %d vs oracle fp32: max abs err %.3e (vs the oracle's layer %d: %.3e)"
              % (eng.S, l, errs[-1], 1 - l, other[-1]))
    for l in range(L):
        report("engine S%d encoded layer %d vs oracle" % (eng.S, l), valid_rows(layers[l].cpu(), mask), valid_rows(want_x[l], mask), *HID)
        assert float((valid_rows(probs[l].cpu(), mask).sum(-1) - 1.0).abs().max()) <= 2e-3
        assert float((probs[l].cpu() * (~mask)[:, None, None, :]).abs().max()) == 0.0           # padded keys: exact zeros
    assert max(errs) <= PROBS_BAR, errs
    assert min(other) > PROBS_BAR, other                        # the other layer's probabilities miss the bar
    # one layer, a given n; and the same call again is bit-identical
    one = eng.attention_probs(layers=[1], n=n - 3)
    assert len(one) == 1 and torch.equal(one[0], probs[1][:, :, :n - 3, :n - 3])
    assert torch.equal(eng.encoded_layers(1, n=5)[0], layers[1][:, :5])
    with pytest.raises(ValueError):
        eng.attention_probs(layers=[2])


def test_engine_attention_probs_after_a_whole_training_step_carry_the_forwards_masks():
    """forward(True), backward, optimizer_step -- which advances the dropout seed -- and only then attention_probs(): the result is the
    un-dropped probabilities of that forward times keep / 0.9 under the seed the FORWARD drew from, not the next step's."""
    syn, ops = pkg("synthetic"), pkg("ops")
    cfg = O.VLBertConfig(num_hidden_layers=2, max_position_embeddings=512)
    B, T, R = 2, 24, 12
    eng = make_engine(cfg, B, T, R, train=True, lr=1e-4)
    eng.load_state_dict({k: v.to(dev()) for k, v in O.init_params(cfg, seed=91).items()})
    eng.set_batch(*[t.to(dev()) for t in syn.make_batch(B, T, R, seed=92, ragged=True)])
    seed = device_seed(eng)
    eng.zero_grad()
    eng.forward(train=True)
    before = eng.attention_probs()
    eng.backward(train=True)
    eng.optimizer_step()
    moved = device_seed(eng)
    assert moved != seed
    after = eng.attention_probs()
    nh, S, n = cfg.num_attention_heads, eng.S, after[0].shape[-1]
    for l in range(cfg.num_hidden_layers):
        undropped = ops.attention_probs(eng.QKV[l], eng.lay["attn_mask"], eng.LSE[l], B, S, cfg.hidden_size, nh, n=n).cpu()
        keep = AR.keep_scale(seed, l * 8, B, nh, S, cfg.attention_probs_dropout_prob)[:, :, :n, :n].float()
        wrong = AR.keep_scale(moved, l * 8, B, nh, S, cfg.attention_probs_dropout_prob)[:, :, :n, :n].float()
        assert torch.equal(after[l], before[l])
        assert float((after[l].cpu() - undropped * keep).abs().max()) <= 1e-6
        assert float((after[l].cpu() - undropped * wrong).abs().max()) > 2e-3
    eng.forward(train=False)                                    # the next forward: no dropout, every valid query's row sums to 1
    valid = eng.lay["attn_mask"].view(B, S)[:, :n].bool().cpu()
    assert float((valid_rows(eng.attention_probs([0])[0].cpu(), valid).sum(-1) - 1.0).abs().max()) <= 2e-3


def test_engine_methods_point_an_fp32_encoder_engine_at_its_own_buffers():
    cfg = O.VLBertConfig(num_hidden_layers=1)
    eng = make_engine(cfg, 1, 8, 4, train=False, encoder_fp32=True)
    with pytest.raises(ValueError, match=r"enc32\.P"):
        eng.attention_probs()
    with pytest.raises(ValueError, match=r"enc32\.X"):
        eng.encoded_layers()


# ------------------------------------------------------------------------------------------------- module API
def core_case(B, T, R, H, seed, vocab=30522):
    """Ragged VisualLinguisticBert inputs (CPU): sample 0 has the full text, the last sample every object."""
    g = torch.Generator().manual_seed(seed)
    tlen = torch.randint(T // 2, T + 1, (B,), generator=g)
    nobj = torch.randint(R // 2, R + 1, (B,), generator=g)
    tlen[0], nobj[-1] = T, R
    text_mask = torch.arange(T)[None] < tlen[:, None]
    obj_mask = torch.arange(R)[None] < nobj[:, None]
    ids = torch.randint(1000, vocab, (B, T), generator=g) * text_mask
    return [ids, torch.zeros_like(ids), torch.randn(B, T, H, generator=g), text_mask, torch.randn(B, R, 2 * H, generator=g), obj_mask]


def vlbert_params(params):
    return {k[len("vlbert."):]: v for k, v in params.items()
            if k.startswith("vlbert.") and not k.startswith(("vlbert.mlm_head.", "vlbert.mvrc_head."))}


def make_net(cfg, params, p_hidden=0.1, **kw):
    VL = pkg("common.visual_linguistic_bert")
    vcfg = _module_config(cfg)["NETWORK"]["VLBERT"]
    vcfg["hidden_dropout_prob"] = p_hidden
    net = VL.VisualLinguisticBert(vcfg, **kw)
    net.load_state_dict(vlbert_params(params))
    return net.eval()


def test_module_inspection_forms_run_on_the_fused_path_at_281_positions():
    cfg = O.VLBertConfig(num_hidden_layers=2, max_position_embeddings=512)
    params = O.init_params(cfg, seed=73)
    B, T, R, H = 2, 180, 100, cfg.hidden_size
    ins = core_case(B, T, R, H, 74)
    net = make_net(cfg, params)
    gi = [t.to(dev()) for t in ins]
    layers, pooled, probs = net(*gi, output_all_encoded_layers=True, output_attention_probs=True)
    want_x, want_p, mask = AR.oracle_layers_and_probs(params, cfg, ins)
    L, nh, n = cfg.num_hidden_layers, cfg.num_attention_heads, mask.shape[1]
    assert n > 256 and pooled is None and len(layers) == L and len(probs) == L
    assert layers[0].shape == (B, n, H) and probs[0].shape == (B, nh, n, n) and not probs[0].requires_grad and not layers[0].requires_grad
    assert ("inspect_fused", B, T, R) in net._engines and ("inspect", B, T, R) not in net._engines
    for l in range(L):
        report("module S281 layer %d vs oracle" % l, valid_rows(layers[l].cpu(), mask), valid_rows(want_x[l], mask), *HID)
        err = float((valid_rows(probs[l].cpu(), mask) - valid_rows(want_p[l], mask)).abs().max())
        print("module S281 attention_probs layer %d vs oracle fp32: max abs err %.3e" % (l, err))
        assert err <= PROBS_BAR
    last, _ = net(*gi, output_all_encoded_layers=False, output_attention_probs=False, output_text_and_object_separately=False)
    report("module S281: last layer vs the default call form", layers[-1], last[:, :n], *HID)
    only_last, _, _ = net(*gi, output_all_encoded_layers=False, output_attention_probs=True)
    assert torch.equal(only_last, layers[-1])
    # text and objects separately: objects placed as the oracle's masked scatter does
    texts, objs, pooled, probs2 = net(*gi, output_all_encoded_layers=True, output_text_and_object_separately=True, output_attention_probs=True)
    rt, ro, _, _ = O.vlbert_forward(params, cfg, *ins, False)
    assert len(texts) == L and texts[-1].shape == (B, T, H) and objs[-1].shape == (B, R, H) and torch.equal(probs2[0], probs[0])
    tm = ins[3].unsqueeze(-1).float()
    report("module S281 separately: text rows vs oracle", texts[-1][:, :n].cpu() * tm[:, :n], (rt * tm[:, :rt.shape[1]])[:, :n], *HID)
    report("module S281 separately: object rows vs oracle", objs[-1], ro, *HID)
    assert float(objs[-1].cpu()[~ins[5]].abs().max()) == 0.0


def test_module_fp32_encoder_still_refuses_281_positions(monkeypatch):
    monkeypatch.setenv("VLB_ENCODER_FP32", "1")
    cfg = O.VLBertConfig(num_hidden_layers=1, max_position_embeddings=512)
    net = make_net(cfg, O.init_params(cfg, seed=75))
    assert net.fp32_encoder
    with pytest.raises(ValueError, match="at most 256 positions"):
        net(*[t.to(dev()) for t in core_case(1, 180, 100, cfg.hidden_size, 76)], output_all_encoded_layers=True, output_attention_probs=True)


def test_module_inspect_fused_switch_at_101_positions(monkeypatch):
    cfg = O.VLBertConfig(num_hidden_layers=2, max_position_embeddings=512)
    params = O.init_params(cfg, seed=77)
    B, T, R, H = 2, 64, 36, cfg.hidden_size
    ins = core_case(B, T, R, H, 78)
    gi = [t.to(dev()) for t in ins]
    plain, fused = make_net(cfg, params), make_net(cfg, params, inspect_fused=True)
    assert not plain.inspect_fused and fused.inspect_fused
    l32, _, p32 = plain(*gi, output_all_encoded_layers=True, output_attention_probs=True)
    l16, _, p16 = fused(*gi, output_all_encoded_layers=True, output_attention_probs=True)
    # switch off: today's engine and no fused-inspection engine; switch on: the reverse
    assert list(plain._engines) == [("inspect", B, T, R)] and plain._engines[("inspect", B, T, R)].enc32 is not None
    assert list(fused._engines) == [("inspect_fused", B, T, R)] and fused._engines[("inspect_fused", B, T, R)].enc32 is None
    mask = (torch.arange(l32[0].shape[1])[None] <= (ins[3].sum(1) + ins[5].sum(1))[:, None])
    for l in range(cfg.num_hidden_layers):
        assert p16[l].shape == p32[l].shape and l16[l].shape == l32[l].shape
        report("inspect_fused S101 layer %d vs the fp32-encoder path" % l, valid_rows(l16[l].cpu(), mask), valid_rows(l32[l].cpu(), mask), *HID)
        err = float((valid_rows(p16[l].cpu(), mask) - valid_rows(p32[l].cpu(), mask)).abs().max())
        print("inspect_fused S101 attention_probs layer %d vs the fp32-encoder path: max abs err %.3e" % (l, err))
        assert err <= PROBS_BAR
    monkeypatch.setenv("VLB_INSPECT_FUSED", "1")
    assert make_net(cfg, params).inspect_fused


def test_module_training_mode_returns_the_probabilities_after_their_dropout():
    """attention dropout 0.1, hidden dropout 0 (so that layer 0 sees the eval inputs): every layer's result is the un-dropped
    probabilities of the same forward times keep / 0.9 under tag 8 l of the engine's seed; layer 0's also the eval result times it."""
    cfg = O.VLBertConfig(num_hidden_layers=2, max_position_embeddings=512)
    params = O.init_params(cfg, seed=79)
    B, T, R, H = 2, 40, 20, cfg.hidden_size
    gi = [t.to(dev()) for t in core_case(B, T, R, H, 80)]
    net = make_net(cfg, params, p_hidden=0.0, inspect_fused=True)
    _, _, p_eval = net(*gi, output_all_encoded_layers=True, output_attention_probs=True)
    net.train()
    _, _, p_train = net(*gi, output_all_encoded_layers=True, output_attention_probs=True)
    eng = net._engines[("inspect_fused", B, T, R)]
    ops, n, nh, S = pkg("ops"), p_train[0].shape[-1], cfg.num_attention_heads, eng.S
    seed = device_seed(eng)
    for l in range(cfg.num_hidden_layers):
        keep = AR.keep_scale(seed, l * 8, B, nh, S, 0.1)[:, :, :n, :n].float()
        undropped = ops.attention_probs(eng.QKV[l], eng.lay["attn_mask"], eng.LSE[l], B, S, H, nh, n=n).cpu()
        assert 0.05 < float((keep == 0).float().mean()) < 0.15
        assert float((p_train[l].cpu() - undropped * keep).abs().max()) <= 1e-6
        assert float((p_train[l].cpu() - AR.keep_scale(seed, l * 8 + 1, B, nh, S, 0.1)[:, :, :n, :n].float() * undropped).abs().max()) > 2e-3
    keep0 = AR.keep_scale(seed, 0, B, nh, S, 0.1)[:, :, :n, :n].float()
    report("training-mode layer 0 vs eval x keep / 0.9", p_train[0], p_eval[0].cpu() * keep0, 2e-3, 0)


# ------------------------------------------------------------------------------------------------- mirror
def load_fixture(**net):
    te = pkg("pretrain.train_end2end")
    config = te.load_config(FIXTURE)
    config.NETWORK.update(net)
    return config


def test_mirror_state_dict_outputs_and_agreement_with_the_bare_encoder_mirror():
    M = pkg("pretrain.modules")
    names = pkg("pretrain.modules.resnet_vlbert_for_attention_vis").parameter_names
    syn = pkg("synthetic")
    config = load_fixture()
    net = M.ResNetVLBERTForAttentionVis(config).eval()
    assert set(net.state_dict()) == set(names(config)) == set(k for k, _ in net.named_parameters())
    assert net.vlbert.inspect_fused and "object_mask_word_embedding.weight" in net.state_dict()
    no_mvrc = load_fixture(WITH_MVRC_LOSS=False)
    assert "object_mask_word_embedding.weight" not in names(no_mvrc) and "object_mask_visual_embedding.weight" in names(no_mvrc)
    with torch.no_grad():                                       # visual LayerNorm scales start at 0: give the visual half a say
        net.vlbert.visual_ln_text.weight.fill_(0.5)
        net.vlbert.visual_ln_object.weight.fill_(0.5)
        net.object_mask_visual_embedding.weight.normal_(0.0, 0.5)
    B, T, R = 2, 24, 10
    batch = [t.to(dev()) for t in syn.make_batch(B, T, R, seed=81, ragged=True)]
    boxes_before = batch[0].clone()
    out = net(None, *batch)
    vl = config.NETWORK.VLBERT
    L, nh, H = vl.num_hidden_layers, vl.num_attention_heads, vl.hidden_size
    n = int(((batch[2] > 0).sum(1) + (batch[0][:, :, 0] > -1.5).sum(1)).max()) + 1
    assert set(out) == {"attention_probs", "hidden_states"} and torch.equal(batch[0], boxes_before)
    assert out["attention_probs"].shape == (B, L, nh, n, n) and out["attention_probs"].dtype == torch.float32
    assert out["hidden_states"].shape == (B, L, n, H) and out["hidden_states"].dtype == torch.float32
    assert not out["attention_probs"].requires_grad
    ins = net.embeddings(None, batch[0], batch[1], batch[2], batch[5])
    layers, _, probs = net.vlbert(*ins, output_all_encoded_layers=True, output_attention_probs=True)
    for l in range(L):
        assert torch.equal(out["attention_probs"][:, l], probs[l]) and torch.equal(out["hidden_states"][:, l], layers[l])
    # the masked regions reach the encoder: without the mvrc_ops the maps differ
    batch2 = list(batch)
    batch2[5] = torch.zeros_like(batch[5])
    assert float((net(None, *batch2)["attention_probs"] - out["attention_probs"]).abs().max()) > 1e-4
    # text-only auxiliary samples ride along (the multitask loaders' batches)
    aux_text, aux_lab = syn.make_aux_text(3, 16, seed=82)
    both = net(None, *batch, aux_text.to(dev()), aux_lab.to(dev()))
    assert both["attention_probs"].shape == (B + 3, L, nh, n, n)
    report("mirror: caption samples beside aux samples", both["attention_probs"][:B], out["attention_probs"], 1e-6, 0)


def test_mirror_refuses_what_its_building_blocks_refuse():
    M = pkg("pretrain.modules")
    with pytest.raises(NotImplementedError, match="IMAGE_SEMANTIC"):
        M.ResNetVLBERTForAttentionVis(load_fixture(IMAGE_SEMANTIC=True))
    bad = load_fixture()
    bad.NETWORK.VLBERT["visual_size"] = 512
    with pytest.raises(NotImplementedError, match="visual_size != hidden_size"):
        M.ResNetVLBERTForAttentionVis(bad)
    bad = load_fixture()
    bad.NETWORK.VLBERT["word_embedding_frozen"] = True
    with pytest.raises(NotImplementedError, match="frozen embeddings"):
        M.ResNetVLBERTForAttentionVis(bad)


def test_mirror_e2e_image_branch():
    """IMAGE_FEAT_PRECOMPUTED false at the image size and box count of the FastRCNN-mirror e2e test (tests/golden/vision): shapes,
    finiteness and row sums only."""
    from tests.test_vision_gpu import _vision_fixture
    M = pkg("pretrain.modules")
    z, nl, _ = _vision_fixture()
    img, boxes4, im_info = [torch.from_numpy(z[k]).to(dev()) for k in ("img", "boxes", "im_info")]
    B, R = boxes4.shape[:2]
    net = M.ResNetVLBERTForAttentionVis(load_fixture(IMAGE_FEAT_PRECOMPUTED=False, IMAGE_NUM_LAYERS=nl)).eval()
    assert "object_mask_visual_embedding.weight" not in net.state_dict()          # MASK_RAW_PIXELS: the dataset masks the pixels
    g = torch.Generator().manual_seed(83)
    text = torch.randint(1000, 30522, (B, 12), generator=g).to(dev())
    text[-1, 9:] = 0
    zeros = torch.zeros((B, R), dtype=torch.long, device=dev())
    out = net(img, boxes4, im_info, text, None, None, zeros, None)
    n = int(((text > 0).sum(1) + (boxes4[:, :, 0] > -1.5).sum(1)).max()) + 1
    pr = out["attention_probs"].cpu()
    assert pr.shape == (B, 2, 12, n, n) and out["hidden_states"].shape == (B, 2, n, 768)
    assert bool(torch.isfinite(pr).all()) and bool(torch.isfinite(out["hidden_states"]).all())
    length = ((text > 0).sum(1) + (boxes4[:, :, 0] > -1.5).sum(1)).cpu() + 1
    mask = torch.arange(n)[None] < length[:, None]
    assert float((pr.sum(-1).permute(0, 3, 1, 2)[mask] - 1.0).abs().max()) <= 2e-3
    assert float((pr * (~mask)[:, None, None, None, :]).abs().max()) == 0.0
    mve = load_fixture(IMAGE_FEAT_PRECOMPUTED=False, IMAGE_NUM_LAYERS=nl, MASK_RAW_PIXELS=False)
    with pytest.raises(NotImplementedError, match="mask_visual_embed is not supported"):
        M.ResNetVLBERTForAttentionVis(mve).eval()(img, boxes4, im_info, text, None, None, zeros, None)


# ------------------------------------------------------------------------------------------------- entry point
# main() sets this variable for its process (setdefault): the tests put it there themselves, so that it is taken back afterwards
IPC = ("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))


def check_maps(folder, lengths, L=2, nh=12):
    """{image id: valid length}: one float32 [L, nh, n, n] file per sample, rows over valid keys sum to 1, padded keys exactly 0."""
    assert sorted(os.listdir(folder)) == sorted("%s.npy" % k for k in lengths)
    for image_id, length in lengths.items():
        a = np.load(os.path.join(folder, "%s.npy" % image_id))
        assert a.dtype == np.float32 and a.ndim == 4 and a.shape[:2] == (L, nh) and a.shape[2] == a.shape[3] >= length, (image_id, a.shape)
        assert np.abs(a[:, :, :length, :length].sum(-1) - 1.0).max() <= 2e-3, image_id
        assert np.abs(a[:, :, :, length:]).max(initial=0.0) == 0.0, image_id


def test_entry_point_writes_one_map_per_synthetic_sample(tmp_path, monkeypatch):
    monkeypatch.setenv(IPC[0], IPC[1])
    V, syn = pkg("pretrain.vis_attention_maps"), pkg("synthetic")
    for B, folder in ((1, tmp_path / "one"), (2, tmp_path / "two")):      # the fixture's one sample per batch; two per batch
        written = V.main(["--cfg", FIXTURE, "--save-dir", str(folder), "--steps", "2"] + (["--batch-images", "2"] if B == 2 else []))
        lengths = {}
        for step in range(2):
            b = syn.make_batch(B, 64, 36, seed=step, ragged=True)
            for i in range(B):
                lengths["synthetic_%06d" % (B * step + i)] = int((b[2][i] > 0).sum() + (b[0][i, :, 0] > -1.5).sum()) + 1
        assert len(written) == 2 * B
        check_maps(str(folder / "attention_probs"), lengths)


def test_entry_point_reads_a_caption_data_set(tmp_path, monkeypatch):
    """--data: the tiny caption set with full-width detector records (tests/test_data_cpu.write_dataset over tests/fixtures/cc_tiny's
    captions and vocabulary: cc_tiny's own records carry 8-dimensional features, the model reads 2048), validation set = its train set."""
    import yaml
    from tests.test_data_cpu import FIX, write_dataset
    monkeypatch.setenv(IPC[0], IPC[1])
    V, data, te = pkg("pretrain.vis_attention_maps"), pkg("pretrain.data"), pkg("pretrain.train_end2end")
    root = write_dataset(str(tmp_path / "cc"))
    with open(FIXTURE) as f:
        cfg = yaml.safe_load(f)
    cfg["DATASET"] = dict(DATASET="conceptual_captions", DATASET_PATH=root, ROOT_PATH=root, TRAIN_IMAGE_SET="train", VAL_IMAGE_SET="train",
                          ADD_IMAGE_AS_A_BOX=True, SEQ_LEN=32)
    cfg["NETWORK"].update(BERT_MODEL_NAME=os.path.join(FIX, "vocab"), PIXEL_MEANS=[102.9801, 115.9465, 122.7717], PIXEL_STDS=[1.0, 1.0, 1.0])
    path = str(tmp_path / "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    written = V.main(["--cfg", path, "--save-dir", str(tmp_path / "maps"), "--data", "--batch-images", "4"])      # batches of 4 and 2
    ds = data.make_dataloader(te.load_config(path), mode="val").dataset
    lengths = {}
    for index in range(len(ds)):
        s = ds[index]
        lengths[V.image_id_of(ds, index)] = int((torch.as_tensor(s[3]) > 0).sum() + (s[1][:, 0] > -1.5).sum()) + 1
    assert len(written) == len(ds) == 6 and sorted(lengths) == ["%04d" % i for i in range(6)]
    check_maps(str(tmp_path / "maps" / "attention_probs"), lengths)
