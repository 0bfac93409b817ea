"""The pre-training objective switches without a GPU: the CPU restatement (tests/objectives_ref.py) against what the real reference
recorded (tests/golden/objectives/objectives_small.npz, tools/make_objectives_golden.py), the parameter tables per switch setting against
the reference's named_parameters(), the refusals, the command line and the C ABI of the row-weighted losses."""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import vlbert_oracle as O
from tests import objectives_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "objectives", "objectives_small.npz")
NEW_ENTRY_POINTS = ("vlb_sample_norm_weights", "vlb_ce_rowweight_fwd_bwd", "vlb_soft_ce_rowweight_fwd_bwd", "vlb_ce_rowweight_eval",
                    "vlb_soft_ce_rowweight_eval")
_cache = {}


def fixture():
    if "z" not in _cache:
        _cache["z"] = np.load(FIXTURE, allow_pickle=False)
    return _cache["z"]


def case(name, multitask):
    """(tag, cfg, switches, batch) of one fixture case; the batch has 9 tensors for the multitask wrapper."""
    z = fixture()
    tag = "%s/%s/" % ("multitask" if multitask else "plain", name)
    kw = {str(k): int(v) for k, v in zip(z["cfg_keys"], z["cfg_vals"])}
    cfg = O.VLBertConfig(multitask=multitask, **kw)
    sw = R.Switches(*[bool(v) for v in z[tag + "switches"]])
    keys = ("boxes", "im_info", "text", "relationship_label", "mlm_labels", "mvrc_ops", "mvrc_labels") + \
        (("aux_text", "aux_mlm_labels") if multitask else ())
    return tag, cfg, sw, tuple(torch.from_numpy(z["in_" + k]) for k in keys)


def ref_result(name, multitask):
    """objectives_ref's (outputs, loss, grads, norm) of a case, computed once for every test that reads it."""
    key = (name, multitask)
    if key not in _cache:
        tag, cfg, sw, batch = case(name, multitask)
        _cache[key] = R.loss_and_grads(R.init_params(cfg, int(fixture()["pseed"]), sw), cfg, batch, sw)
    return _cache[key]


def cases():
    z = np.load(FIXTURE, allow_pickle=False)
    return [(str(n), m) for m in (False, True) for n in z["cases"]]


def sample(t, n=2048):
    t = t.detach().double().reshape(-1)
    return t[::max(1, t.numel() // n)][:n].float().numpy()


def test_fixture_holds_the_cases_the_engine_tests_need():
    z = fixture()
    assert [str(n) for n in z["cases"]] == ["mlm_only", "mvrc_only", "both_norm", "mlm_only_norm", "mvrc_only_norm", "both"]
    assert str(z["key_lists"]).startswith("named_parameters()")
    lab, soft = z["in_mlm_labels"], z["in_mvrc_labels"]
    # unequal counts among the samples that have any, so that a per-sample mean is not the batch mean; one sample without an MLM
    # label, one without a valid region
    assert int(z["B"]) == 3 and (lab >= 0).sum(1).tolist() == [1, 0, 3]
    assert (np.abs(soft.sum(-1) - 1) < 0.1).sum(1).tolist() == [1, 3, 0]
    assert (z["in_aux_mlm_labels"] >= 0).sum(1).tolist() == [1, 3]
    # the one combination the reference's own multitask forward cannot run (it reads mlm_loss_wvc, set only under WITH_MLM_LOSS)
    ran = {(w, str(n)): bool(z["%s/%s/ran" % (w, n)]) for w in ("plain", "multitask") for n in z["cases"]}
    assert [k for k, v in ran.items() if not v] == [("multitask", "mvrc_only"), ("multitask", "mvrc_only_norm")]


def test_a_norm_switch_moves_the_recorded_gradient_norm_beyond_the_engine_bar():
    """What the engine tests compare at 1e-2 -- the REAL reference's gradient norm -- differs between a norm switch on and off by far
    more than that on this batch (the losses hardly move: every token of an untrained model costs about ln V), so an engine that
    ignored a switch, or grouped the rows of the wrong samples, misses the bar."""
    z = fixture()
    moved = {}
    for on, off in (("plain/mlm_only_norm/", "plain/mlm_only/"), ("plain/mvrc_only_norm/", "plain/mvrc_only/"), ("plain/both_norm/", "plain/both/"),
                    ("multitask/mlm_only_norm/", "multitask/mlm_only/"), ("multitask/both_norm/", "multitask/both/")):
        a, b = float(z[on + "grad_norm"]), float(z[off + "grad_norm"])
        moved[on] = abs(a - b) / b
        assert moved[on] >= 5 * 1e-2, (on, a, b)
    # and the restatement says which gradients: with the MLM switch the MLM head's, with the MVRC switch the MVRC head's, each by more
    # than the engine tests' 5e-2 per-parameter bar
    tag, cfg, sw, batch = case("both", False)
    params = R.init_params(cfg, int(z["pseed"]), sw)
    g_off = ref_result("both", False)[2]
    for field, name in (("mlm_norm_in_batch_first", "vlbert.mlm_head.predictions.transform.dense.weight"),
                        ("mvrc_norm_in_batch_first", "vlbert.mvrc_head.region_cls_pred.weight")):
        g_on = R.loss_and_grads(params, cfg, batch, R.Switches(**{field: True}))[2]
        d = float((g_on[name] - g_off[name]).norm() / g_off[name].norm())
        assert d >= 2 * 5e-2, (field, d)


@pytest.mark.parametrize("name,multitask", cases())
def test_restatement_matches_the_reference(name, multitask):
    """Bars of tests/test_oracle_golden.py: losses and gradient norm 1e-5, logits rtol 1e-4 / atol 2e-5."""
    z = fixture()
    tag, cfg, sw, batch = case(name, multitask)
    if not bool(z[tag + "ran"]):
        assert multitask and not sw.with_mlm_loss
        return
    outputs, loss, grads, norm = ref_result(name, multitask)
    for k in (("mlm_loss_wvc", "mlm_loss_aux", "mvrc_loss") if multitask else ("mlm_loss", "mvrc_loss")):
        assert abs(float(outputs[k]) - float(z[tag + k])) <= 1e-5 * max(1.0, abs(float(z[tag + k]))), k
    assert abs(float(loss) - float(z[tag + "loss"])) <= 1e-5 * abs(float(z[tag + "loss"]))
    assert abs(norm - float(z[tag + "grad_norm"])) <= 1e-5 * float(z[tag + "grad_norm"])
    B = batch[2].shape[0]
    got = {"mvrc_logits": outputs["mvrc_logits"]}
    if outputs["mlm_logits"] is not None:
        got.update({"mlm_logits_wvc": outputs["mlm_logits"][:B], "mlm_logits_aux": outputs["mlm_logits"][B:]} if multitask
                   else {"mlm_logits": outputs["mlm_logits"]})
    for k in (("mlm_logits_wvc", "mlm_logits_aux", "mvrc_logits") if multitask else ("mlm_logits", "mvrc_logits")):
        shape = tuple(int(v) for v in z[tag + k + "_shape"])
        if not shape:                       # the reference returned None for the absent head
            assert got.get(k) is None, k
            continue
        t = got[k]
        if k == "mvrc_logits":              # the reference pads the region axis back to the batch's box slots with -10000 (:195-197)
            pad = t.new_full(shape, -10000.0)
            pad[:, :t.shape[1]] = t
            t = pad
        assert tuple(t.shape) == shape, (k, tuple(t.shape), shape)
        np.testing.assert_allclose(sample(t), z[tag + k + "_smp"], rtol=1e-4, atol=2e-5, err_msg=k)
    # an absent head has no parameters, so nothing of it has a gradient
    assert not [n for n in grads if R.absent(n, sw)]


@pytest.mark.parametrize("name,multitask", cases())
def test_parameter_tables_follow_the_reference_named_parameters(name, multitask):
    """FlatParams' shapes table per switch setting, put in the reference's order by common/checkpoint.py (the optimizer-state order),
    against named_parameters() of the real reference module: same keys, same order."""
    E, ck = importlib.import_module("vl-bert_amd.engine"), importlib.import_module("vl-bert_amd.common.checkpoint")
    z = fixture()
    tag, cfg, sw, _ = case(name, multitask)
    mc = E.ModelConfig(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                       intermediate_size=cfg.intermediate_size, vocab_size=cfg.vocab_size, max_position_embeddings=cfg.max_position_embeddings,
                       visual_region_classes=cfg.visual_region_classes, multitask=multitask, **sw.engine_kw())
    mc.validate()
    flat = E.FlatParams(mc, "cpu")
    want = [str(k) for k in z[tag + "keys"]]
    assert ck.reference_param_order(flat.shapes) == want
    shapes = {k: tuple(v.shape) for k, v in R.init_params(cfg, 0, sw).items()}
    assert {k: tuple(v) for k, v in flat.shapes.items()} == shapes
    assert ("vlbert.word_embeddings.weight" in flat.shapes) and (("object_mask_word_embedding.weight" in flat.shapes) == sw.with_mvrc_loss)


def test_default_switches_leave_the_parameter_table_alone():
    E = importlib.import_module("vl-bert_amd.engine")
    a = E.param_layout(E.ModelConfig(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256))
    b = E.param_layout(E.ModelConfig(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, with_mlm_loss=True,
                                     with_mvrc_loss=True, mlm_norm_in_batch_first=True, mvrc_norm_in_batch_first=True))
    assert list(a.items()) == list(b.items())      # (the norm switches change no parameter)
    assert set(a) == set(O.param_shapes(O.VLBertConfig(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256)))
    assert E.ModelConfig().default_objective and not E.ModelConfig(mlm_norm_in_batch_first=True).default_objective


def test_validate_refuses_a_model_without_a_loss_and_fp32_full_refuses_the_switches():
    E = importlib.import_module("vl-bert_amd.engine")
    small = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, intermediate_size=256)
    with pytest.raises(ValueError, match="no loss to train on"):
        E.ModelConfig(with_mlm_loss=False, with_mvrc_loss=False, **small).validate()
    E.ModelConfig(with_mlm_loss=False, with_mvrc_loss=False, with_pooler=True, with_rel_loss=True, **small).validate()
    for kw in (dict(with_mlm_loss=False), dict(with_mvrc_loss=False), dict(mlm_norm_in_batch_first=True), dict(mvrc_norm_in_batch_first=True)):
        with pytest.raises(ValueError, match=r"fp32_full needs .*unsupported here: .*objective switches"):
            E.PretrainEngine._check_fp32_full(E.ModelConfig(**small, **kw), 8, 4, False, True, None, "allreduce", 0, None)
    E.PretrainEngine._check_fp32_full(E.ModelConfig(**small), 8, 4, False, True, None, "allreduce", 0, None)


def test_dry_run_resolves_the_objective_keys(tmp_path):
    tr = importlib.import_module("vl-bert_amd.pretrain.train_end2end")
    y = tmp_path / "cfg.yaml"
    y.write_text("MODULE: ResNetVLBERTForPretraining\nNETWORK:\n  WITH_MVRC_LOSS: false\n  MLM_LOSS_NORM_IN_BATCH_FIRST: true\n"
                 "  MVRC_LOSS_NORM_IN_BATCH_FIRST: true\n  VLBERT:\n    num_hidden_layers: 2\n")
    r = tr.main(["--cfg", str(y), "--dry-run"])
    # (a norm switch of an absent loss means nothing: the reference never reads it there)
    assert r["objective"] == dict(with_mlm_loss=True, with_mvrc_loss=False, mlm_norm_in_batch_first=True, mvrc_norm_in_batch_first=False)
    assert tr.describe_objective(r["objective"]) == "mlm (norm in batch first)"
    assert tr.describe_objective(tr.objective_of(tr.load_config(None))) == "mlm + mvrc"
    y.write_text("MODULE: ResNetVLBERTForPretraining\nNETWORK:\n  WITH_MLM_LOSS: false\n  MVRC_LOSS_NORM_IN_BATCH_FIRST: true\n")
    assert tr.describe_objective(tr.main(["--cfg", str(y), "--dry-run"])["objective"]) == "mvrc (norm in batch first)"
    y.write_text("MODULE: ResNetVLBERTForPretraining\n")
    assert tr.main(["--cfg", str(y), "--dry-run"])["objective"] == dict(with_mlm_loss=True, with_mvrc_loss=True, mlm_norm_in_batch_first=False,
                                                                         mvrc_norm_in_batch_first=False)
    y.write_text("MODULE: ResNetVLBERTForPretrainingMultitask\nNETWORK:\n  WITH_MLM_LOSS: false\n")
    with pytest.raises(NotImplementedError, match="multitask wrapper without WITH_MLM_LOSS"):
        tr.main(["--cfg", str(y), "--dry-run"])


def test_header_bindings_and_both_builds_agree_on_the_new_entry_points():
    import ctypes
    from tests.test_abi import header_prototypes
    lib = importlib.import_module("vl-bert_amd._lib")
    protos = header_prototypes()
    for name in NEW_ENTRY_POINTS:
        assert protos[name] == lib._SIGS[name], name
    for path in (lib._default_path("bf16"), lib._default_path("f16")):
        if not os.path.isfile(path):
            import __graft_entry__
            __graft_entry__.build()
        h = ctypes.CDLL(path)
        h.vlb_version.restype = ctypes.c_int
        assert h.vlb_version() == 300
        for name in NEW_ENTRY_POINTS:
            assert hasattr(h, name), "%s does not export %s" % (os.path.basename(path), name)


def test_restated_weighted_losses_on_batches_without_a_labelled_row():
    """A batch with no labelled row at all: loss 0, d(logits) all zero, nothing NaN; and a sample with n_b = 0 adds nothing."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(6, 11, generator=g)
    l0, l1, d = R.weighted_ce(x, torch.full((6,), -1, dtype=torch.int64), 2, 3, B_split=1)
    assert l0 == 0.0 and l1 == 0.0 and torch.equal(d, torch.zeros_like(d))
    l, d = R.weighted_soft_ce(x, torch.zeros(6, 11), 2, 3)
    assert l == 0.0 and torch.equal(d, torch.zeros_like(d))
    lab = torch.tensor([2, -1, 5, -1, -1, -1])
    l0, _, d = R.weighted_ce(x, lab, 2, 3)
    ce = torch.nn.functional.cross_entropy(x.double(), lab, ignore_index=-1, reduction="none")
    assert abs(l0 - float((ce[0] + ce[2]) / (2 + 1e-4) / (1 + 1e-4))) < 1e-12 and not d[3:].any() and not d[1].any() and d[0].any()
