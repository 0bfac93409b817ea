"""The engine as three parts that own their buffers (front / encoder / back), checked on the CPU with the library stubbed
(tests/step_trace.py): no build, no GPU.

* the stubbed step reproduces the call counts of the five modes (the helper sees what the engine launches);
* an fp32_full / fp32_ends engine launches no 16-bit kernel and holds no 16-bit activation-sized tensor;
* an encoder_fp32 engine with 16-bit ends keeps exactly the three 16-bit boundary tensors of the encoder, and its batched transpose
  holds the pairs of the ends only;
* the step functions of engine.py name none of the precision flags.
"""
import importlib
import inspect

import pytest
import torch

from tests import step_trace as ST

E = ST.ENGINE
OPS = ST.OPS
H = 768

MODES = {
    "default": dict(),
    "encoder_fp32": dict(encoder_fp32=True),
    "fp32_full": dict(encoder_fp32=True, fp32_full=True),
    "core": dict(core=True),
    "fp32_ends": dict(core=True, core_heads=False, core_sequence=True, encoder_fp32=True, fp32_ends=True),
}
# library calls of zero_grad -> forward(True) -> backward(True) -> optimizer_step() at 2 layers, B=2, T=8, R=4; the two fp32 modes
# without the two launches of the batched 16-bit transpose (sync_weights, optimizer_step) they have no use for
CALLS = {"default": 78, "encoder_fp32": 137, "fp32_full": 148 - 2, "core": 68, "fp32_ends": 105 - 2}


@pytest.fixture(scope="module")
def traced():
    return {name: ST.run(**kw) for name, kw in MODES.items()}


def tensors_of(obj, seen=None):
    """Every tensor reachable from an engine or a part through attributes, lists, tuples, dicts and plain objects of the package
    (a part's back-reference to its engine is not followed)."""
    seen = {} if seen is None else seen
    todo = [obj]
    visited = set()
    while todo:
        o = todo.pop()
        if id(o) in visited:
            continue
        visited.add(id(o))
        if isinstance(o, torch.Tensor):
            seen[id(o)] = o
        elif isinstance(o, (list, tuple)):
            todo.extend(o)
        elif isinstance(o, dict):
            todo.extend(o.values())
        elif type(o).__module__.startswith(("vl-bert_amd", "types")) and hasattr(o, "__dict__"):
            todo.extend(v for k, v in vars(o).items() if k != "eng")
    return list(seen.values())


def same_storage(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_stubbed_step_reproduces_the_call_counts(traced, mode):
    eng, calls = traced[mode]
    assert len(ST.names(calls)) == CALLS[mode]
    assert {type(p).__name__ for p in (eng.front, eng.encoder, eng.back)} == {
        "default": {"PretrainFront16", "Encoder16", "Heads16"}, "encoder_fp32": {"PretrainFront16", "EncoderF32", "Heads16"},
        "fp32_full": {"PretrainF32", "EncoderF32"}, "core": {"CoreFront16", "Encoder16", "Heads16"},
        "fp32_ends": {"CoreFrontF32", "EncoderF32", "SequenceOutF32"}}[mode]


@pytest.mark.parametrize("mode", ["fp32_full", "fp32_ends"])
def test_fp32_modes_launch_no_16_bit_kernel(traced, mode):
    """Only the flat working copy is still written in 16 bits: vlb_cast_f32_bf16 in sync_weights (and inside vlb_adamw_step)."""
    _, calls = traced[mode]
    names = ST.names(calls)
    bf16 = [n for n in names if n.endswith("_bf16")]
    assert bf16 == ["vlb_cast_f32_bf16"], bf16
    assert "vlb_adamw_step" in names and names.count("vlb_transpose_f32") > 0


@pytest.mark.parametrize("mode", ["fp32_full", "fp32_ends"])
def test_fp32_modes_hold_no_16_bit_activation(traced, mode):
    eng, _ = traced[mode]
    big = [t for t in tensors_of(eng) if t.dtype in (OPS.BF16, torch.float16) and t.numel() >= eng.M * H and not same_storage(t, eng.P.w16)]
    assert not big, [(tuple(t.shape), t.dtype) for t in big]
    assert eng.wT == {} and eng._tbatch.n == 0
    assert eng.X is eng.enc32.X and eng.X[0].dtype == torch.float32


def test_fp32_encoder_with_16_bit_ends_keeps_its_three_boundary_tensors(traced):
    eng, calls = traced["encoder_fp32"]
    enc, L = eng.enc32, eng.cfg.num_hidden_layers
    assert enc.cast and eng.encoder is enc and eng.pre32 is None
    # of the 16-bit encoder state: X[0], X[L] and one d X buffer
    is_big16 = lambda t: t.dtype in (OPS.BF16, torch.float16) and t.numel() >= eng.M * H
    big = [t for t in tensors_of(enc) if is_big16(t)]
    assert {id(t) for t in big} == {id(enc.x_in), id(enc.x_out), id(enc.dx_in)}, [tuple(t.shape) for t in big]
    assert all(tuple(t.shape) == (eng.M, H) for t in big) and len({t.data_ptr() for t in big}) == 3
    # and the engine itself holds none beyond the flat working copy and what its three parts own
    owned = {id(t) for part in (eng.front, eng.encoder, eng.back) for t in tensors_of(part)}
    loose = [t for t in tensors_of(eng) if is_big16(t) and id(t) not in owned and not same_storage(t, eng.P.w16)]
    assert not loose, [tuple(t.shape) for t in loose]
    assert eng.X[0] is enc.x_in and eng.X[L] is enc.x_out and eng.X[-1] is enc.x_out and len(eng.X) == L + 1
    assert eng.front.x0 is enc.x_in and eng.back.xl is enc.x_out and eng.back.dx is enc.dx_in
    # the batched transpose: the heads' four pairs and the front's one, no encoder layer
    assert sorted(eng.wT) == sorted(["vlbert.mlm_head.predictions.transform.dense.weight", "vlbert.word_embeddings.weight",
                                     "vlbert.mvrc_head.transform.dense.weight", "vlbert.mvrc_head.region_cls_pred.weight",
                                     "image_feature_extractor.obj_downsample.1.weight"])
    launches = [a for n, a in calls if n == "vlb_transpose_batched_bf16"]
    assert len(launches) == 2 and all(a[2] == 5 for a in launches)


def test_16_bit_engine_aliases_its_parts_tensors(traced):
    eng, calls = traced["default"]
    L = eng.cfg.num_hidden_layers
    assert eng.X is eng.encoder.X and eng.QKV is eng.encoder.QKV and eng.LSE is eng.encoder.LSE
    assert eng.mlm_logits is eng.back.mlm_logits and eng.text_out is eng.back.text_out and eng.st_emb is eng.front.st_emb
    assert eng.enc32 is None and eng.pre32 is None and eng.vision is None
    for n, t in eng.wT.items():
        assert any(t is part.wT.get(n) for part in (eng.front, eng.encoder, eng.back)), n
    assert len(eng.wT) == 4 * L + 5
    launches = [a for n, a in calls if n == "vlb_transpose_batched_bf16"]
    assert len(launches) == 2 and all(a[2] == 4 * L + 5 for a in launches)
    assert sorted(eng._gemm_weight_names()) == sorted(n for n, sh in eng.P.shapes.items() if len(sh) == 2 and (
        ".dense.weight" in n or n.endswith(("query.weight", "key.weight", "value.weight", "region_cls_pred.weight",
                                            "obj_downsample.1.weight", "word_embeddings.weight"))))


def test_fp32_full_eval_step_is_refused_before_anything_runs(traced):
    eng, _ = traced["fp32_full"]
    with ST.recording() as calls:
        with pytest.raises(ValueError, match="eval_step: not built for an fp32_full engine"):
            eng.eval_step()
    assert calls == []


def test_step_functions_name_no_precision_flag():
    for fn in ("forward", "_forward_to_logits", "backward", "eval_step", "zero_grad", "sync_weights", "sequence_output",
               "backward_core", "backward_core_hidden", "backward_core_sequence"):
        src = inspect.getsource(getattr(E.PretrainEngine, fn))
        for flag in ("fp32_ends", "fp32_full", "enc32", "pre32"):
            assert flag not in src, (fn, flag)
    for mod in ("encoder_16", "ends_16", "encoder_f32", "core_f32", "pretrain_f32"):      # nor does a part ask the engine for its mode
        src = inspect.getsource(importlib.import_module("vl-bert_amd." + mod))
        for flag in ("eng.fp32_ends", "e.fp32_ends", "eng.fp32_full", "e.fp32_full", "e.enc32", "e.pre32", "eng.enc32", "eng.pre32", "getattr(e,"):
            assert flag not in src, (mod, flag)


# -- the objective switches: one Heads16 for every setting ------------------------------------------------------------------------------
VARIANTS = {
    "mlm_only": dict(with_mvrc_loss=False),
    "mvrc_only": dict(with_mlm_loss=False),
    "mlm_norm": dict(mlm_norm_in_batch_first=True),
    "mvrc_norm": dict(mvrc_norm_in_batch_first=True),
    "both_norm": dict(mlm_norm_in_batch_first=True, mvrc_norm_in_batch_first=True),
    "mlm_only_rel": dict(with_mvrc_loss=False, with_pooler=True, with_rel_loss=True),
}
# library calls at 2 layers, B=2, T=160 (so that the compaction capacity of 256 rows is below B*T), R=4, as the separate variant part
# launched them before it was folded into Heads16: (train_step, eval_step) compacted, then with VLB_MLM_COMPACT=0
VARIANT_CALLS = {"mlm_only": (73, 29, 71, 28), "mvrc_only": (66, 27, 66, 27), "mlm_norm": (81, 34, 79, 33), "mvrc_norm": (80, 33, 78, 32),
                 "both_norm": (81, 34, 79, 33), "mlm_only_rel": (81, 32, 79, 31)}
MLM_ONLY = ("text_out", "mlm_u", "mlm_g", "mlm_h", "st_mlm", "mlm_logits", "mlm_logits_copy", "d_mlm_h", "d_mlm_g", "d_mlm_u", "sel_pos",
            "sel_src", "labels_c", "mlm_overflow", "d_text_out_c", "mlm_w")
MVRC_ONLY = ("obj_out", "mvrc_u", "mvrc_g", "mvrc_logits", "mvrc_logits_copy", "mvrc_tsum", "d_mvrc_u", "mvrc_w")
PLAIN_LOSS = {"vlb_ce_rowweight_eval": "vlb_ce_eval", "vlb_soft_ce_rowweight_fwd_bwd": "vlb_soft_ce_fwd_bwd",
              "vlb_soft_ce_rowweight_eval": "vlb_soft_ce_eval"}


def eval_step(eng):
    eng.eval_step()


def head_order(calls, compact):
    """Entry points of a step with the row-weighted losses named as the plain ones whose place they take."""
    plain = dict(PLAIN_LOSS, vlb_ce_rowweight_fwd_bwd="vlb_ce_fwd_bwd_compact" if compact else "vlb_ce_fwd_bwd")
    return [plain.get(n, n) for n in ST.names(calls) if n != "vlb_sample_norm_weights"]


def is_subsequence(short, full):
    it = iter(full)
    return all(n in it for n in short)


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_objective_variants_run_the_one_heads_part_in_its_order(monkeypatch, variant, compact):
    monkeypatch.setenv("VLB_MLM_COMPACT", "1" if compact else "0")
    kw = VARIANTS[variant]
    base_kw = {k: v for k, v in kw.items() if k in ("with_pooler", "with_rel_loss")}
    for i, step in enumerate((ST.train_step, eval_step)):
        eng, calls = ST.run(cfg_kw=kw, T=160, step=step)
        back = eng.back
        assert len(ST.names(calls)) == VARIANT_CALLS[variant][(0 if compact else 2) + i], (variant, compact, step.__name__)
        assert type(back).__name__ == "Heads16" and type(back).__module__ == "vl-bert_amd.ends_16"
        assert eng._mlm_compact_now == (compact and eng.cfg.with_mlm_loss)
        # an absent head owns nothing; d(text_out) / d(obj_out) exist whatever the heads
        for present, names, wts in ((back.mlm, MLM_ONLY, ("vlbert.mlm_head.predictions.transform.dense.weight", "vlbert.word_embeddings.weight")),
                                    (back.mvrc, MVRC_ONLY, ("vlbert.mvrc_head.transform.dense.weight", "vlbert.mvrc_head.region_cls_pred.weight"))):
            assert all((n in back.wT) == present for n in wts)
            if not present:
                assert not [n for n in names if hasattr(back, n)]
        assert tuple(back.d_text_out.shape) == (eng.BT, H) and tuple(back.d_obj_out.shape) == (eng.BR, H)
        assert hasattr(back, "mlm_w") == bool(kw.get("mlm_norm_in_batch_first")) and hasattr(back, "mvrc_w") == bool(kw.get("mvrc_norm_in_batch_first"))
        # the order is the default part's: with both heads the very sequence of the default objective (each row-weighted loss where
        # the plain one stands, after the weights of its samples), with one head that sequence less the absent head's launches
        _, base = ST.run(cfg_kw=base_kw, T=160, step=step)
        got, want = head_order(calls, eng._mlm_compact_now), ST.names(base)
        if back.mlm and back.mvrc:
            assert got == want
        else:
            # (the front of a model without MVRC adds its one-row table gradient in a launch of its own: PretrainFront16.front_bwd)
            got = [n for n in got if n != "vlb_add_rows_f32"]
            assert len(got) < len(want) and is_subsequence(got, want)


def test_every_16_bit_engine_has_the_one_heads_part(traced):
    for mode in ("default", "encoder_fp32", "core"):
        assert type(traced[mode][0].back).__name__ == "Heads16"
    with pytest.raises(ImportError):
        importlib.import_module("vl-bert_amd.objectives_16")
    eng, _ = ST.run(cfg_kw=dict(with_mlm_loss=False))
    with pytest.raises(RuntimeError, match="no module-API outputs"):
        eng.back.outputs()
    with pytest.raises(ValueError):
        ST.run(cfg_kw=dict(mlm_norm_in_batch_first=True), core=True)
