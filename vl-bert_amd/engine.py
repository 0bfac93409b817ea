"""MI355X-native VL-BERT pre-training engine: the whole training step of
`ResNetVLBERTForPretraining` (precomputed-feature configuration) as a fixed sequence of
hand-written HIP kernels called through the C ABI.

Reference path being replaced: pretrain/modules/resnet_vlbert_for_pretraining.py:93-216
-> common/fast_rcnn.py:128-203 -> common/visual_linguistic_bert.py:95-241,346-380 ->
external/pytorch_pretrained_bert/modeling.py:268-482, its autograd backward, clip_grad_norm_ +
AdamW.step (common/trainer.py:123-153, common/nlp/bert/optimization.py:129-187) and the DDP gradient
all-reduce (pretrain/function/train.py:89-90).

Design: static shapes [B, S=T+R+1] with in-kernel masking (no .item()/.nonzero() host
syncs), bf16 activations / fp32 accumulation / fp32 master weights, every parameter in ONE flat fp32
buffer (nn.Parameter views alias it; gradients, Adam moments and the bf16 working copy are flat
twins), explicit hand-scheduled backward (no autograd) so gradient buckets can be all-reduced over
RCCL while earlier layers are still running, whole step capturable in a hipGraph.

PyTorch supplies device memory, streams and torch.distributed; no torch arithmetic on the hot path.
"""
import math
import os
from collections import OrderedDict
from dataclasses import dataclass

import torch

from . import ops
from .side_streams import SideStreams

F32 = torch.float32
MAX_SEQ = 512           # longest packed sequence of the fused attention kernels (csrc/attention_common.h: ATT_LONG_MAX)
VIS_DIM = 2048          # hard-coded in the reference (common/fast_rcnn.py:107, resnet_vlbert_for_pretraining.py:25)
TAG_EMBED, TAG_DOWNSAMPLE = 1000, 1001


def _ru(x, m):
    return (x + m - 1) // m * m


@dataclass
class ModelConfig:
    """NETWORK.VLBERT keys the hot path reads (pretrain/function/config.py:86-122)."""
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    vocab_size: int = 30522
    max_position_embeddings: int = 512
    type_vocab_size: int = 3
    visual_region_classes: int = 1601
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    obj_downsample_dropout: float = 0.1
    multitask: bool = False      # ResNetVLBERTForPretrainingMultitask: text-only auxiliary samples (+1 parameter)
    with_pooler: bool = False    # BertPooler on the first token (modeling.py:424-436)
    with_rel_loss: bool = False  # relationship head on the pooled output + its CE loss (needs with_pooler)
    e2e: bool = False            # IMAGE_FEAT_PRECOMPUTED false: ResNet trunk -> ROIAlign -> layer4 head on the device (vision.py)
    image_num_layers: int = 101  # NETWORK.IMAGE_NUM_LAYERS (50 / 101 / 152)
    image_frozen_stages: tuple = (1, 2)   # NETWORK.IMAGE_FROZEN_BACKBONE_STAGES (BatchNorm is always frozen: IMAGE_FROZEN_BN)
    # objective switches (NETWORK.WITH_MLM_LOSS / WITH_MVRC_LOSS / *_LOSS_NORM_IN_BATCH_FIRST): an absent loss takes its head and the
    # parameters only it reads out of the model; norm in batch first = per-sample means (ends_16.Heads16).  The defaults change nothing
    with_mlm_loss: bool = True
    with_mvrc_loss: bool = True
    mlm_norm_in_batch_first: bool = False
    mvrc_norm_in_batch_first: bool = False

    @property
    def default_objective(self):
        return self.with_mlm_loss and self.with_mvrc_loss and not (self.mlm_norm_in_batch_first or self.mvrc_norm_in_batch_first)

    def validate(self):
        H, nh = self.hidden_size, self.num_attention_heads
        if H % 64 or H // nh != 64:
            raise ValueError("engine supports head dim 64 and hidden_size % 64 == 0 (got H=%d, heads=%d)" % (H, nh))
        if self.intermediate_size % 64:
            raise ValueError("intermediate_size must be a multiple of 64")
        if self.with_rel_loss and not self.with_pooler:
            raise ValueError("with_rel_loss needs with_pooler (the relationship head reads the pooled output)")
        if not (self.with_mlm_loss or self.with_mvrc_loss or self.with_rel_loss):
            raise ValueError("with_mlm_loss=False and with_mvrc_loss=False need with_rel_loss: there would be no loss to train on")


def param_layout(cfg):
    """Ordered {state_dict name: shape} -- the reference's key names (SURVEY.md §8b state-dict contract).
    Order matters: q/k/v weights (and biases) are adjacent so the fused [3H,H] QKV operand is a plain
    view; the two object linguistic vectors are adjacent so they form a [2,H] table."""
    H, I, V, C = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.visual_region_classes
    s = OrderedDict()
    s["vlbert.word_embeddings.weight"] = (V, H)
    s["vlbert.position_embeddings.weight"] = (cfg.max_position_embeddings, H)
    s["vlbert.token_type_embeddings.weight"] = (cfg.type_vocab_size, H)
    s["vlbert.end_embedding.weight"] = (1, H)
    s["object_linguistic_embeddings.weight"] = (1, H)
    if cfg.with_mvrc_loss:     # resnet_vlbert_for_pretraining.py:26-27
        s["object_mask_word_embedding.weight"] = (1, H)
    if cfg.multitask:
        s["aux_text_visual_embedding.weight"] = (1, H)     # resnet_vlbert_for_pretraining_multitask.py:28
    s["object_mask_visual_embedding.weight"] = (1, VIS_DIM)
    s["image_feature_extractor.obj_downsample.1.weight"] = (H, 2 * VIS_DIM)
    s["image_feature_extractor.obj_downsample.1.bias"] = (H,)
    for ln in ("embedding_LayerNorm", "visual_ln_text", "visual_ln_object"):
        s["vlbert.%s.weight" % ln] = (H,)
        s["vlbert.%s.bias" % ln] = (H,)
    for l in range(cfg.num_hidden_layers):
        p = "vlbert.encoder.layer.%d." % l
        for n in ("query", "key", "value"):
            s[p + "attention.self.%s.weight" % n] = (H, H)
        for n in ("query", "key", "value"):
            s[p + "attention.self.%s.bias" % n] = (H,)
        s[p + "attention.output.dense.weight"] = (H, H)
        s[p + "attention.output.dense.bias"] = (H,)
        s[p + "attention.output.LayerNorm.weight"] = (H,)
        s[p + "attention.output.LayerNorm.bias"] = (H,)
        s[p + "intermediate.dense.weight"] = (I, H)
        s[p + "intermediate.dense.bias"] = (I,)
        s[p + "output.dense.weight"] = (H, I)
        s[p + "output.dense.bias"] = (H,)
        s[p + "output.LayerNorm.weight"] = (H,)
        s[p + "output.LayerNorm.bias"] = (H,)
    if cfg.with_pooler:
        s["vlbert.pooler.dense.weight"] = (H, H)
        s["vlbert.pooler.dense.bias"] = (H,)
    if cfg.with_rel_loss:       # [sic] the typo is part of the reference's key (common/visual_linguistic_bert.py:322)
        s["vlbert.relationsip_head.caption_image_relationship.weight"] = (2, H)
        s["vlbert.relationsip_head.caption_image_relationship.bias"] = (2,)
    if cfg.with_mlm_loss:      # common/visual_linguistic_bert.py:323-326: a head exists only with its loss
        p = "vlbert.mlm_head.predictions."
        s[p + "transform.dense.weight"] = (H, H)
        s[p + "transform.dense.bias"] = (H,)
        s[p + "transform.LayerNorm.weight"] = (H,)
        s[p + "transform.LayerNorm.bias"] = (H,)
        s[p + "bias"] = (V,)
    if cfg.with_mvrc_loss:
        s["vlbert.mvrc_head.transform.dense.weight"] = (H, H)
        s["vlbert.mvrc_head.transform.dense.bias"] = (H,)
        s["vlbert.mvrc_head.region_cls_pred.weight"] = (C, H)
        s["vlbert.mvrc_head.region_cls_pred.bias"] = (C,)
    if cfg.e2e:      # trainable convolution weights of the vision path, LAST (their gradients complete last; parallel.GradBuckets)
        from .vision import vision_param_layout
        s.update(vision_param_layout(cfg.image_num_layers, cfg.image_frozen_stages))
    return s


TIED_DECODER_KEY = "vlbert.mlm_head.predictions.decoder.weight"   # alias of word_embeddings.weight (modeling.py:463-466)


class FlatParams:
    """One contiguous buffer per role (fp32 master / fp32 grad / Adam m / Adam v / bf16 copy); every
    tensor starts on a 64-element boundary (256 B fp32, 128 B bf16)."""

    def __init__(self, cfg, device, align=64):
        """align: the buffers' length is rounded up to it (parallel.shard_alignment(world): every data-parallel bucket then splits
        evenly over the ranks; the zero tail belongs to no parameter)."""
        self.shapes = param_layout(cfg)
        self.offsets = OrderedDict()
        off = 0
        for name, shape in self.shapes.items():
            self.offsets[name] = off
            off = _ru(off + math.prod(shape), 64)
        off = _ru(off, max(64, int(align)))
        self.numel = off
        self.master = torch.zeros(off, dtype=F32, device=device)
        self.grad = torch.zeros(off, dtype=F32, device=device)
        self.m = torch.zeros(off, dtype=F32, device=device)
        self.v = torch.zeros(off, dtype=F32, device=device)
        self.w16 = torch.zeros(off, dtype=ops.BF16, device=device)

    def view(self, buf, name, shape=None, span=1):
        """View of `name` in `buf`; span>1 extends over the following adjacent tensors."""
        names = list(self.shapes)
        i = names.index(name)
        n = sum(math.prod(self.shapes[k]) for k in names[i:i + span])
        if span > 1:   # adjacency requires no padding in between
            assert self.offsets[names[i + span - 1]] + math.prod(self.shapes[names[i + span - 1]]) - self.offsets[name] == n
        t = buf[self.offsets[name]:self.offsets[name] + n]
        return t.view(*(shape if shape is not None else self.shapes[name]))

    def named(self, buf):
        return OrderedDict((k, self.view(buf, k)) for k in self.shapes)


class PretrainEngine:
    def __init__(self, cfg, B, T, R, device="cuda:0", train=True, lr=1e-4, weight_decay=1e-4, max_grad_norm=10.0,
                 betas=(0.9, 0.999), eps=1e-6, seed=1234, grad_accum=1, process_group=None, keep_logits=False, flat=None,
                 B_aux=0, core=False, core_heads=True, core_sequence=False, lr_schedule=None, warmup_steps=0, t_total=0,
                 image_size=None, dp_mode="default", dp_wire="default", loss_scale=None, encoder_fp32=False, max_seq=256, fp32_ends=False, fp32_full=False,
                 train_metrics=False):
        cfg.validate()
        # train_metrics: every forward() also adds [top-1 hits, counted rows] per head to `train_metric_acc`, from the fused loss kernels
        # themselves (the ACC forms of csrc/loss.hip / csrc/f32_pretrain.hip) -- the reference's train_metrics (common/trainer.py:84,157-158).
        # Without it no launch changes.  Checked here, before anything is allocated
        self.train_metrics = bool(train_metrics)
        if self.train_metrics and core:
            raise ValueError("train_metrics=True needs an engine that owns the loss heads: core=True (the module-API engine) computes no "
                             "loss, so it has no training-time metrics (they belong to the wrapper that owns the labels)")
        # fp32_ends: the module-API front end (visual LayerNorms, fused embedding) and the hand-over of the sequence output run in fp32
        # too (csrc/f32_ends.hip), so that an encoder_fp32 engine holds no 16-bit tensor between its inputs and X[L].  One route only:
        # checked here, before anything is allocated
        self.fp32_ends = bool(fp32_ends)
        if self.fp32_ends:
            self._check_fp32_ends(cfg, T, R, core, core_heads, core_sequence, encoder_fp32, image_size, dp_mode, B_aux)
        # fp32_full: the pre-training step itself in fp32 -- this engine's own front end, the MLM / MVRC heads and both losses
        # (pretrain_f32.py, csrc/f32_pretrain.hip) around the fp32 encoder.  One configuration (precomputed features, no pooler, no
        # relationship loss, no text-only samples, no loss scale): checked here, before anything is allocated
        self.fp32_full = bool(fp32_full)
        if self.fp32_full:
            self._check_fp32_full(cfg, T, R, core, encoder_fp32, image_size, dp_mode, B_aux, loss_scale)
            loss_scale = 1.0
        # max_seq: the longest packed sequence S = T + R + 1 this engine may be built for, 256..512.  Up to 256 positions attention runs
        # the whole-sequence kernels (csrc/attention.hip), 257..512 the streaming ones (csrc/attention_long.hip: seven products per tile
        # pair instead of five).  The default stays 256 so that a caller opts into the long path knowingly.
        if not (isinstance(max_seq, int) and 256 <= max_seq <= MAX_SEQ):
            raise ValueError("max_seq must be an integer in 256..%d (got %r)" % (MAX_SEQ, max_seq))
        self.max_seq = max_seq
        if core and not cfg.default_objective:
            raise ValueError("the objective switches (with_mlm_loss / with_mvrc_loss / *_norm_in_batch_first) belong to the pre-training "
                             "engine: core=True (the module-API engine) computes no loss and always carries both heads")
        if cfg.e2e and (core or image_size is None):
            raise ValueError("e2e needs image_size=(H, W) and a pretraining wrapper (plain or multitask; not the core module mode)")
        # lr_schedule: None (host sets lr) | "constant" | "warmup_constant" | "triangle" (WarmupLinearSchedule,
        # pretrain/function/train.py:316-320) -- evaluated on the device from the step counter each optimizer step.
        kinds = {None: None, "constant": ops.LR_CONSTANT, "warmup_constant": ops.LR_WARMUP_CONSTANT,
                 "triangle": ops.LR_WARMUP_LINEAR, "warmup_linear": ops.LR_WARMUP_LINEAR}
        if lr_schedule not in kinds:
            raise ValueError("lr_schedule must be one of %s" % sorted(k for k in kinds if k))
        if kinds[lr_schedule] == ops.LR_WARMUP_LINEAR and t_total <= warmup_steps:
            raise ValueError("triangle schedule needs t_total > warmup_steps")
        self.lr_kind, self.base_lr, self.warmup_steps, self.t_total = kinds[lr_schedule], lr, warmup_steps, t_total
        self.cfg, self.B, self.T, self.R = cfg, B, T, R
        # Static loss scale (the reference's TRAIN.FP16_LOSS_SCALE, pretrain/function/train.py:345-352): d(loss)/d(logits) leaves the
        # loss kernels multiplied by it, every 16-bit gradient tensor and the flat fp32 gradient carry it, and the optimizer's
        # grad_scale divides it out (clip norm included).  1 in the bf16 build (fp32 exponent range); 4096 by default in the fp16
        # build (VLB_PRECISION=f16): d(logits) ~ 1/n_valid ~ 4e-4 at batch 256 would sit in fp16's subnormals otherwise.  Engines behind
        # the autograd mirrors (flat=... / core=True) hand their parameter gradients to torch unscaled, so they default to 1.
        # loss_scale="dynamic" / a loss_scale.DynamicLossScale (the reference's FP16_LOSS_SCALE: 'dynamic', Apex's dynamic scaler): the
        # scale lives in a device array (self.scaler) that the loss kernels multiply by and the optimizer kernels divide out; a step
        # whose squared gradient norm is not finite is skipped on the device, the scale halves, and doubles again after a window of
        # clean steps (loss_scale.py).  Static engines run exactly the launches they ran before.
        from . import loss_scale as LS
        self._scaler_spec = LS.resolve(loss_scale)
        self.scaler = None
        if self._scaler_spec is not None:
            if flat is not None or core:
                raise ValueError("loss_scale='dynamic' needs an engine that owns its optimizer step (not the flat=... / core=True modes)")
            self._loss_scale = None
        else:
            if loss_scale is None:
                loss_scale = 4096.0 if (ops.BF16 == torch.float16 and flat is None and not core) else 1.0
            self._loss_scale = float(loss_scale)
        # multitask: B_aux text-only samples are appended after the B image-caption samples; they have no
        # objects, their text-visual embedding is the learned aux_text_visual_embedding and their MLM loss is
        # accounted separately (resnet_vlbert_for_pretraining_multitask.py:96-290).  T = max(caption, aux) length.
        # core=True: the engine is driven through the module API of common/visual_linguistic_bert.py:95-171,346-380 --
        # per-token text-visual embeddings and [visual || linguistic] object embeddings come in as tensors, logits go
        # out, d(logits) comes back in (set_core_inputs / forward_core / backward_core); the FastRCNN front end, the
        # losses and the wrapper-level parameters are not used.
        self.core = core
        self.with_heads = core_heads or not core      # core_heads=False: hidden states out, d(hidden states) in
        self.seq_out = bool(core and core_sequence and not core_heads)   # the packed [B,S,H] sequence instead of text / object splits
        self.Ba = B_aux
        if B_aux and not cfg.multitask:
            raise ValueError("B_aux > 0 needs ModelConfig(multitask=True)")
        self.Bt = B + B_aux
        self.S = T + R + 1
        if self.S > MAX_SEQ:
            raise ValueError("sequence %d+%d+1 > %d: the fused attention kernels handle S <= %d" % (T, R, MAX_SEQ, MAX_SEQ))
        if self.S > max_seq:
            raise ValueError("sequence %d+%d+1 > max_seq=%d: build the engine with max_seq up to %d for longer sequences"
                             % (T, R, max_seq, MAX_SEQ))
        self.dev = torch.device(device)
        self.train = train
        self.grad_accum = grad_accum
        self.pg = process_group
        self.keep_logits = keep_logits
        H, I, V, C, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.visual_region_classes, cfg.num_hidden_layers
        self.M, self.BT, self.BR = self.Bt * self.S, self.Bt * T, B * R
        self.Mp, self.BTp, self.BRp = _ru(self.M, 64), _ru(self.BT, 64), _ru(self.BR, 64)
        self.Vp, self.Cp = _ru(V, 64), _ru(C, 64)
        d = self.dev
        import torch.distributed as dist
        world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self._own_flat = flat is None
        if flat is None:
            from .parallel import shard_alignment
            flat = FlatParams(cfg, d, align=shard_alignment(world))
        self.P = flat                                                # (`flat` given: storage shared with an nn.Module mirror)
        P = self.P
        self.w16 = P.named(P.w16)
        self.w32 = P.named(P.master)
        self.g32 = P.named(P.grad)
        if cfg.e2e:
            self.in_image = torch.zeros((B, 3, image_size[0], image_size[1]), dtype=F32, device=d)

        def zf(*s):
            return torch.zeros(s, dtype=F32, device=d)

        self._zero_small, self._fresh_grads = None, False

        # device-resident step state
        # odd (the advance kernel keeps it odd) and injective in `seed`: `seed | 1` collapsed ranks 2k / 2k+1 of a
        # seed = RNG_SEED + rank launch onto one dropout stream
        self.seed = torch.tensor([((seed * 2 + 1) & 0x7FFFFFFF)], dtype=torch.int32, device=d)
        self._seed_prev = torch.zeros_like(self.seed)      # the seed of the last forward once a step has advanced it (_advance_seed)
        self._last_p_a, self._seed_moved = None, False
        self.adam = torch.tensor([lr, betas[0], betas[1], eps, weight_decay, 0.0, max_grad_norm, 0.0], dtype=F32, device=d)
        self.hyper = dict(betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay))   # as given (checkpoints)
        if self._scaler_spec is not None:
            self.scaler = LS.LossScaler(self._scaler_spec, d)
        self.sumsq_ws = zf(2048)  # per-block partial sums of the gradient norm
        self.losses = zf(4)       # mlm (with visual content), mvrc, mlm (aux text), relationship
        self.counts = zf(4)       # n_valid mlm, n_valid mvrc, n_valid mlm aux
        # validation counters of eval_step(): [hits, counted rows] per row of METRIC_ROWS
        self.metric_acc = torch.zeros((4, 2), dtype=torch.int64, device=d)
        # training counters of forward() (train_metrics=True), same rows; a table of their own, allocated here so that a captured step
        # graph holds its address and validation in between (eval_step, the ValidationMonitor) keeps its own counts
        self.train_metric_acc = torch.zeros((4, 2), dtype=torch.int64, device=d) if self.train_metrics else None

        # static batch buffers (graph-capturable: the host copies new batches into them)
        self.in_boxes = zf(B, R, 4 + VIS_DIM)
        self.in_im_info = zf(B, 5)
        Bt = self.Bt
        self.in_text = torch.zeros((Bt, T), dtype=torch.int64, device=d)
        self.in_mlm_labels = torch.full((Bt, T), -1, dtype=torch.int64, device=d)
        self.in_mvrc_ops = torch.zeros((B, R), dtype=torch.int64, device=d)
        self.in_mvrc_labels = zf(B, R, C)
        self.in_rel_label = torch.zeros((B,), dtype=torch.int64, device=d)
        self.text_mask = torch.zeros((Bt, T), dtype=torch.uint8, device=d)
        self.box_mask = torch.zeros((Bt, R), dtype=torch.uint8, device=d)     # aux rows stay 0: no objects
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=d)
        self.lay = dict(code=i32(Bt, self.S), text_len=i32(Bt), nobj=i32(Bt), text_rows=i32(Bt, T), obj_rows=i32(Bt, R),
                        attn_mask=zf(Bt, self.S))

        # MLM head compaction (DESIGN.md "MLM head"): ~85 % of the text positions carry no label -- their logits are never read by the
        # loss and their d(logits) rows are exactly zero -- so transform -> LayerNorm -> decoder and the head's whole backward run on
        # the labelled rows only, gathered into the first `mlm_cap` rows of the same buffers.  Capacity is a contract with the data
        # pipeline (BERT masking labels 15 % of the valid tokens; at 16384 positions 20 % is 17 standard deviations away): 20 % of the B*T
        # positions rounded up to 256; a batch that exceeds it raises (the
        # device flag is checked at loss_values(); labels handed over as CPU tensors are counted exactly and such a batch simply
        # takes the full path).  Off with keep_logits (the module mirrors return every logit) and in module-API mode.  Batch state of
        # the engine (set_batch decides per batch); the heads -- 16-bit or fp32 -- own the buffers that go with it
        BT = self.BT
        cap = min(self.BTp, max(256, _ru(int(math.ceil(0.20 * BT)), 256)))
        want = os.environ.get("VLB_MLM_COMPACT", "1") != "0" and not keep_logits and not core and cap < BT and cfg.with_mlm_loss
        self.mlm_cap = cap if want else None
        self._mlm_compact_now = want

        # fp32 slab workspace for split-K weight gradients (largest request over this engine's wgrad shapes)
        need = [ops.wgrad_workspace_floats(n, k, rp) for n, k, rp in
                ((3 * H, H, self.Mp), (H, H, self.Mp), (I, H, self.Mp), (H, I, self.Mp), (V, H, self.BTp), (H, H, self.BTp),
                 (C, H, self.BRp), (H, H, self.BRp), (H, 2 * VIS_DIM, self.BRp))]
        need_dec = ops.wgrad_workspace_floats(self.BT, H, self.Vp)       # tied-decoder dgrad (K = vocabulary) at small batch
        need.append(need_dec)
        need.append(3 * (3 * H * H + H * H + 2 * I * H) + 64)             # grouped launch of a layer's four gradients, <= 3 K slices
        self.wg_ws = zf(max(max(need), 4))
        # Weight gradients run on a second stream: they only feed the optimizer, while the dgrad chain is the critical
        # path, and at small per-GPU batch neither fills the chip (312 + 432 workgroups for 512 slots at B = 32).
        # Hazards: a wgrad reads the gradient buffer the main stream produced (event after the producer) and the main
        # stream must not overwrite that buffer before the wgrad is done (event recorded after it, waited by the
        # next writer -- a full layer later thanks to the dD / dDb double buffer).  VLB_WGRAD_STREAM=0 serialises.
        self.side = torch.cuda.Stream(device=d) if (d.type == "cuda" and os.environ.get("VLB_WGRAD_STREAM", "1") != "0") else None
        self.wg_ws_main = zf(max(need_dec, 4)) if self.side is not None else self.wg_ws    # decoder dgrad split-K (main stream)
        self._hazards = SideStreams()
        self.ln_ws = zf(ops.ln_bwd_workspace_floats(H))     # per-workgroup partial dgamma/dbeta sums of the LayerNorm backward
        # The encoder's LayerNorm backwards (2 per layer + the MLM head's) leave their partial sums in a workspace slice of their
        # own; one batched launch (ops.ln_param_finalize_batch) adds them into the gradients when those are next needed -- a
        # bucket's all-reduce, or the end of backward -- instead of a 7-10 us finalize launch behind each of the 25 calls.
        self._ln_slices = list(zf(min(2 * L + 1, 32), ops.ln_bwd_workspace_floats(H)).unbind(0))
        self._ln_pending = []
        self.graph = None
        self._weights_dirty = True
        self.buckets = None
        # sharded optimizer: the weight gather of the last update may still be in flight (forward waits per bucket); the transposed /
        # folded weight copies are refreshed once it has landed (backward / the next forward of the vision path)
        self._wT_stale = self._gather_pending = self._vision_stale = False
        self._dp_hook = None         # set by parallel.DistributedDataParallel on the engines of a module mirror (shared flat buffers)
        from .parallel import force_exchange
        if (world > 1 or force_exchange()) and self._own_flat:      # (VLB_DP_FORCE_EXCHANGE: the exchange as identities in a world of one)
            from .parallel import GradBuckets
            vstart = min((o for n, o in self.P.offsets.items() if n.startswith("image_feature_extractor.") and
                          not n.startswith("image_feature_extractor.obj_downsample")), default=None)
            self.buckets = GradBuckets(self.P.grad, self.P.offsets, self.P.numel, L, group=process_group, vision_start=vstart,
                                       wire_dtype=dp_wire, mode=dp_mode)
            if self.buckets.sharded:
                # this rank's slice of every bucket: clip-norm partial + AdamW run on those only, one launch each (ops.ShardRanges);
                # wshard = the compact bf16 image of the updated slices the weight all-gather distributes (parallel.py)
                self.shard_tbl = ops.ShardRanges(self.buckets.owned_rows(), d)
                self.wshard = torch.zeros(self.P.numel // world, dtype=ops.BF16, device=d)
        # The three parts of the step, chosen here and nowhere else: `front` (inputs -> X[0] and back), `encoder` (X[0] -> X[L] and
        # back) and `back` (X[L] -> logits, losses, d X[L]).  Each is a plain object that owns every buffer only it touches and answers
        # the same few questions (transposes / refresh / overwritten, a front also grads); the step functions below call them in order
        # and never ask which they are.
        # encoder_fp32 (the reference's TRAIN.FP16: false configurations; encoder_f32.py): the layers run on fp32 tensors and the fp32
        # MASTER weights; the ends stay on the 16-bit kernels (use the fp16 build) and the encoder casts at its two boundaries, unless
        # fp32_ends (module API, sequence output: core_f32.py) or fp32_full (the pre-training step: pretrain_f32.py) make them fp32 too
        self.wT, self.vision, self.enc32, self.pre32 = {}, None, None, None      # wT: every 16-bit W^T copy of the dgrad GEMMs, by name
        if encoder_fp32:
            if self.buckets is not None and self.buckets.sharded:
                raise ValueError("encoder_fp32 reads the fp32 master weights on every rank: use dp_mode='allreduce' (the sharded optimizer "
                                 "keeps them authoritative on the owner only)")
            from .encoder_f32 import EncoderF32
            self.encoder = self.enc32 = EncoderF32(self, cast=not (self.fp32_ends or self.fp32_full))
            self.X = self.encoder.X16 if self.encoder.cast else self.encoder.X
        else:
            from .encoder_16 import Encoder16
            self.encoder = Encoder16(self)
            self.wT.update(self.encoder.wT)
            self._alias(self.encoder, "X", "QKV", "LSE")
        if self.fp32_full:
            from .pretrain_f32 import PretrainF32
            self.front = self.back = self.pre32 = PretrainF32(self)
        elif self.fp32_ends:
            from .core_f32 import CoreFrontF32, SequenceOutF32
            self.front, self.back = CoreFrontF32(self), SequenceOutF32(self)
        else:
            from .ends_16 import CoreFront16, Heads16, PretrainFront16
            self.front = CoreFront16(self) if core else PretrainFront16(self, image_size)
            self.back = Heads16(self)
            self.vision = None if core else self.front.vision
            self.wT.update(self.back.wT)
            self.wT.update(self.front.wT)
        self._parts = list(dict.fromkeys((self.encoder, self.back, self.front)))      # (one object may serve as front and back)
        # what callers read on the engine itself (tests, tools, the module mirrors): plain aliases of the parts' tensors
        self._alias(self.front, "st_objvis", "st_textvis", "st_emb", "st_tv")
        self._alias(self.back, "mlm_logits", "mlm_logits_copy", "mvrc_logits", "mvrc_logits_copy", "rel_logits", "rel_logits_copy",
                    "text_out", "obj_out", "pooled", "st_mlm", "mvrc_tsum", "labels_c", "sel_pos", "sel_src", "mlm_overflow")
        self._tbatch = None      # every 16-bit (weight, W^T copy) pair of the parts as one launch, built on first use
        over = [part.overwritten() for part in self._parts]
        self._overwritten = None if any(o is None for o in over) else [n for o in over for n in o]
        if self.buckets is not None and self.buckets.sharded:
            # the tensors forward / backward read from the fp32 MASTER (not from the gathered 16-bit copy) are replicated after
            # every owner-only update (parallel.GradBuckets.set_replicated_fp32)
            self.buckets.set_replicated_fp32(self._fp32_read_ranges())

    def _alias(self, part, *names):
        for n in names:
            if hasattr(part, n):
                setattr(self, n, getattr(part, n))

    @staticmethod
    def _check_fp32_ends(cfg, T, R, core, core_heads, core_sequence, encoder_fp32, image_size, dp_mode, B_aux):
        """fp32_ends covers the sequence-output module API on an fp32 encoder (the VQA fine-tuning route); everything else is named."""
        bad = []
        if not core:
            bad.append("core=False (the pre-training engine's own front end, MLM / MVRC / relationship heads and losses)")
        elif core_heads:
            bad.append("core_heads=True (the MLM / MVRC / relationship heads)")
        elif not core_sequence:
            bad.append("core_sequence=False (text and objects returned separately)")
        if not encoder_fp32:
            bad.append("encoder_fp32=False")
        if cfg.with_pooler:
            bad.append("with_pooler (the pooled output of VCR)")
        if cfg.e2e or image_size is not None:
            bad.append("the image branch (CNN, ROIAlign)")
        if B_aux:
            bad.append("B_aux > 0 (multitask text-only samples)")
        if dp_mode == "sharded":
            bad.append("dp_mode='sharded' (the sharded optimizer)")
        if T + R + 1 > 256:
            bad.append("a sequence of %d+%d+1 positions (the fp32 encoder handles at most 256)" % (T, R))
        if bad:
            raise ValueError("fp32_ends needs core=True, core_heads=False, core_sequence=True, encoder_fp32=True and no pooler; "
                             "unsupported here: " + "; ".join(bad))

    @staticmethod
    def _check_fp32_full(cfg, T, R, core, encoder_fp32, image_size, dp_mode, B_aux, loss_scale):
        """fp32_full covers the pre-training step of the precomputed-feature configuration on an fp32 encoder; everything else is named."""
        from . import loss_scale as LS
        bad = []
        if core:
            bad.append("core=True (the module-API engine; its sequence-output route is fp32_ends)")
        if not encoder_fp32:
            bad.append("encoder_fp32=False")
        if cfg.e2e or image_size is not None:
            bad.append("the image branch (CNN, ROIAlign)")
        if B_aux:
            bad.append("B_aux > 0 (multitask text-only samples)")
        if cfg.with_pooler or cfg.with_rel_loss:
            bad.append("with_pooler / with_rel_loss (the pooler and the relationship head and loss)")
        if not cfg.default_objective:
            bad.append("with_mlm_loss / with_mvrc_loss off or a *_norm_in_batch_first switch (the objective switches)")
        if dp_mode == "sharded":
            bad.append("dp_mode='sharded' (the sharded optimizer)")
        if loss_scale is not None and (LS.resolve(loss_scale) is not None or float(loss_scale) != 1.0):
            bad.append("loss_scale=%r (a loss scaler: fp32 gradients need none)" % (loss_scale,))
        if T + R + 1 > 256:
            bad.append("a sequence of %d+%d+1 positions (the fp32 encoder handles at most 256)" % (T, R))
        if bad:
            raise ValueError("fp32_full needs core=False, encoder_fp32=True, precomputed features, MLM + MVRC only and no loss scale; "
                             "unsupported here: " + "; ".join(bad))

    # ------------------------------------------------------------------------------------------
    # parameters
    # ------------------------------------------------------------------------------------------
    def load_state_dict(self, sd):
        """sd: {reference state_dict name: tensor}.  The tied decoder key is accepted and ignored."""
        vis = self._vision_names()
        for name in self.P.shapes:
            if name in vis:
                continue
            if name not in sd:
                raise KeyError("missing parameter %s" % name)
            self.w32[name].copy_(sd[name].to(F32))
        if self.vision is not None:     # conv weights ([O,I,KH,KW] in the reference) + BatchNorm tensors + frozen stages
            self.vision.load_state_dict(sd)
        self._weights_dirty = True

    def _fp32_read_ranges(self):
        """[(lo, hi)] of the flat buffer for every parameter the kernels read from the fp32 master: all 1-D tensors (Linear biases,
        LayerNorm gamma / beta, the decoder bias) and the mask visual embedding (obj_prep reads it as fp32).  Matrices and embedding
        tables are read through the 16-bit working copy; the e2e convolution weights travel as master slices with their buckets."""
        vis = self._vision_names()
        return [(self.P.offsets[n], self.P.offsets[n] + math.prod(sh)) for n, sh in self.P.shapes.items()
                if n not in vis and (len(sh) == 1 or n == "object_mask_visual_embedding.weight")]

    def _vision_names(self):
        if self.vision is None:
            return ()
        return {"image_feature_extractor." + k + ".weight" for k, c in self.vision.convs.items() if c.trainable}

    def state_dict(self):
        """With the sharded data-parallel optimizer the fp32 master is authoritative on the owning rank only: the slices are gathered
        first, so this is a COLLECTIVE there (call it on every rank, save on one)."""
        if self.buckets is not None and self.buckets.sharded:
            self.buckets.gather_master(self.P.master)
        vis = self._vision_names()
        sd = OrderedDict((k, v.detach().clone()) for k, v in self.w32.items() if k not in vis)
        if self.cfg.with_mlm_loss:      # (the decoder lives in the MLM head)
            sd[TIED_DECODER_KEY] = sd["vlbert.word_embeddings.weight"]
        if self.vision is not None:
            sd.update(self.vision.state_dict())
        return sd

    def sync_weights(self):
        """fp32 master -> bf16 working copy + transposed copies (after load / external modification)."""
        if self.buckets is not None:
            self.buckets.wait_params("all")
        self._wT_stale = self._gather_pending = self._vision_stale = False
        ops.cast_f32_bf16(self.P.master, self.P.w16)
        self._refresh_transposes()
        if self.vision is not None:
            self.vision.refresh_weights()
        self._weights_dirty = False

    def _refresh_transposes(self):
        """Every weight copy the parts read: the 16-bit W^T copies of the dgrad GEMMs (dX = dY W as an NT product) of all parts in
        one launch, all ~50 of them, then whatever each part derives from the weights itself (the fp32 parts' own transposes)."""
        if self._tbatch is None:
            self._tbatch = ops.TransposeBatch([p for part in self._parts for p in part.transposes()], self.dev)
        if self._tbatch.n:
            self._tbatch.run()
        for part in self._parts:
            part.refresh()

    # ------------------------------------------------------------------------------------------
    # batch
    # ------------------------------------------------------------------------------------------
    def set_batch(self, boxes, im_info, text, relationship_label, mlm_labels, mvrc_ops, mvrc_labels, aux_text=None,
                  aux_mlm_labels=None, image=None, mask_raw_pixels=False):
        """Copies a collated batch (pretrain/data/collate_batch.py layout) into the static device buffers
        and derives the masks exactly as resnet_vlbert_for_pretraining.py:106,134 does
        (box_mask = boxes[:,:,0] > -1.5 ; text_mask = text > 0).  `relationship_label` is only read
        with ModelConfig(with_rel_loss=True) (WITH_REL_LOSS is false in the north-star configuration).
        mask_raw_pixels (e2e): the image arrives UNMASKED and the pixels of the regions with mvrc_op == 1 are zeroed here, on the
        device copy -- the step the reference's dataset does per sample (conceptual_captions.py:201-206, MASK_RAW_PIXELS)."""
        B = self.B
        if self.mlm_cap is not None:    # labels still on the host: count them exactly (no sync) and take the full path if they do not fit
            self._mlm_compact_now = True
            if not mlm_labels.is_cuda and (aux_mlm_labels is None or not aux_mlm_labels.is_cuda):
                n_lab = int((mlm_labels >= 0).sum()) + (int((aux_mlm_labels >= 0).sum()) if aux_mlm_labels is not None else 0)
                self._mlm_compact_now = n_lab <= self.mlm_cap
        if self.vision is not None:     # e2e: `image` [B,3,H,W] fp32 (mean-subtracted, collate_batch.py), boxes [B,R,4]; features come from the CNN
            if image is None:
                raise ValueError("engine built with e2e=True needs image=")
            self.in_image.copy_(image, non_blocking=True)
        # the collator pads to the batch's own largest box count (pretrain/data/collate_batch.py:21,39): fewer slots than this engine's R
        # are completed with its padding markers (boxes -2, mvrc_ops 0, soft labels 0)
        Rb = boxes.shape[1]
        if Rb > self.R:
            raise ValueError("batch has %d box slots, engine was built for %d" % (Rb, self.R))
        if Rb < self.R:
            self.in_boxes[:, Rb:].fill_(-2.0)
            self.in_mvrc_ops[:, Rb:].zero_()
            self.in_mvrc_labels[:, Rb:].zero_()
        if self.vision is not None:
            self.in_boxes[:, :Rb, :4].copy_(boxes[:, :, :4], non_blocking=True)
        else:
            self.in_boxes[:, :Rb].copy_(boxes, non_blocking=True)
        self.in_im_info[:, :2].copy_(im_info[:, :2], non_blocking=True)      # (width, height); the datasets append 2-3 more columns
        if self.Ba or text.shape[1] != self.T:
            self.in_text.zero_()
            self.in_mlm_labels.fill_(-1)
        self.in_text[:B, :text.shape[1]].copy_(text, non_blocking=True)
        self.in_mlm_labels[:B, :mlm_labels.shape[1]].copy_(mlm_labels, non_blocking=True)
        if self.Ba:
            if aux_text is None or aux_text.shape[0] != self.Ba:
                raise ValueError("engine built with B_aux=%d needs aux_text of that many rows" % self.Ba)
            self.in_text[B:, :aux_text.shape[1]].copy_(aux_text, non_blocking=True)
            self.in_mlm_labels[B:, :aux_mlm_labels.shape[1]].copy_(aux_mlm_labels, non_blocking=True)
        self.in_mvrc_ops[:, :Rb].copy_(mvrc_ops, non_blocking=True)
        self.in_mvrc_labels[:, :Rb].copy_(mvrc_labels, non_blocking=True)
        if self.cfg.with_rel_loss:
            self.in_rel_label.copy_(relationship_label, non_blocking=True)
        torch.gt(self.in_text, 0, out=self.text_mask.view(torch.bool))
        torch.gt(self.in_boxes[:, :, 0], -1.5, out=self.box_mask[:B].view(torch.bool))
        if mask_raw_pixels:
            if self.vision is None:
                raise ValueError("mask_raw_pixels applies to the e2e configuration (precomputed features are masked by the "
                                 "object_mask_visual_embedding overwrite, resnet_vlbert_for_pretraining.py:114-117)")
            ops.mask_image_boxes(self.in_image, self.in_boxes, self.in_mvrc_ops)

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def _p(self, train):
        c = self.cfg
        if not train:
            return 0.0, 0.0, 0.0
        return c.hidden_dropout_prob, c.attention_probs_dropout_prob, c.obj_downsample_dropout

    def forward(self, train=None, gscale=1.0):
        train = self.train if train is None else train
        self._forward_to_logits(train)
        if not self.core:
            self._losses_fwd_bwd(gscale if self.scaler is not None else gscale * self.loss_scale, True)

    def _forward_to_logits(self, train):
        """Everything of a forward up to the logits (loss slots zeroed, losses not yet computed): shared by forward() and eval_step()."""
        if self._weights_dirty:
            self.sync_weights()
        p_h, p_a, p_ds = self._p(train)
        self.losses.zero_()
        ops.seq_layout_into(self.text_mask, self.box_mask, self.S, self.lay)
        stale = self._gather_pending
        if stale:    # sharded optimizer: the bf16 weights of the last update arrive bucket by bucket (parallel.gather_params)
            if self.vision is not None:
                self.buckets.wait_params("vision")
                if self._vision_stale:
                    self.vision.refresh_weights(trainable_only=True)
                    self._vision_stale = False
            self.buckets.wait_params("front")
        self.front.front_fwd(p_h, p_ds)
        self._last_p_a, self._seed_moved = p_a, False      # attention_probs() recomputes this forward's dropout masks
        self.encoder.forward(p_h, p_a)
        if stale:
            self.buckets.wait_params("heads")
            self._gather_pending = False
        self.back.heads_fwd()

    def _losses_fwd_bwd(self, gscale, keep):
        """Loss values + d(logits) written in place over the logits.  Called again by the nn.Module mirror (keep=False:
        logits restored from the kept copies, loss slots untouched) when autograd hands down an upstream scale != 1."""
        self.back.losses(gscale, keep)

    # ------------------------------------------------------------------------------------------
    # validation (forward only)
    # ------------------------------------------------------------------------------------------
    METRIC_ROWS = ("mlm", "mlm_aux", "mvrc", "relationship")      # rows of metric_acc; "mlm" = MLMAcc, or MLMAccWVC of the multitask model

    def eval_step(self):
        """One validation batch (the reference's do_validation body, pretrain/function/val.py:6-13, on the batch in the static input
        buffers): the forward with every dropout probability 0 up to the logits -- forward(train=False)'s own path, compaction / aux
        rows / e2e / fp32 encoder / relationship head included -- then the forward-only kernels of csrc/metrics.hip in place of the
        fused forward+backward losses.  Writes the four `losses` slots as a forward does and ADDS [hits, counted rows] per head to
        `metric_acc`; the logits stay as the GEMMs wrote them, and neither the dropout seed nor any gradient / optimizer state is
        touched.  No host synchronisation (read with metric_counts() / loss_values(), whose MLM-overflow contract applies)."""
        if self.core:
            raise ValueError("eval_step: the module-API engine has no loss heads (metrics belong to the wrapper that owns the labels)")
        self.back.eval_check()
        self._forward_to_logits(False)
        self.back.eval_losses()

    def reset_metrics(self):
        self.metric_acc.zero_()

    def metric_counts(self):
        """{head: (hits, counted rows)} accumulated by eval_step() since reset_metrics() (one host synchronisation)."""
        a = self.metric_acc.cpu()
        return {k: (int(a[i, 0]), int(a[i, 1])) for i, k in enumerate(self.METRIC_ROWS)}

    # ------------------------------------------------------------------------------------------
    # training-time metrics (train_metrics=True): counters of forward(), rows as METRIC_ROWS
    # ------------------------------------------------------------------------------------------
    def _need_train_metrics(self, what):
        if not self.train_metrics:
            raise ValueError("%s: the engine was built without train_metrics=True" % what)

    def reset_train_metrics(self):
        self._need_train_metrics("reset_train_metrics")
        self.train_metric_acc.zero_()

    def train_metric_counts(self):
        """{head: (hits, counted rows)} added by forward() since reset_train_metrics() (one host synchronisation)."""
        self._need_train_metrics("train_metric_counts")
        a = self.train_metric_acc.cpu()
        return {k: (int(a[i, 0]), int(a[i, 1])) for i, k in enumerate(self.METRIC_ROWS)}

    class _TrainMetricsSource(object):
        """What common/metrics.py's classes update() from, over the TRAINING counters: metric_acc = train_metric_acc, losses = the
        mean losses of the last forward (the reference's LossLogger reads them per batch), reset_metrics() zeroes the counters."""

        def __init__(self, eng):
            self.metric_acc, self.losses, self.reset_metrics = eng.train_metric_acc, eng.losses, eng.reset_train_metrics

    @property
    def train_metrics_source(self):
        self._need_train_metrics("train_metrics_source")
        return self._TrainMetricsSource(self)

    # ------------------------------------------------------------------------------------------
    # backward (explicit; weight gradients are ACCUMULATED into the flat fp32 grad buffer)
    # ------------------------------------------------------------------------------------------
    def _on_side(self, launch, items):
        """launch() on the side stream (inline without one); whoever overwrites a gradient operand `dy` of `items` next waits for it."""
        self._hazards.run(self.side, launch, [dy for dy, _, _, _ in items], writes=[g for _, _, gw, gb in items for g in (gw, gb)])

    def _wgrad(self, dy, x, gw, gb):
        """gw[N,K] (+)= dy^T x ; gb[N] += colsum(dy), straight from the row-major operands (LDS transpose reads), bias gradient fused."""
        acc = not self._fresh_grads
        self._on_side(lambda: ops.wgrad_tn(dy, x, gw, colsum=gb, workspace=self.wg_ws, accumulate=acc), [(dy, x, gw, gb)])

    def _before_write(self, *bufs):
        """Main stream is about to overwrite these buffers: wait for side-stream weight gradients still reading them."""
        self._hazards.before_write(*bufs)

    def _join_side(self):
        """All side-stream weight gradients issued so far complete before later main-stream work."""
        if self.side is not None:
            self._hazards.join([self.side])

    def _ln_bwd(self, dy, x, stats, gamma, dgamma, dbeta, **kw):
        if len(self._ln_pending) == len(self._ln_slices):
            self._flush_ln()                 # (more deferred calls than slices: the 24-layer model)
        ws = self._ln_slices[len(self._ln_pending)]
        slabs = ops.layernorm_bwd(dy, x, stats, gamma, dgamma=dgamma, dbeta=dbeta, workspace=ws, defer=True, **kw)
        if slabs:
            self._ln_pending.append((ws, slabs, dgamma, dbeta))

    def _flush_ln(self):
        if self._ln_pending:
            ops.ln_param_finalize_batch(self._ln_pending, self.cfg.hidden_size)
            self._ln_pending = []

    def backward(self, train=None, on_layer_done=None):
        will_launch = None
        if on_layer_done is None and self._dp_hook is not None:
            on_layer_done = self._dp_hook       # module mirror under parallel.DistributedDataParallel: exchange the flat gradient's buckets
        if on_layer_done is not None:       # a bucket is about to be reduced: the deferred LayerNorm parameter gradients first
            user_hook = on_layer_done
            will_launch = getattr(getattr(user_hook, "__self__", None), "will_launch", None)     # GradBuckets.on_done -> its predicate

            def on_layer_done(what):
                self._flush_ln()
                user_hook(what)
        train = self.train if train is None else train
        p_h, p_a, p_ds = self._p(train)
        if self._wT_stale:           # sharded optimizer: every gathered weight has landed by now -> the dgrad operands W^T
            self.buckets.wait_params("all")
            self._refresh_transposes()
            self._wT_stale = False
        if self.buckets is not None and on_layer_done is None:
            self.buckets.invalidate()      # (a micro-step without the exchange: the reduced images are stale until a hooked backward)
        dx = self.back.heads_bwd()          # d(logits) / the caller's gradients -> d X[L]
        if on_layer_done:
            self._join_side()
            on_layer_done("heads")
        dx = self.encoder.backward(dx, p_h, p_a, on_layer_done, will_launch)      # last layer first -> d X[0]
        # embed_bwd adds into the word-embedding gradient the decoder weight-gradient launch wrote: the front waits for the side
        # launches that wrote one of ITS gradient tensors, not for the encoder's last weight-gradient launch, which it runs beside.
        # With a bucket hook the exchange reads whole buckets behind the front: everything on the side stream completes first.
        if on_layer_done:
            self._join_side()
        else:
            self._hazards.before_accumulate(*self.front.grads())
        self.front.front_bwd(dx, p_h, p_ds, on_layer_done)
        self._join_side()
        self._flush_ln()
        self._fresh_grads = False       # a further backward before the next zero_grad() accumulates
        if on_layer_done:
            on_layer_done("embed")
            on_layer_done("vision")

    # ------------------------------------------------------------------------------------------
    # module-API mode (core=True)
    # ------------------------------------------------------------------------------------------
    def set_core_inputs(self, text_input_ids, text_token_type_ids, text_visual_embeddings, text_mask, object_vl_embeddings,
                        object_mask):
        """Arguments of VisualLinguisticBert.forward (common/visual_linguistic_bert.py:95-104), device tensors."""
        if not self.core:
            raise RuntimeError("engine was not built with core=True")
        Bt, T, R, H = self.Bt, self.T, self.R, self.cfg.hidden_size
        if tuple(text_input_ids.shape) != (Bt, T) or tuple(object_vl_embeddings.shape) != (Bt, R, 2 * H) or \
                tuple(text_visual_embeddings.shape) != (Bt, T, H):
            raise ValueError("core inputs must be text [%d,%d], text_visual [%d,%d,%d], object_vl [%d,%d,%d]"
                             % (Bt, T, Bt, T, H, Bt, R, 2 * H))
        self.in_text.copy_(text_input_ids)
        self.text_mask.view(torch.bool).copy_(text_mask)
        self.box_mask.view(torch.bool).copy_(object_mask)
        self.front.set_inputs(text_token_type_ids, text_visual_embeddings, object_vl_embeddings)      # in the front's own precision

    def forward_core(self, train=None):
        """-> (mlm_logits [B,T,V], mvrc_logits [B,R,C], text_out [B,T,H], obj_out [B,R,H], pooled [B,H] | None,
        relationship_logits [B,2] | None) as bf16 views of the back's buffers (all None where the back only hands the sequence over)."""
        self.forward(train)
        return self.back.outputs()

    def backward_core_hidden(self, d_text_out, d_obj_out, d_pooled=None, train=None):
        """core_heads=False: d(text_out) [B,T,H] / d(obj_out) [B,R,H] (/ d(pooled) [B,H]) -> input gradients (see backward_core)."""
        H, back = self.cfg.hidden_size, self.back
        if self.cfg.with_pooler:
            if d_pooled is None:
                back.d_pooled.zero_()
            else:
                back.d_pooled.copy_(d_pooled)
        if d_text_out is None:
            back.d_text_out.zero_()
        else:
            back.d_text_out.copy_(d_text_out.reshape(self.BT, H))
        if d_obj_out is None:
            back.d_obj_out.zero_()
        else:
            back.d_obj_out.copy_(d_obj_out.reshape(self.BR, H))
        self.backward(train)
        return self.front.input_grads()

    def sequence_output(self):
        """Last encoder layer as the packed [B, S, H] sequence (text || objects || END || padding): a view of what the back reads,
        16-bit, or the fp32 encoder's own X[L] where the back is fp32."""
        return self.encoder.x_out.view(self.Bt, self.S, self.cfg.hidden_size)

    # ------------------------------------------------------------------------------------------
    # inspection of the last forward (16-bit encoder): no per-layer state beyond what the forward leaves behind anyway
    # ------------------------------------------------------------------------------------------
    def longest_sequence(self):
        """The batch's longest packed sequence, text + objects + END (common/visual_linguistic_bert.py:202; one host synchronisation)."""
        return int((self.lay["text_len"] + self.lay["nobj"]).max()) + 1

    def _inspect_args(self, what, layers, n):
        if self.enc32 is not None:
            raise ValueError("%s() reads the 16-bit encoder's buffers; an encoder_fp32 engine keeps fp32 ones: read enc32.P "
                             "(enc32.Pd after dropout) / enc32.X" % what)
        if self._last_p_a is None:
            raise RuntimeError("%s() needs a forward first" % what)
        L = self.cfg.num_hidden_layers
        layers = list(range(L)) if layers is None else [int(l) for l in ([layers] if isinstance(layers, int) else layers)]
        if any(l < 0 or l >= L for l in layers):
            raise ValueError("%s(): layers must lie in 0..%d (got %r)" % (what, L - 1, layers))
        n = self.longest_sequence() if n is None else int(n)
        if not 1 <= n <= self.S:
            raise ValueError("%s(): n=%d outside 1..S=%d" % (what, n, self.S))
        return layers, n

    def attention_probs(self, layers=None, n=None):
        """Attention probabilities of the last forward (full step, eval_step or core), recomputed from the QKV and lse it left behind
        (csrc/attention_probs.hip): a list of fp32 [Bt, heads, n, n], one per layer in `layers` (default: all).  With the dropout
        probability, seed and tag of that forward: after a training-mode forward these are the probabilities AFTER their dropout, what
        the reference returns (modeling.py:311-316) -- also once optimizer_step() has advanced the seed: the forward's value is kept.  n defaults to the batch's longest packed sequence.  Each layer's buffer is
        allocated by the call; ask for one layer at a time where all of them together would not fit."""
        layers, n = self._inspect_args("attention_probs", layers, n)
        seed = self._seed_prev if self._seed_moved else self.seed      # optimizer_step has moved on: the forward's value was kept
        return self.encoder.attention_probs(layers, n, seed)

    def encoded_layers(self, layers=None, n=None):
        """Outputs of the encoder layers of the last forward: fp32 copies of X[l + 1] as [Bt, n, H], one per layer in `layers`."""
        layers, n = self._inspect_args("encoded_layers", layers, n)
        return self.encoder.encoded_layers(layers, n)

    def backward_core_sequence(self, d_seq, d_pooled=None, train=None):
        """core_sequence=True: d(sequence_output) [B, <=S, H] (rows beyond the given length are zero) -> input gradients."""
        H = self.cfg.hidden_size
        dx = self.back.dx.view(self.Bt, self.S, H)      # where the back leaves d X[L]: here the caller writes it
        dx.zero_()
        if d_seq is not None:
            dx[:, :d_seq.shape[1]].copy_(d_seq)
        if self.cfg.with_pooler:
            if d_pooled is None:
                self.back.d_pooled.zero_()
            else:
                self.back.d_pooled.copy_(d_pooled)
        self.backward(train)
        return self.front.input_grads()

    def backward_core(self, d_mlm_logits, d_mvrc_logits, d_rel_logits=None, train=None):
        """d(logits) [B,T,V] / [B,R,C] (any float dtype; None = zero) -> parameter gradients accumulated into the flat
        gradient, returns (d text_visual_embeddings [B,T,H], d object_vl_embeddings [B,R,2H]) as bf16 views."""
        V, C = self.cfg.vocab_size, self.cfg.visual_region_classes
        if d_mlm_logits is None:
            self.mlm_logits.zero_()
        else:
            self.mlm_logits[:, :V].copy_(d_mlm_logits.reshape(self.BT, V))
        if d_mvrc_logits is None:
            self.mvrc_logits.zero_()
        else:
            self.mvrc_logits[:, :C].copy_(d_mvrc_logits.reshape(self.BR, C))
        if self.cfg.with_rel_loss:
            if d_rel_logits is None:
                self.rel_logits.zero_()
            else:
                self.rel_logits[:, :2].copy_(d_rel_logits)
        self.backward(train)
        return self.front.input_grads()

    # ------------------------------------------------------------------------------------------
    # optimizer
    # ------------------------------------------------------------------------------------------
    def zero_grad(self):
        """Start of an optimizer step.  The Linear weight gradients (97 % of the buffer) are OVERWRITTEN by the first
        backward, so only the ranges that are accumulated with atomics are cleared."""
        if self._overwritten is None:      # a part ACCUMULATES its weight gradients, or may not run at all (overwritten() of the parts)
            self.P.grad.zero_()
            self._fresh_grads = False
            return
        if self._zero_small is None:
            covered = sorted((self.P.offsets[n], self.P.offsets[n] + math.prod(self.P.shapes[n])) for n in self._overwritten)
            ranges, cur = [], 0
            for lo, hi in covered:
                ranges.append((cur, lo))
                cur = hi
            ranges.append((cur, self.P.numel))
            self._zero_small = ops.ZeroRanges(self.P.grad, ranges)
        self._zero_small.run()
        self._fresh_grads = True

    def _gemm_weight_names(self):
        """Parameters whose gradient is produced (whole tensor) by exactly one weight-gradient product per backward: what the parts
        answer (overwritten()); empty where a part accumulates and zero_grad() therefore clears everything."""
        return list(self._overwritten or ())

    def optimizer_step(self, lr=None):
        """global-norm clip + AdamW + bf16 / transposed weight refresh + dropout seed advance.  With data
        parallelism the flat gradient holds the SUM over ranks; the 1/world average (DDP semantics,
        pretrain/function/train.py:89-90) is folded into the AdamW kernel's grad_scale."""
        if lr is not None:
            if self.lr_kind is not None:
                raise ValueError("optimizer_step(lr=...) conflicts with the device-side lr_schedule of this engine")
            self.adam[0:1].fill_(lr)
        sc = self.scaler.state if self.scaler is not None else None
        if self.lr_kind is not None:
            ops.lr_schedule_step(self.adam, self.lr_kind, self.base_lr, self.warmup_steps, self.t_total, scaler=sc)
        # dynamic loss scale: the kernels divide the device scale out themselves, skip the update when the (all-reduced) squared norm
        # is not finite -- every rank sees the same value, so every rank takes the same branch -- and then apply the scaler's rule.
        # Everything else in the step (weight refresh / gather, dropout seed) runs as usual, on unchanged data after a skip.
        scale = (self.buckets.grad_scale if self.buckets is not None else 1.0) / (1.0 if sc is not None else self.loss_scale)
        self._check_mlm_overflow_now_and_then()
        if self.buckets is not None and self.buckets.pending:
            self.buckets.wait()
        if self.buckets is not None and self.buckets.sharded:
            # sharded optimizer (parallel.py): this rank holds the reduced slices it owns; partial clip norm -> sum over ranks ->
            # AdamW on the owned slices -> the updated bf16 slices are all-gathered bucket by bucket under the next forward
            g = self.buckets.grad_shard
            self.shard_tbl.sumsq(g, self.sumsq_ws, self.adam[7:8])
            self.buckets.all_reduce_scalar(self.adam[7:8])
            self.shard_tbl.adamw(self.P.master, g, self.P.m, self.P.v, self.wshard, self.adam, grad_scale=scale, scaler=sc)
            self.buckets.gather_params(self.P.w16, self.wshard, master=self.P.master, vision_master=self.vision is not None)
            self._wT_stale = self._gather_pending = True
            self._vision_stale = self.vision is not None
            self._advance_seed()
            return
        # data parallel: the reduced gradient is read where the exchange left it (the bf16 wire image by default, parallel.py)
        grad = self.buckets.reduced if self.buckets is not None else self.P.grad
        ops.sumsq_det(grad, self.sumsq_ws, self.adam[7:8])     # fixed summation order: replicas stay bit-identical
        ops.adamw_step(self.P.master, grad, self.P.m, self.P.v, self.P.w16, self.adam, grad_scale=scale, scaler=sc)
        self._refresh_transposes()
        if self.vision is not None:
            self.vision.refresh_weights(trainable_only=True)
        self._advance_seed()

    def _advance_seed(self):
        """Fresh dropout masks for the next step.  The value the last forward drew from is kept (4 bytes, on the device, graph-
        replayable) so that attention_probs() can still regenerate that forward's masks after the step has finished."""
        self._seed_prev.copy_(self.seed)
        ops.rng_advance(self.seed)
        self._seed_moved = True

    def _check_mlm_overflow_now_and_then(self, every=64):
        """MLM head compaction with device-resident labels: the overflow flag (a batch with more labelled positions than mlm_cap ran
        truncated) is otherwise only read by loss_values(); loops that never call it get the check every `every` optimizer steps
        (one 4-byte readback)."""
        if self.mlm_cap is None and self.scaler is None:
            return
        self._opt_steps = getattr(self, "_opt_steps", 0) + 1
        if self._opt_steps % every == 0 and not torch.cuda.is_current_stream_capturing():
            self._periodic_host_checks()

    def _periodic_host_checks(self):
        if self.mlm_cap is not None:
            self._raise_on_mlm_overflow()
        if self.scaler is not None:
            self._raise_on_stuck_scaler()

    def _raise_on_stuck_scaler(self):
        """Dynamic loss scale: skipped_in_a_row >= 32 with the scale on its floor means the gradients still are not finite after every
        halving there was to take -- a run that would otherwise go on forever without training (one 36-byte readback).  A scale that
        is still above its floor (a gentle backoff factor, a very large start) is a run that is still recovering."""
        from .loss_scale import stuck
        v = self.scaler.values()
        if stuck(v):
            raise FloatingPointError("dynamic loss scale: %d optimizer steps in a row were skipped for non-finite gradients and the scale "
                                     "is at its floor (%g): the gradients are inf / NaN for a reason no loss scale can fix" % (int(v[6]), v[0]))

    def _raise_on_mlm_overflow(self):
        if int(self.mlm_overflow.cpu()) != 0:
            self.mlm_overflow.zero_()
            raise RuntimeError("MLM head compaction: a batch carried more than mlm_cap = %d labelled text positions (the excess was "
                               "not trained on).  Build the engine with VLB_MLM_COMPACT=0 or hand the labels over as CPU tensors "
                               "(they are then counted exactly and oversize batches take the full path)." % self.mlm_cap)

    # -- dropout seed discipline of the nn.Module mirrors (reference-style loop: net.train(); loss.backward(); optimizer.step()) --
    # Masks are never stored: forward and backward regenerate them from the device-resident seed, so the seed a backward sees must
    # be the one its forward used.  The mirrors therefore advance the seed BEFORE each training forward (not after it) and the
    # autograd nodes run their backward under the seed value snapshotted right after the forward (robust to interleaved
    # forward / backward orders and to several engines sharing autograd).
    def mirror_pre_forward(self, training):
        if training:
            if getattr(self, "_seed_used", False):
                ops.rng_advance(self.seed)
            self._seed_used = True

    def seed_snapshot(self):
        return self.seed.clone()

    class _SeedGuard:
        def __init__(self, eng, snap):
            self.eng, self.snap = eng, snap

        def __enter__(self):
            self.cur = self.eng.seed.clone()
            self.eng.seed.copy_(self.snap)

        def __exit__(self, *exc):
            self.eng.seed.copy_(self.cur)
            return False

    def seed_guard(self, snap):
        return PretrainEngine._SeedGuard(self, snap)

    def broadcast_parameters(self, src=0):
        """Rank `src`'s parameters, optimizer state and (e2e) frozen vision tensors to every rank -- the start-up broadcast of
        pretrain/function/train.py:331-334, so that a checkpoint loaded on rank 0 only cannot leave the replicas diverged."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(self.pg) == 1:
            return
        for t in (self.P.master, self.P.m, self.P.v, self.adam) + ((self.scaler.state,) if self.scaler is not None else ()):
            dist.broadcast(t, src=src, group=self.pg)
        if self.vision is not None:
            for t in self.vision.broadcast_tensors():
                dist.broadcast(t, src=src, group=self.pg)
        self._weights_dirty = True

    def train_step(self, lr=None):
        """zero_grad -> forward -> backward (gradient buckets all-reduced over RCCL as they complete,
        overlapped with the rest of backward) -> clip + AdamW: one optimizer step on the batch currently
        held in the static input buffers."""
        self.zero_grad()
        self.forward(True)
        self.backward(True, on_layer_done=self.buckets.on_done if self.buckets is not None else None)
        if self.buckets is not None:
            self.buckets.wait()
        self.optimizer_step(lr)

    def make_step_graph(self, lr=None):
        """train_step() captured as hipGraph SEGMENTS -> a callable that replays one optimizer step.  A captured graph cannot contain
        the RCCL calls of the data-parallel exchange (work handles, the communicator's own stream), so with more than one rank the
        step is cut at every collective: [graph] bucket launch [graph] ... wait [graph] norm all-reduce [graph] weight gather, and in
        the forward at every per-bucket wait of the sharded optimizer's weight gather -- ~2 x (buckets + 2) graph launches + as many
        collective calls per step instead of ~350 kernel launches from Python (host side ~5 ms -> ~1 ms; at 32 samples per GPU the
        device step is 5-6 ms, so the eager launch loop is the bound there).  One rank: a single graph.
        Call it in steady state (after at least one eager train_step on this engine); the batch is read from the static input
        buffers (set_batch between replays is fine), lr / step count / dropout seed live on the device."""
        return _SegmentedStep(self, lr)

    # ------------------------------------------------------------------------------------------
    # results (host side, sync) -- used by tests / API parity, not by the timed loop
    # ------------------------------------------------------------------------------------------
    def loss_values(self):
        if self.mlm_cap is not None:
            self._raise_on_mlm_overflow()
        l = self.losses.cpu()
        from . import _lib
        bad = _lib.nonfinite_status(reset=True)
        if bad:
            raise FloatingPointError("non-finite LayerNorm input (%s): %s" % (
                "fp16 residual stream" if bad & 1 else "bf16 rows",
                "a pre-LayerNorm sum exceeded the fp16 range (65504); run with VLB_RESIDUAL_STREAM=bf16" if bad & 1
                else "the activations already held inf / NaN"))
        out = dict(mlm_loss=float(l[0]), mvrc_loss=float(l[1]), relationship_loss=float(l[3]), loss=float(l[0] + l[1] + l[2] + l[3]))
        if self.Ba:
            out.update(mlm_loss_wvc=float(l[0]), mlm_loss_aux=float(l[2]))
        return out

    @property
    def loss_scale(self):
        """The loss scale as a plain float: the constructor's value for a static engine; for a dynamic one the device value (one
        4-byte readback: not for the timed loop)."""
        if self.scaler is not None:
            return float(self.scaler.scale.cpu())
        return self._loss_scale

    @loss_scale.setter
    def loss_scale(self, value):
        if self.scaler is not None:
            raise AttributeError("the loss scale of a dynamic engine lives on the device (eng.scaler)")
        self._loss_scale = float(value)

    def scaler_state(self):
        """{scale, growth_factor, backoff_factor, growth_interval, unskipped, skipped_total, skipped_in_a_row, min_scale, max_scale} of a
        dynamic engine, with one readback; None for a static one."""
        return self.scaler.read() if self.scaler is not None else None

    def grads(self):
        """Parameter gradients of the local batch (the loss scale divided out).  With a dynamic loss scale this and grad_norm() divide
        by the CURRENT device scale: valid between backward() and optimizer_step(), which may halve or grow it."""
        inv = 1.0 / self.loss_scale
        return OrderedDict((k, v.detach().clone() * inv if inv != 1.0 else v.detach().clone()) for k, v in self.g32.items())

    def grad_norm(self):
        return float(self.P.grad.double().norm()) / self.loss_scale

    def init_random(self, seed=0, visual_ln_init=0.0):
        """Reference initialisation statistics on the device (BaseModel.init_weights,
        common/visual_linguistic_bert.py:14-25,330-332; resnet_vlbert_for_pretraining.py:55-63): N(0, 0.02)
        weights / embeddings, zero biases, unit LayerNorm gammas, visual_ln gammas = visual_scale_*_init,
        zero mask-visual embedding.  Used by bench.py / smoke (no checkpoints exist offline)."""
        g = torch.Generator(device=self.dev).manual_seed(seed)
        vis = self._vision_names()
        if self.vision is not None:
            self.vision.init_random(seed + 1)
        for name, t in self.w32.items():
            if name in vis:
                continue
            if "LayerNorm.weight" in name:
                t.fill_(1.0)
            elif name.endswith("visual_ln_text.weight") or name.endswith("visual_ln_object.weight"):
                t.fill_(visual_ln_init)
            elif name.endswith(".bias") or name == "object_mask_visual_embedding.weight":
                t.zero_()
            else:
                t.normal_(0.0, 0.02, generator=g)
        self._weights_dirty = True


class _SegmentedStep:
    """Capture of PretrainEngine.train_step as alternating [hipGraph segment] / [host call] items (PretrainEngine.make_step_graph)."""

    class _Recorder:
        """Stands in for engine.buckets during capture: the calls that start or wait for a collective END the current segment, are
        recorded (not executed: nothing runs during capture) and a new segment begins; everything else is delegated."""
        BREAKS = ("on_done", "wait", "all_reduce_scalar", "gather_params", "wait_params", "gather_master")

        def __init__(self, real, owner):
            self._real, self._owner = real, owner

        def __getattr__(self, name):
            attr = getattr(self._real, name)
            if name not in self.BREAKS:
                return attr
            owner = self._owner

            def recorded(*a, **kw):
                if name == "wait_params":       # only where a wait can block: gathers pending, and an encoder layer that opens a bucket
                    if not owner.eng._gather_pending or (isinstance(a[0], int) and self._real.layer_key[a[0]] != a[0]):
                        return None
                if name == "on_done" and not self._real.will_launch(a[0]):
                    return None
                owner.cut(lambda: attr(*a, **kw))
            recorded.__self__ = self             # (engine.backward looks up the hook owner's will_launch predicate)
            return recorded

    CHECK_EVERY = 64

    def __init__(self, eng, lr):
        if not eng.dev.type == "cuda":
            raise RuntimeError("make_step_graph needs a GPU engine")
        self.eng, self.items = eng, []
        self.replays = 0
        self.pool = torch.cuda.graph_pool_handle()
        self.stream = torch.cuda.Stream(device=eng.dev)
        self._g = None
        torch.cuda.synchronize()
        real = eng.buckets
        if real is not None:
            if real.pending or real.launched:
                raise RuntimeError("make_step_graph: a data-parallel exchange is in flight")
            real.wait_params("all")          # weight gathers of the last eager step: let them land before anything is captured
            torch.cuda.synchronize()
            eng.buckets = self._Recorder(real, self)
        try:
            self._begin()
            eng.train_step(lr)
            self._end()
        finally:
            eng.buckets = real
        torch.cuda.synchronize()
        self.n_graphs = sum(1 for k, _ in self.items if k == "graph")
        self.n_calls = len(self.items) - self.n_graphs

    def _begin(self):
        self._g = torch.cuda.CUDAGraph()
        # thread_local: the collective backend's helper threads (gloo's host copies, RCCL's proxy) keep making runtime calls while this
        # thread captures; under the default "global" mode any of them invalidates the capture
        self._ctx = torch.cuda.graph(self._g, pool=self.pool, stream=self.stream, capture_error_mode="thread_local")
        self._ctx.__enter__()

    def _end(self):
        self._ctx.__exit__(None, None, None)
        self.items.append(("graph", self._g))
        self._g = None

    def cut(self, fn):
        self._end()
        self.items.append(("call", fn))
        self._begin()

    def __call__(self):
        for kind, x in self.items:
            if kind == "graph":
                x.replay()
            else:
                x()
        # optimizer_step's periodic host-side checks ran once, at capture: the replay loop carries them itself (MLM head compaction
        # overflow flag, one 4-byte readback every CHECK_EVERY replays -- never a silent truncation of the labelled positions)
        self.replays += 1
        # (and, with a dynamic loss scale, the scaler's skipped_in_a_row counter: a run pinned at the floor must not go on silently)
        if self.replays % self.CHECK_EVERY == 0 and (self.eng.mlm_cap is not None or self.eng.scaler is not None):
            self.eng._periodic_host_checks()
