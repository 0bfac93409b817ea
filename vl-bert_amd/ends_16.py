"""16-bit ends of the engine, around whichever encoder it was built with: the pre-training front end (PretrainFront16), the
module-API front end (CoreFront16) and the hand-over, heads and losses behind the encoder (Heads16).  Each owns the buffers it uses
and the transposed weight copies its data gradients read; the engine supplies the flat parameters, the input buffers, `lay`, the seed,
the loss / count / metric slots and the side-stream weight gradients (_wgrad).  The neighbours' tensors they touch are the encoder's
x_in (written by a front), x_out and dx_in (read / written by the heads).

Reference code replaced: common/fast_rcnn.py:165-175 and common/visual_linguistic_bert.py:173-241 (fronts), :146-166, the pooler and
heads of modeling.py:424-472 / visual_linguistic_bert.py:505-531 and the losses of resnet_vlbert_for_pretraining.py:150-216 (heads).
"""
import torch

from . import ops
from .engine import F32, TAG_DOWNSAMPLE, TAG_EMBED, VIS_DIM

EMBED_GRADS = ("vlbert.word_embeddings.weight", "vlbert.position_embeddings.weight", "vlbert.token_type_embeddings.weight",
               "vlbert.end_embedding.weight", "vlbert.embedding_LayerNorm.weight", "vlbert.embedding_LayerNorm.bias",
               "vlbert.visual_ln_text.weight", "vlbert.visual_ln_text.bias", "vlbert.visual_ln_object.weight",
               "vlbert.visual_ln_object.bias")
PRETRAIN_FRONT_GRADS = EMBED_GRADS + (
    "object_linguistic_embeddings.weight", "object_mask_word_embedding.weight", "aux_text_visual_embedding.weight",
    "object_mask_visual_embedding.weight", "image_feature_extractor.obj_downsample.1.weight", "image_feature_extractor.obj_downsample.1.bias")

# the heads' GEMM weights (each has a W^T copy in Heads16.wT)
MLM_T = "vlbert.mlm_head.predictions.transform.dense.weight"
WORD = "vlbert.word_embeddings.weight"
MVRC_T = "vlbert.mvrc_head.transform.dense.weight"
MVRC_C = "vlbert.mvrc_head.region_cls_pred.weight"
POOL = "vlbert.pooler.dense.weight"
REL = "vlbert.relationsip_head.caption_image_relationship.weight"


def _zeros(eng, dtype):
    return lambda *s: torch.zeros(s, dtype=dtype, device=eng.dev)


class PretrainFront16:
    """Object preparation -> obj_downsample -> visual LayerNorms -> fused embedding, forward and backward; with e2e the vision stack
    (CNN trunk, ROIAlign, RoI head) that produces the region features hangs off it."""

    def __init__(self, eng, image_size):
        self.eng = eng
        cfg, B, R, Bt, BR, M, H = eng.cfg, eng.B, eng.R, eng.Bt, eng.BR, eng.M, eng.cfg.hidden_size
        zb, zf = _zeros(eng, ops.BF16), _zeros(eng, F32)
        self.vision = None
        if cfg.e2e:
            from .vision import VisionStack
            self.vision = VisionStack(B, image_size[0], image_size[1], R, device=eng.dev, num_layers=cfg.image_num_layers,
                                      frozen_stages=cfg.image_frozen_stages, storage=lambda n, shape: (eng.w32[n], eng.g32[n]))
        self.wT = {"image_feature_extractor.obj_downsample.1.weight": zb(2 * VIS_DIM, H)}
        self.a_ds = zb(BR, 2 * VIS_DIM)
        self.obj_reps = zb(BR, H)
        self.objvis, self.st_objvis = zb(BR, H), zf(BR, 2)
        self.textvis, self.st_textvis = zb(Bt, H), zf(Bt, 2)
        self.emb_pre, self.st_emb = zb(M, H), zf(M, 2)
        self.d_textvis, self.d_objvis = zf(Bt, H), zf(BR, H)
        self.d_obj_reps = zf(BR, H)
        self.d_yds = zb(BR, H)
        self.d_afeat = zb(BR, VIS_DIM)
        self.x0 = eng.encoder.x_in
        if cfg.with_mvrc_loss:
            self.ling_idx = eng.in_mvrc_ops
            self.g_ling_table = eng.P.view(eng.P.grad, "object_linguistic_embeddings.weight", (2, H), span=2)
        else:
            # without the MVRC loss there is no object_mask_word_embedding (resnet_vlbert_for_pretraining.py:26-27, 140-141): every
            # region reads row 0 of the table, through an all-zero selector in place of mvrc_ops.  embed_bwd writes a two-row table
            # gradient whatever the selector holds, and the flat gradient has one row here: it gets a two-row scratch table of its own,
            # whose row 0 front_bwd adds to the parameter's gradient (row 1 takes nothing and is never read)
            self.ling_idx = torch.zeros_like(eng.in_mvrc_ops)
            self.g_ling_scratch = self.g_ling_table = zf(2, H)

    def transposes(self):
        n = "image_feature_extractor.obj_downsample.1.weight"
        return [(self.eng.w16[n], self.wT[n])]

    def refresh(self):
        pass

    def overwritten(self):
        return ["image_feature_extractor.obj_downsample.1.weight"]

    def grads(self):
        """Every gradient tensor front_bwd adds into or overwrites on the main stream (or hands to a side launch of its own)."""
        return [self.eng.g32[n] for n in PRETRAIN_FRONT_GRADS if n in self.eng.g32]

    def front_fwd(self, p_h, p_ds):
        e = self.eng
        B, T, R, S, Bt, Ba, H = e.B, e.T, e.R, e.S, e.Bt, e.Ba, e.cfg.hidden_size
        w16, w32, seed = e.w16, e.w32, e.seed
        # --- e2e: ResNet trunk -> ROIAlign -> layer4 head -> avg-pool, written into the feature slots of in_boxes; the raw
        #     pixels are masked by the dataset, so no mask embedding is substituted (mask_visual_embed=None, :120-127) ----
        e2e = self.vision is not None
        if e2e:
            self.vision.forward(e.in_image, e.in_boxes)
        # --- FastRCNN: (coord || feature) -> Dropout -> Linear(4096->H) -> ReLU (common/fast_rcnn.py:165-175) -------
        ops.obj_prep_fwd(e.in_boxes, e.in_im_info, None if e2e else e.in_mvrc_ops.view(-1),
                         w32["object_mask_visual_embedding.weight"], self.a_ds, drop_p=p_ds, seed=seed, tag=TAG_DOWNSAMPLE)
        ops.gemm_nt(self.a_ds, w16["image_feature_extractor.obj_downsample.1.weight"], self.obj_reps,
                    bias=w32["image_feature_extractor.obj_downsample.1.bias"], act=ops.ACT_RELU)
        ops.zero_padded_rows(self.obj_reps, e.in_boxes)      # pad_sequence zeros (a padded box 0 feeds the text tokens' visual embedding)
        # --- visual LayerNorms + fused embedding ---------------------------------------------------------
        ops.layernorm_fwd(self.obj_reps, w32["vlbert.visual_ln_object.weight"], w32["vlbert.visual_ln_object.bias"], self.objvis,
                          self.st_objvis)
        reps0 = self.obj_reps.view(B, R * H)[:, :H]          # obj_reps[:, 0]  (text tags are all 0, :132-135)
        ops.layernorm_fwd(reps0, w32["vlbert.visual_ln_text.weight"], w32["vlbert.visual_ln_text.bias"], self.textvis[:B],
                          self.st_textvis[:B])
        if Ba:   # aux text-only samples: every token sees LN(aux_text_visual_embedding) (multitask.py:176)
            ops.layernorm_fwd(w16["aux_text_visual_embedding.weight"], w32["vlbert.visual_ln_text.weight"],
                              w32["vlbert.visual_ln_text.bias"], self.textvis[B:], self.st_textvis[B:], rows=Ba, ldx=0)
        ops.embed_fwd(e.lay, e.in_text, None, w16["vlbert.word_embeddings.weight"], w16["vlbert.position_embeddings.weight"],
                      w16["vlbert.token_type_embeddings.weight"], w16["vlbert.end_embedding.weight"], self.textvis, (H, 0),
                      self.objvis, (R * H, H), w16["object_linguistic_embeddings.weight"], (0, 0), self.ling_idx,
                      w32["vlbert.embedding_LayerNorm.weight"], w32["vlbert.embedding_LayerNorm.bias"], self.emb_pre, self.st_emb,
                      self.x0, Bt, T, R, S, H, drop_p=p_h, seed=seed, tag=TAG_EMBED)

    def front_bwd(self, dx, p_h, p_ds, on_layer_done=None):
        e = self.eng
        B, T, R, S, Bt, Ba, H = e.B, e.T, e.R, e.S, e.Bt, e.Ba, e.cfg.hidden_size
        w16, w32, g32, seed = e.w16, e.w32, e.g32, e.seed
        # --- embedding + visual LayerNorms + obj_downsample ---------------------------------------------
        self.d_objvis.zero_()
        self.d_obj_reps.zero_()
        self.d_textvis.zero_()
        pe = "vlbert.embedding_LayerNorm."
        scratch = getattr(self, "g_ling_scratch", None)
        if scratch is not None:
            scratch.zero_()
        ops.embed_bwd(dx, self.emb_pre, self.st_emb, w32[pe + "weight"], e.lay, e.in_text, None, self.ling_idx,
                      g32["vlbert.word_embeddings.weight"], g32["vlbert.position_embeddings.weight"],
                      g32["vlbert.token_type_embeddings.weight"], g32["vlbert.end_embedding.weight"], g32[pe + "weight"],
                      g32[pe + "bias"], self.d_textvis, (H, 0), self.d_objvis, (R * H, H), self.g_ling_table, (0, 0), Bt, T, R, S, H,
                      drop_p=p_h, seed=seed, tag=TAG_EMBED, text_vis_zeroed=True)
        if scratch is not None:
            ops.add_rows_f32(g32["object_linguistic_embeddings.weight"], scratch[:1])
        if on_layer_done:      # the tied word-embedding gradient (decoder wgrad + this scatter-add) is complete: its 94 MB go out first
            on_layer_done("word_emb")
        ops.layernorm_bwd(self.d_objvis, self.obj_reps, self.st_objvis, w32["vlbert.visual_ln_object.weight"],
                          dx_acc=self.d_obj_reps, dgamma=g32["vlbert.visual_ln_object.weight"],
                          dbeta=g32["vlbert.visual_ln_object.bias"], workspace=e.ln_ws)
        reps0 = self.obj_reps.view(B, R * H)[:, :H]
        ops.layernorm_bwd(self.d_textvis[:B], reps0, self.st_textvis[:B], w32["vlbert.visual_ln_text.weight"],
                          dx_acc=self.d_obj_reps.view(B, R * H)[:, :H], dgamma=g32["vlbert.visual_ln_text.weight"],
                          dbeta=g32["vlbert.visual_ln_text.bias"])
        if Ba:   # all aux samples share one input row: stride-0 input, gradient accumulated into the single parameter row
            ops.layernorm_bwd(self.d_textvis[B:], w16["aux_text_visual_embedding.weight"], self.st_textvis[B:],
                              w32["vlbert.visual_ln_text.weight"], dx_acc=g32["aux_text_visual_embedding.weight"],
                              dgamma=g32["vlbert.visual_ln_text.weight"], dbeta=g32["vlbert.visual_ln_text.bias"],
                              rows=Ba, ldx=0, ldacc=0)
        ops.relu_bwd_cast(self.d_obj_reps, self.obj_reps, self.d_yds)
        pd = "image_feature_extractor.obj_downsample.1."
        e._wgrad(self.d_yds, self.a_ds, g32[pd + "weight"], g32[pd + "bias"])
        # gradient of the mask embedding: feature half of dA = dY W, masked regions only
        ops.gemm_nt(self.d_yds, self.wT[pd + "weight"][VIS_DIM:], self.d_afeat)
        if self.vision is not None:      # the features are activations of the CNN: RoI head, ROIAlign and trunk backward
            e._join_side()
            hook = None
            if on_layer_done:     # everything but the convolutions is complete: its bucket goes out under the CNN backward
                on_layer_done("embed")
                hook = lambda layer: on_layer_done("vision%d" % layer)
            self.vision.backward(self.d_afeat, e.in_boxes, drop_p=p_ds, seed=seed, tag=TAG_DOWNSAMPLE, on_stage_done=hook)
            return
        ops.masked_colsum(self.d_afeat, e.in_mvrc_ops.view(-1), g32["object_mask_visual_embedding.weight"].view(-1),
                          drop_p=p_ds, seed=seed, tag=TAG_DOWNSAMPLE, row_elems=2 * VIS_DIM, col_off=VIS_DIM)


class CoreFront16:
    """VisualLinguisticBert.embedding (common/visual_linguistic_bert.py:173-241) on caller-provided embeddings: the inputs as 16-bit
    copies, the two visual LayerNorms, the fused embedding, and the gradients handed back to autograd."""

    def __init__(self, eng):
        self.eng = eng
        T, Bt, BT, BR, M, H = eng.T, eng.Bt, eng.BT, eng.BR, eng.M, eng.cfg.hidden_size
        zb, zf = _zeros(eng, ops.BF16), _zeros(eng, F32)
        # the transposed obj_downsample weight is not read here; it stays in the batched transpose so that the launch of the
        # module-API engines keeps its item count
        self.wT = {"image_feature_extractor.obj_downsample.1.weight": zb(2 * VIS_DIM, H)}
        self.in_text_type = torch.zeros((Bt, T), dtype=torch.int64, device=eng.dev)
        self.tv_in, self.ovl_in = zb(BT, H), zb(BR, 2 * H)          # inputs as bf16: text_visual [B,T,H], object_vl [B,R,2H]
        self.tv_n, self.st_tv = zb(BT, H), zf(BT, 2)                # visual_ln_text per token
        self.objvis, self.st_objvis = zb(BR, H), zf(BR, 2)
        self.emb_pre, self.st_emb = zb(M, H), zf(M, 2)
        self.d_tv_n, self.d_objvis, self.d_ol = zf(BT, H), zf(BR, H), zf(BR, H)   # d(LN(text_visual)), d(LN(object visual half)), d(object linguistic half)
        self.d_tv_in, self.d_ovl_in = zb(BT, H), zb(BR, 2 * H)      # gradients handed back to autograd
        self.x0 = eng.encoder.x_in

    def transposes(self):
        n = "image_feature_extractor.obj_downsample.1.weight"
        return [(self.eng.w16[n], self.wT[n])]

    def refresh(self):
        pass

    def overwritten(self):
        """None: nothing is overwritten.  The module mirrors accumulate (autograd semantics, several engines on one flat gradient) and
        may run without the heads, so the whole flat gradient is cleared and every product adds."""
        return None

    def grads(self):
        return [self.eng.g32[n] for n in EMBED_GRADS]

    def set_inputs(self, text_token_type_ids, text_visual_embeddings, object_vl_embeddings):
        e = self.eng
        self.in_text_type.copy_(text_token_type_ids)
        self.tv_in.view(e.Bt, e.T, -1).copy_(text_visual_embeddings)            # dtype conversion to bf16 (glue)
        self.ovl_in.view(e.Bt, e.R, -1).copy_(object_vl_embeddings)

    def input_grads(self):
        e, H = self.eng, self.eng.cfg.hidden_size
        return self.d_tv_in.view(e.Bt, e.T, H), self.d_ovl_in.view(e.Bt, e.R, 2 * H)

    def front_fwd(self, p_h, p_ds):
        e = self.eng
        T, R, S, Bt, H = e.T, e.R, e.S, e.Bt, e.cfg.hidden_size
        w16, w32 = e.w16, e.w32
        ops.layernorm_fwd(self.tv_in, w32["vlbert.visual_ln_text.weight"], w32["vlbert.visual_ln_text.bias"], self.tv_n, self.st_tv)
        ops.layernorm_fwd(self.ovl_in[:, :H], w32["vlbert.visual_ln_object.weight"], w32["vlbert.visual_ln_object.bias"], self.objvis,
                          self.st_objvis)
        ops.embed_fwd(e.lay, e.in_text, self.in_text_type, w16["vlbert.word_embeddings.weight"],
                      w16["vlbert.position_embeddings.weight"], w16["vlbert.token_type_embeddings.weight"],
                      w16["vlbert.end_embedding.weight"], self.tv_n, (T * H, H), self.objvis, (R * H, H),
                      self.ovl_in[:, H:], (R * 2 * H, 2 * H), None, w32["vlbert.embedding_LayerNorm.weight"],
                      w32["vlbert.embedding_LayerNorm.bias"], self.emb_pre, self.st_emb, self.x0, Bt, T, R, S, H, drop_p=p_h,
                      seed=e.seed, tag=TAG_EMBED)

    def front_bwd(self, dx, p_h, p_ds, on_layer_done=None):
        e = self.eng
        T, R, S, Bt, H = e.T, e.R, e.S, e.Bt, e.cfg.hidden_size
        w32, g32 = e.w32, e.g32
        self.d_tv_n.zero_()
        self.d_objvis.zero_()
        self.d_ol.zero_()
        pe = "vlbert.embedding_LayerNorm."
        ops.embed_bwd(dx, self.emb_pre, self.st_emb, w32[pe + "weight"], e.lay, e.in_text, self.in_text_type, None,
                      g32["vlbert.word_embeddings.weight"], g32["vlbert.position_embeddings.weight"],
                      g32["vlbert.token_type_embeddings.weight"], g32["vlbert.end_embedding.weight"], g32[pe + "weight"],
                      g32[pe + "bias"], self.d_tv_n, (T * H, H), self.d_objvis, (R * H, H), self.d_ol, (R * H, H), Bt, T, R, S, H,
                      drop_p=p_h, seed=e.seed, tag=TAG_EMBED)
        # gradients of the two inputs (padded positions: zero rows, as the reference's masked scatter gives)
        ops.layernorm_bwd(self.d_tv_n, self.tv_in, self.st_tv, w32["vlbert.visual_ln_text.weight"], dx=self.d_tv_in,
                          dgamma=g32["vlbert.visual_ln_text.weight"], dbeta=g32["vlbert.visual_ln_text.bias"], workspace=e.ln_ws)
        ops.layernorm_bwd(self.d_objvis, self.ovl_in[:, :H], self.st_objvis, w32["vlbert.visual_ln_object.weight"],
                          dx=self.d_ovl_in[:, :H], dgamma=g32["vlbert.visual_ln_object.weight"],
                          dbeta=g32["vlbert.visual_ln_object.bias"], workspace=e.ln_ws)
        self.d_ovl_in[:, H:].copy_(self.d_ol)      # fp32 -> bf16 strided copy (glue: hands the gradient to autograd)


class Heads16:
    """Behind the encoder: the hand-over gathers (text / object rows of X[L]), the pooler and the relationship head, the MLM head (on
    the labelled rows only when the engine's batch state says so: eng.mlm_cap / eng._mlm_compact_now) and the MVRC head, the fused
    losses, the forward-only losses of eval_step and the backward of all of them down to d X[L].  with_heads=False (module API):
    hidden states out, d(hidden states) in; seq_out: the caller reads x_out and writes d X[L] into `dx` itself.

    The objective switches (pre-training engine only): with cfg.with_mlm_loss / with_mvrc_loss false that head is absent -- it owns no
    buffer and no W^T copy, launches nothing and leaves its loss, count and metric slots at zero; its rows of d(text_out) / d(obj_out)
    are never written and stay the zeros head_grad_combine reads.  With a norm switch the loss of that head is the reference's
    per-sample mean (resnet_vlbert_for_pretraining.py:168-174, 183-190; multitask :219-231, 252-259): per-sample weights
    (vlb_sample_norm_weights) and the row-weighted losses of csrc/loss.hip, on the full rows or on the rows mlm_compact listed."""

    def __init__(self, eng):
        self.eng = eng
        cfg, keep = eng.cfg, eng.keep_logits
        B, Bt, BT, BR, H, Vp, Cp = eng.B, eng.Bt, eng.BT, eng.BR, cfg.hidden_size, eng.Vp, eng.Cp
        zb, zf = _zeros(eng, ops.BF16), _zeros(eng, F32)
        self.with_heads, self.seq_out = eng.with_heads, eng.seq_out
        self.mlm, self.mvrc = cfg.with_mlm_loss, cfg.with_mvrc_loss
        self.mlm_norm, self.mvrc_norm = self.mlm and cfg.mlm_norm_in_batch_first, self.mvrc and cfg.mvrc_norm_in_batch_first
        self.wT = {}
        if self.mlm:
            self.wT[MLM_T], self.wT[WORD] = zb(H, H), zb(H, Vp)
            self.text_out = zb(BT, H)
            self.mlm_u, self.mlm_g, self.mlm_h, self.st_mlm = zb(BT, H), zb(BT, H), zb(BT, H), zf(BT, 2)
            self.mlm_logits = zb(BT, Vp)
            self.mlm_logits_copy = zb(BT, Vp) if keep else None
            self.d_mlm_h, self.d_mlm_g, self.d_mlm_u = zb(BT, H), zb(BT, H), zb(BT, H)
            if eng.mlm_cap is not None:      # MLM head compaction (DESIGN.md "MLM head"): the labelled rows, gathered into the first mlm_cap rows
                cap, d = eng.mlm_cap, eng.dev
                self.sel_pos = torch.full((cap,), -1, dtype=torch.int32, device=d)
                self.sel_src = torch.full((cap,), -1, dtype=torch.int32, device=d)
                self.labels_c = torch.full((cap,), -1, dtype=torch.int64, device=d)
                self.mlm_overflow = torch.zeros((1,), dtype=torch.int32, device=d)
                self.d_text_out_c = zb(cap, H)
            if self.mlm_norm:
                self.mlm_w = zf(Bt)                      # per-sample weights of the caption and the text-only samples
        if self.mvrc:
            self.wT[MVRC_T], self.wT[MVRC_C] = zb(H, H), zb(H, Cp)
            self.obj_out = zb(BR, H)
            self.mvrc_u, self.mvrc_g = zb(BR, H), zb(BR, H)
            self.mvrc_logits = zb(BR, Cp)
            self.mvrc_logits_copy = zb(BR, Cp) if keep else None
            self.mvrc_tsum = zf(BR)
            self.d_mvrc_u = zb(BR, H)
            if self.mvrc_norm:
                self.mvrc_w = zf(B)
        if cfg.with_pooler:
            self.wT[POOL] = zb(H, H)
            self.pooled, self.d_pooled, self.d_pool_pre = zb(B, H), zb(B, H), zb(B, H)
        if cfg.with_rel_loss:
            self.wT[REL] = zb(H, 64)                      # K padded to one 64-wide tile
            self.rel_logits = zb(B, 64)                   # 2 logits, row padded to 64 (pad columns stay zero)
            self.rel_logits_copy = zb(B, 64) if keep else None
        self.d_text_out, self.d_obj_out = zb(BT, H), zb(BR, H)      # what head_grad_combine reads, whichever heads exist
        self.xl, self.dx = eng.encoder.x_out, eng.encoder.dx_in

    def transposes(self):
        return [(self.eng.w16[n], t) for n, t in self.wT.items()]

    def refresh(self):
        pass

    def overwritten(self):
        """Parameters whose gradient is produced (whole tensor) by exactly one _wgrad call per backward; None without the heads
        (nothing overwrites their gradients)."""
        if not self.with_heads:
            return None
        names = ([WORD, MLM_T] if self.mlm else []) + ([MVRC_T, MVRC_C] if self.mvrc else [])
        if self.eng.cfg.with_rel_loss:
            names += [POOL, REL]
        return names

    def _mlm_rows(self):
        e = self.eng
        return (e.mlm_cap if e._mlm_compact_now else e.BT)          # rows the MLM head runs on

    def _mlm_weights(self):
        """Per-sample MLM weights from the labels in the input buffer; on the full-row path also the labelled-row totals into the count
        slots (mlm_compact has written them on the other)."""
        e = self.eng
        c = (None, None) if e._mlm_compact_now else (e.counts[0:1], e.counts[2:3] if e.Ba else None)
        ops.sample_norm_weights(self.mlm_w, e.T, labels=e.in_mlm_labels.view(-1), V=e.cfg.vocab_size, B_split=e.B, count0=c[0], count1=c[1])

    # -- forward ------------------------------------------------------------------------------------------------------
    def heads_fwd(self):
        e, cfg = self.eng, self.eng.cfg
        H, V, C, S, Bt = cfg.hidden_size, cfg.vocab_size, cfg.visual_region_classes, e.S, e.Bt
        w16, w32, xl = e.w16, e.w32, self.xl
        nr = self._mlm_rows()
        if self.mlm:
            if e._mlm_compact_now:
                ops.mlm_compact(e.in_mlm_labels.view(-1), e.lay["text_rows"].view(-1), e.B * e.T, V, self.sel_pos, self.sel_src,
                                self.labels_c, e.counts[0:1], e.counts[2:3], self.mlm_overflow)
                ops.gather_rows(xl, self.sel_src, self.text_out[:nr])
            else:
                ops.gather_rows(xl, e.lay["text_rows"].view(-1), self.text_out)
        if self.mvrc:
            ops.gather_rows(xl, e.lay["obj_rows"].view(-1)[:e.BR], self.obj_out)
        if cfg.with_pooler:       # BertPooler: tanh(dense(first token)) for the image-caption samples; A operand = strided view of X[L]
            x0 = xl.view(Bt, S * H)[:e.B, :H]
            ops.gemm_nt(x0, w16[POOL], self.pooled, bias=w32["vlbert.pooler.dense.bias"], act=ops.ACT_TANH)
        if not self.with_heads:
            return
        if cfg.with_rel_loss:     # relationsip_head: Linear(H -> 2) on the pooled output (common/visual_linguistic_bert.py:505-516)
            ops.gemm_nt(self.pooled, w16[REL], self.rel_logits[:, :2], bias=w32["vlbert.relationsip_head.caption_image_relationship.bias"])
        if self.mlm:
            pm = "vlbert.mlm_head.predictions."
            ops.gemm_nt(self.text_out[:nr], w16[MLM_T], self.mlm_g[:nr], bias=w32[pm + "transform.dense.bias"], act=ops.ACT_GELU_D,
                        pre=self.mlm_u[:nr])
            ops.layernorm_fwd(self.mlm_g[:nr], w32[pm + "transform.LayerNorm.weight"], w32[pm + "transform.LayerNorm.bias"],
                              self.mlm_h[:nr], self.st_mlm[:nr])
            ops.gemm_nt(self.mlm_h[:nr], w16[WORD], self.mlm_logits[:nr, :V], bias=w32[pm + "bias"])
        if self.mvrc:
            ops.gemm_nt(self.obj_out, w16[MVRC_T], self.mvrc_g, bias=w32["vlbert.mvrc_head.transform.dense.bias"], act=ops.ACT_GELU_D,
                        pre=self.mvrc_u)
            ops.gemm_nt(self.mvrc_g, w16[MVRC_C], self.mvrc_logits[:, :C], bias=w32["vlbert.mvrc_head.region_cls_pred.bias"])

    def outputs(self):
        """What engine.forward_core returns: views of the logits, the split hidden states, the pooled output, the relationship logits."""
        if not self.eng.cfg.default_objective:
            raise RuntimeError("the objective variants belong to the pre-training engine (no module-API outputs)")
        e, cfg = self.eng, self.eng.cfg
        V, C, H = cfg.vocab_size, cfg.visual_region_classes, cfg.hidden_size
        return (self.mlm_logits[:, :V].view(e.Bt, e.T, V), self.mvrc_logits[:, :C].view(e.B, e.R, C),
                self.text_out.view(e.Bt, e.T, H), self.obj_out.view(e.B, e.R, H),
                self.pooled if cfg.with_pooler else None, self.rel_logits[:, :2] if cfg.with_rel_loss else None)

    def losses(self, gscale, keep):
        """Loss values + d(logits) written in place over the logits.  Called again by the nn.Module mirror (keep=False:
        logits restored from the kept copies, loss slots untouched) when autograd hands down an upstream scale != 1."""
        e = self.eng
        B, T, Ba, V, C = e.B, e.T, e.Ba, e.cfg.vocab_size, e.cfg.visual_region_classes
        if keep:
            losses, mcopy, vcopy = e.losses, (self.mlm_logits_copy if self.mlm else None), (self.mvrc_logits_copy if self.mvrc else None)
        else:
            if self.mlm:
                self.mlm_logits.copy_(self.mlm_logits_copy)
            if self.mvrc:
                self.mvrc_logits.copy_(self.mvrc_logits_copy)
            losses, mcopy, vcopy = torch.zeros_like(e.losses), None, None
        nw = B * T     # rows of the image-caption samples; the aux rows follow and get their own mean (multitask.py:224-246)
        ds = e.scaler.scale if e.scaler is not None else None      # dynamic loss scale: multiplied into gscale on the device
        # train_metrics: the launches below become their ACC forms and add [hits, counted rows] to a row of train_metric_acc
        # (METRIC_ROWS) -- on the keep=True pass only, so that the mirror's re-run counts nothing twice
        tm = e.train_metric_acc if keep else None
        acc = (lambda *rows: dict(zip(("acc", "acc1"), (tm[r] for r in rows)))) if tm is not None else (lambda *rows: {})
        if self.mlm_norm:           # per-sample means: one weight per sample, the rows of both groups in one launch
            self._mlm_weights()
            two = dict(B_split=B, loss_out1=losses[2:3]) if Ba else {}
            if e._mlm_compact_now:
                ops.ce_rowweight_fwd_bwd(self.mlm_logits[:e.mlm_cap], V, self.labels_c, self.mlm_w, T, losses[0:1], sel_pos=self.sel_pos,
                                         gscale=gscale, dscale=ds, **two, **(acc(0, 1) if Ba else acc(0)))
            else:
                ops.ce_rowweight_fwd_bwd(self.mlm_logits, V, e.in_mlm_labels.view(-1), self.mlm_w, T, losses[0:1], gscale=gscale,
                                         logits_copy=mcopy, dscale=ds, **two, **(acc(0, 1) if Ba else acc(0)))
        elif self.mlm and e._mlm_compact_now:    # labelled rows only: caption rows first, then the aux rows, each group with its own mean
            ops.ce_fwd_bwd_compact(self.mlm_logits[:e.mlm_cap], V, self.labels_c, e.counts[0:1], e.counts[2:3], losses[0:1],
                                   losses[2:3], gscale=gscale, dscale=ds, **acc(0, 1))
        elif self.mlm:
            ops.ce_fwd_bwd(self.mlm_logits[:nw], V, e.in_mlm_labels.view(-1)[:nw], e.counts[0:1], losses[0:1], gscale=gscale,
                           logits_copy=mcopy[:nw] if mcopy is not None else None, dscale=ds, **acc(0))
            if Ba:
                ops.ce_fwd_bwd(self.mlm_logits[nw:], V, e.in_mlm_labels.view(-1)[nw:], e.counts[2:3], losses[2:3],
                               gscale=gscale, logits_copy=mcopy[nw:] if mcopy is not None else None, dscale=ds, **acc(1))
        if self.mvrc_norm:
            ops.soft_ce_rowweight_fwd_bwd(self.mvrc_logits, C, e.in_mvrc_labels.view(e.BR, C), self.mvrc_tsum, self.mvrc_w, e.R,
                                          e.counts[1:2], losses[1:2], gscale=gscale, logits_copy=vcopy, dscale=ds, **acc(2))
        elif self.mvrc:
            ops.soft_ce_fwd_bwd(self.mvrc_logits, C, e.in_mvrc_labels.view(e.BR, C), self.mvrc_tsum, e.counts[1:2],
                                losses[1:2], gscale=gscale, logits_copy=vcopy, dscale=ds, **acc(2))
        if e.cfg.with_rel_loss:     # F.cross_entropy(relationship_logits, relationship_label) (resnet_vlbert_for_pretraining.py:160-161)
            if not keep:
                self.rel_logits.copy_(self.rel_logits_copy)
            ops.ce_fwd_bwd(self.rel_logits, 2, e.in_rel_label, e.counts[3:4], losses[3:4], gscale=gscale,
                           logits_copy=self.rel_logits_copy if keep else None, dscale=ds, **acc(3))

    def eval_check(self):
        pass

    def eval_losses(self):
        """The forward-only kernels of csrc/metrics.hip in place of the fused forward+backward losses (engine.eval_step)."""
        e = self.eng
        B, T, Ba, V, C = e.B, e.T, e.Ba, e.cfg.vocab_size, e.cfg.visual_region_classes
        losses, acc, nw = e.losses, e.metric_acc, B * T
        if self.mlm_norm:
            self._mlm_weights()
            two = dict(B_split=B, loss_out1=losses[2:3], acc1=acc[1]) if Ba else {}
            if e._mlm_compact_now:
                ops.ce_rowweight_eval(self.mlm_logits[:e.mlm_cap], V, self.labels_c, self.mlm_w, T, losses[0:1], acc[0],
                                      sel_pos=self.sel_pos, **two)
            else:
                ops.ce_rowweight_eval(self.mlm_logits, V, e.in_mlm_labels.view(-1), self.mlm_w, T, losses[0:1], acc[0], **two)
        elif self.mlm and e._mlm_compact_now:    # labelled rows only: caption rows, then the aux rows (their counts came from mlm_compact)
            ops.ce_eval(self.mlm_logits[:e.mlm_cap], V, self.labels_c, losses[0:1], acc[0], count0=e.counts[0:1],
                        count1=e.counts[2:3], loss_out1=losses[2:3], acc1=acc[1])
        elif self.mlm:
            ops.ce_eval(self.mlm_logits[:nw], V, e.in_mlm_labels.view(-1)[:nw], losses[0:1], acc[0])
            if Ba:
                ops.ce_eval(self.mlm_logits[nw:], V, e.in_mlm_labels.view(-1)[nw:], losses[2:3], acc[1])
        if self.mvrc_norm:
            ops.soft_ce_rowweight_eval(self.mvrc_logits, C, e.in_mvrc_labels.view(e.BR, C), self.mvrc_tsum, self.mvrc_w, e.R,
                                       e.counts[1:2], losses[1:2], acc[2])
        elif self.mvrc:
            ops.soft_ce_eval(self.mvrc_logits, C, e.in_mvrc_labels.view(e.BR, C), losses[1:2], acc[2])
        if e.cfg.with_rel_loss:
            ops.ce_eval(self.rel_logits, 2, e.in_rel_label, losses[3:4], acc[3])

    # -- backward -----------------------------------------------------------------------------------------------------
    def heads_bwd(self):
        """d(logits) (or the caller's d(hidden states) / d X[L]) -> the heads' parameter gradients and d X[L] in `dx`, which is returned."""
        e, cfg = self.eng, self.eng.cfg
        H, V, C, T, R, S, Bt = cfg.hidden_size, cfg.vocab_size, cfg.visual_region_classes, e.T, e.R, e.S, e.Bt
        w32, g32, wT, dx = e.w32, e.g32, self.wT, self.dx
        if self.with_heads and self.mlm:
            pm = "vlbert.mlm_head.predictions."
            compact, nr = e._mlm_compact_now, self._mlm_rows()
            dlog = self.mlm_logits[:nr]                  # [rows, Vp], pad columns zero
            e._wgrad(dlog[:, :V], self.mlm_h[:nr], g32[WORD], g32[pm + "bias"])
            ops.gemm_nt_splitk(dlog, wT[WORD], self.d_mlm_h[:nr], workspace=e.wg_ws_main)
            e._ln_bwd(self.d_mlm_h[:nr], self.mlm_g[:nr], self.st_mlm[:nr], w32[pm + "transform.LayerNorm.weight"],
                      g32[pm + "transform.LayerNorm.weight"], g32[pm + "transform.LayerNorm.bias"], dx=self.d_mlm_g[:nr])
            ops.mul_bf16(self.d_mlm_g[:nr], self.mlm_u[:nr], self.d_mlm_u[:nr])
            e._wgrad(self.d_mlm_u[:nr], self.text_out[:nr], g32[MLM_T], g32[pm + "transform.dense.bias"])
            if compact:      # gradient of the labelled rows back to their text positions; every other position gets exactly zero
                ops.gemm_nt(self.d_mlm_u[:nr], wT[MLM_T], self.d_text_out_c)
                self.d_text_out.zero_()
                ops.scatter_rows(self.d_text_out_c, self.sel_pos, self.d_text_out)
            else:
                ops.gemm_nt(self.d_mlm_u, wT[MLM_T], self.d_text_out)
        if self.with_heads and self.mvrc:
            dlog2 = self.mvrc_logits                     # [BR, Cp]
            e._wgrad(dlog2[:, :C], self.mvrc_g, g32[MVRC_C], g32["vlbert.mvrc_head.region_cls_pred.bias"])
            ops.gemm_nt(dlog2, wT[MVRC_C], self.d_mvrc_u, act=ops.ACT_MULAUX, aux=self.mvrc_u)
            e._wgrad(self.d_mvrc_u, self.obj_out, g32[MVRC_T], g32["vlbert.mvrc_head.transform.dense.bias"])
            ops.gemm_nt(self.d_mvrc_u, wT[MVRC_T], self.d_obj_out)
        if self.with_heads and cfg.with_rel_loss:
            e._wgrad(self.rel_logits[:, :2], self.pooled, g32[REL], g32["vlbert.relationsip_head.caption_image_relationship.bias"])
            ops.gemm_nt(self.rel_logits, wT[REL], self.d_pooled)      # K = 64: two logits + zero padding
        if not self.seq_out:      # (sequence mode: the caller's d(sequence_output) is already in dx)
            ops.head_grad_combine(self.d_text_out, self.d_obj_out, e.lay["code"], dx, Bt, T, R, S, H)
        if cfg.with_pooler and (cfg.with_rel_loss or not self.with_heads):
            # d(pooled) came from the relationship head (or from the caller in hidden-state mode): through tanh and the
            # dense layer, then ADDED to the first-token rows of dX (gemm epilogue residual = its own output rows)
            ops.tanh_bwd(self.d_pooled, self.pooled, self.d_pool_pre)
            x0 = self.xl.view(Bt, S * H)[:e.B, :H]
            e._wgrad(self.d_pool_pre, x0, g32[POOL], g32["vlbert.pooler.dense.bias"])
            dx0 = dx.view(Bt, S * H)[:e.B, :H]
            ops.gemm_nt(self.d_pool_pre, wT[POOL], dx0, res=dx0)
        return dx
