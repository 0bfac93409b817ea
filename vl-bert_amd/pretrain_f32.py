"""fp32 front end, heads and losses of the pre-training step (`PretrainEngine(..., encoder_fp32=True, fp32_full=True)`): with the fp32
encoder (encoder_f32.py) no 16-bit tensor lies between the engine's input buffers and its two loss values, and none between the losses
and the flat fp32 gradient -- the reference's `TRAIN.FP16: false` pre-training (cfgs/pretrain/base_prec_withouttextonly_4x16G_fp32.yaml).

Replaces, in fp32: common/fast_rcnn.py:165-186 (coordinate embedding || feature -> Dropout -> Linear -> ReLU, with the
object_mask_visual_embedding substitution of resnet_vlbert_for_pretraining.py:114-117), common/visual_linguistic_bert.py:173-241 (visual
LayerNorms + embedding), :146-166 (text / object split), the MLM and MVRC heads (modeling.py:439-472, visual_linguistic_bert.py:519-531),
F.cross_entropy / soft_cross_entropy (common/utils/misc.py:124-151) and the backward of all of them.

Kernels: csrc/f32_pretrain.hip (mask substitution, masked column sums, table rows and their gradient, row gathers, the three losses),
csrc/f32_ends.hip (coordinate embedding, fused embedding, ReLU backward, x GELU') and the split-operand GEMMs / LayerNorm of
csrc/f32_path.hip on the fp32 MASTER weights.  The fused embedding is called in its dense form: the per-sample text_vis row is a
stride-0 operand, the objects' linguistic rows are materialised from the 2-row table (vlb_select_rows2_f32, B*R*H floats), and the
backward's per-token d text_vis / per-object d obj_ling are reduced by vlb_group_rowsum_f32 / vlb_table2_grad_f32 in a fixed order.
Weight gradients are row-reduction ("TN") products straight from the row-major tensors, accumulated by a plain read-modify-write (one K
slice), bias gradients their column sums.  The tied decoder and the region classifier (30522 / 1601 rows: no multiple of 4) multiply by
exact zero-padded fp32 copies of the master weight, refreshed -- with the transposed copies the data gradients read -- whenever the
engine refreshes its weight copies (load, every optimizer step).
"""
import torch

from . import ops
from .engine import F32, TAG_DOWNSAMPLE, TAG_EMBED, VIS_DIM
from .ends_16 import PRETRAIN_FRONT_GRADS


class PretrainF32:
    """Serves as the engine's front AND back: front_fwd / front_bwd around the fp32 encoder's X[0], heads_fwd / losses / heads_bwd
    around its X[L]."""

    def __init__(self, eng):
        self.eng = eng
        cfg, d = eng.cfg, eng.dev
        H, V, C = cfg.hidden_size, cfg.vocab_size, cfg.visual_region_classes
        B, T, R = eng.B, eng.T, eng.R
        BT, BR, M, Vp, Cp = eng.BT, eng.BR, eng.M, eng.Vp, eng.Cp
        z = lambda *s: torch.zeros(s, dtype=F32, device=d)
        # front end
        self.a_ds, self.obj_reps, self.objvis, self.textvis = z(BR, 2 * VIS_DIM), z(BR, H), z(BR, H), z(B, H)
        self.obj_ling, self.emb_pre = z(BR, H), z(M, H)
        self.st_objvis, self.st_textvis, self.st_emb = z(BR, 2), z(B, 2), z(M, 2)
        # heads
        self.text_out, self.mlm_g, self.mlm_dg, self.mlm_h, self.st_mlm = z(BT, H), z(BT, H), z(BT, H), z(BT, H), z(BT, 2)
        self.obj_out, self.mvrc_g, self.mvrc_dg = z(BR, H), z(BR, H), z(BR, H)
        self.mlm_logits, self.mvrc_logits, self.mvrc_tsum = z(BT, Vp), z(BR, Cp), z(BR)
        self.mlm_logits_copy = z(BT, Vp) if eng.keep_logits else None
        self.mvrc_logits_copy = z(BR, Cp) if eng.keep_logits else None
        self.row_loss = z(max(BT, BR, 1))
        if eng.mlm_cap is not None:      # MLM head compaction (DESIGN.md "MLM head"): the labelled rows, gathered into the first mlm_cap rows
            cap = eng.mlm_cap
            self.sel_pos = torch.full((cap,), -1, dtype=torch.int32, device=d)
            self.sel_src = torch.full((cap,), -1, dtype=torch.int32, device=d)
            self.labels_c = torch.full((cap,), -1, dtype=torch.int64, device=d)
            self.mlm_overflow = torch.zeros((1,), dtype=torch.int32, device=d)
        # backward
        self.d_mlm_h, self.d_mlm_g, self.d_mlm_u, self.d_text_out = z(BT, H), z(BT, H), z(BT, H), z(BT, H)
        self.d_text_out_c = z(eng.mlm_cap, H) if eng.mlm_cap is not None else None
        self.d_mvrc_u, self.d_obj_out = z(BR, H), z(BR, H)
        self.dX = z(M, H)
        # The decoder's data gradient reduces over the vocabulary (K = 30528) into few output tiles (96 at 1024 labelled rows): K is cut
        # into dec_split slices that run as the batch dimension of one launch, each writing its own slab -- slab i of row r is row
        # r * dec_split + i of dec_slabs -- and vlb_group_rowsum_f32 adds a row's slabs in order (the single launch took 870 us on 96
        # workgroups at the headline size; the step went from 29.28 to 28.81 ms) -- no atomics: the sum keeps a fixed order
        self.dec_split = next(n for n in (8, 6, 4, 3, 2, 1) if (Vp // 32) % n == 0)
        self.dec_slabs = z(BT * self.dec_split, H)
        self.d_tv_tok, self.d_textvis, self.d_reps0 = z(BT, H), z(B, H), z(B, H)
        self.d_objvis, self.d_obj_ling, self.d_obj_reps, self.d_yds = z(BR, H), z(BR, H), z(BR, H), z(BR, H)
        self.d_afeat = z(BR, VIS_DIM)
        # weight copies: zero-padded (rows up to Vp / Cp) and transposed
        self.Wdec, self.bdec, self.WdecT = z(Vp, H), z(Vp), z(H, Vp)
        self.Wcls, self.bcls, self.WclsT = z(Cp, H), z(Cp), z(H, Cp)
        self.WmT, self.WvT, self.WdsT = z(H, H), z(H, H), z(VIS_DIM, H)
        P = eng.P
        self.ling_table = P.view(P.master, "object_linguistic_embeddings.weight", (2, H), span=2)
        self.g_ling_table = P.view(P.grad, "object_linguistic_embeddings.weight", (2, H), span=2)
        self.x0, self.xl = eng.encoder.x_in, eng.encoder.x_out

    def transposes(self):
        return []        # no 16-bit weight copy: refresh() pads / transposes the fp32 master

    def overwritten(self):
        return None      # every weight gradient is ACCUMULATED (read-modify-write)

    def grads(self):
        return [self.eng.g32[n] for n in PRETRAIN_FRONT_GRADS if n in self.eng.g32]

    def refresh(self):
        """Padded / transposed fp32 copies of the current master weights (exact: data movement only)."""
        e = self.eng
        H, V, C = e.cfg.hidden_size, e.cfg.vocab_size, e.cfg.visual_region_classes
        w = e.w32
        word, cls = w["vlbert.word_embeddings.weight"], w["vlbert.mvrc_head.region_cls_pred.weight"]
        self.Wdec[:V].copy_(word)
        self.bdec[:V].copy_(w["vlbert.mlm_head.predictions.bias"])
        self.Wcls[:C].copy_(cls)
        self.bcls[:C].copy_(w["vlbert.mvrc_head.region_cls_pred.bias"])
        ops.transpose_f32(word, H, self.WdecT, e.Vp, V, H, e.Vp)
        ops.transpose_f32(cls, H, self.WclsT, e.Cp, C, H, e.Cp)
        ops.transpose_f32(w["vlbert.mlm_head.predictions.transform.dense.weight"], H, self.WmT, H, H, H, H)
        ops.transpose_f32(w["vlbert.mvrc_head.transform.dense.weight"], H, self.WvT, H, H, H, H)
        # the feature half of obj_downsample: W[:, 2048:] -> [2048, H]
        ops.transpose_f32((w["image_feature_extractor.obj_downsample.1.weight"], VIS_DIM), 2 * VIS_DIM, self.WdsT, H, H, VIS_DIM, H)

    # -- forward ------------------------------------------------------------------------------------------------------
    def front_fwd(self, p_h, p_ds):
        """Input buffers -> the fp32 encoder's X[0]."""
        e = self.eng
        B, T, R, S, H = e.B, e.T, e.R, e.S, e.cfg.hidden_size
        w, seed = e.w32, e.seed
        ops.obj_prep_f32_fwd(e.in_boxes, e.in_im_info, self.a_ds, drop_p=p_ds, seed=seed, tag=TAG_DOWNSAMPLE)
        ops.mask_feature_f32(self.a_ds, e.in_boxes, e.in_mvrc_ops.view(-1), w["object_mask_visual_embedding.weight"].view(-1), drop_p=p_ds,
                             seed=seed, tag=TAG_DOWNSAMPLE)
        pd = "image_feature_extractor.obj_downsample.1."
        ops.gemm_nt_f32(self.a_ds, 2 * VIS_DIM, w[pd + "weight"], 2 * VIS_DIM, self.obj_reps, H, e.BR, H, 2 * VIS_DIM, bias=w[pd + "bias"], epi=2)
        ops.zero_padded_rows_f32(self.obj_reps, e.in_boxes)      # pad_sequence zeros (a padded box 0 feeds the text tokens' visual embedding)
        ops.layernorm_f32_fwd(self.obj_reps, w["vlbert.visual_ln_object.weight"], w["vlbert.visual_ln_object.bias"], self.objvis, self.st_objvis)
        reps0 = self.obj_reps.view(B, R * H)[:, :H]              # obj_reps[:, 0] (text tags are all 0)
        ops.layernorm_f32_fwd(reps0, w["vlbert.visual_ln_text.weight"], w["vlbert.visual_ln_text.bias"], self.textvis, self.st_textvis)
        ops.select_rows2_f32(self.ling_table, e.in_mvrc_ops.view(-1), self.obj_ling)
        ops.embed_f32_fwd(e.lay, e.in_text, None, w["vlbert.word_embeddings.weight"], w["vlbert.position_embeddings.weight"],
                          w["vlbert.token_type_embeddings.weight"], w["vlbert.end_embedding.weight"], self.textvis, (H, 0), self.objvis,
                          (R * H, H), self.obj_ling, (R * H, H), None, w["vlbert.embedding_LayerNorm.weight"],
                          w["vlbert.embedding_LayerNorm.bias"], self.emb_pre, self.st_emb, self.x0, B, T, R, S, H, drop_p=p_h, seed=seed,
                          tag=TAG_EMBED)

    def _mlm_rows(self):
        e = self.eng
        compact = bool(e._mlm_compact_now)
        return compact, (e.mlm_cap if compact else e.BT)

    def heads_fwd(self):
        """The fp32 encoder's X[L] -> the two logits tensors."""
        e = self.eng
        H, V = e.cfg.hidden_size, e.cfg.vocab_size
        w, xl = e.w32, self.xl
        compact, nr = self._mlm_rows()
        if compact:
            ops.mlm_compact(e.in_mlm_labels.view(-1), e.lay["text_rows"].view(-1), e.B * e.T, V, self.sel_pos, self.sel_src, self.labels_c,
                            e.counts[0:1], e.counts[2:3], self.mlm_overflow)
            ops.gather_rows_f32(xl, self.sel_src, self.text_out[:nr])
        else:
            ops.gather_rows_f32(xl, e.lay["text_rows"].view(-1), self.text_out)
        ops.gather_rows_f32(xl, e.lay["obj_rows"].view(-1)[:e.BR], self.obj_out)
        pm = "vlbert.mlm_head.predictions."
        ops.gemm_nt_f32(self.text_out, H, w[pm + "transform.dense.weight"], H, self.mlm_g, H, nr, H, H, bias=w[pm + "transform.dense.bias"],
                        epi=1, pre=self.mlm_dg, ldpre=H)
        ops.layernorm_f32_fwd(self.mlm_g[:nr], w[pm + "transform.LayerNorm.weight"], w[pm + "transform.LayerNorm.bias"], self.mlm_h[:nr],
                              self.st_mlm[:nr])
        ops.gemm_nt_f32(self.mlm_h, H, self.Wdec, H, self.mlm_logits, e.Vp, nr, e.Vp, H, bias=self.bdec)
        pv = "vlbert.mvrc_head."
        ops.gemm_nt_f32(self.obj_out, H, w[pv + "transform.dense.weight"], H, self.mvrc_g, H, e.BR, H, H, bias=w[pv + "transform.dense.bias"],
                        epi=1, pre=self.mvrc_dg, ldpre=H)
        ops.gemm_nt_f32(self.mvrc_g, H, self.Wcls, H, self.mvrc_logits, e.Cp, e.BR, e.Cp, H, bias=self.bcls)

    def losses(self, gscale, keep):
        """Loss values + d(logits) in place over the fp32 logits (ends_16.Heads16.losses, its keep=False re-run included)."""
        e = self.eng
        V, C = e.cfg.vocab_size, e.cfg.visual_region_classes
        if keep:
            losses, mcopy, vcopy = e.losses, self.mlm_logits_copy, self.mvrc_logits_copy
        else:
            self.mlm_logits.copy_(self.mlm_logits_copy)
            self.mvrc_logits.copy_(self.mvrc_logits_copy)
            losses, mcopy, vcopy = torch.zeros_like(e.losses), None, None
        compact, nr = self._mlm_rows()
        # train_metrics: the ACC forms add [hits, counted rows] to rows 0 (MLM; row 1 takes the empty second group) and 2 (MVRC) of
        # train_metric_acc, on the keep=True pass only (as Heads16.losses)
        tm = e.train_metric_acc if keep else None
        acc = (lambda *rows: dict(zip(("acc", "acc1"), (tm[r] for r in rows)))) if tm is not None else (lambda *rows: {})
        if compact:
            ops.ce_f32_fwd_bwd_compact(self.mlm_logits[:nr], V, self.labels_c, e.counts[0:1], e.counts[2:3], losses[0:1], losses[2:3], gscale=gscale,
                                       row_loss=self.row_loss, **acc(0, 1))
        else:
            ops.ce_f32_fwd_bwd(self.mlm_logits, V, e.in_mlm_labels.view(-1), e.counts[0:1], losses[0:1], gscale=gscale, logits_copy=mcopy,
                               row_loss=self.row_loss, **acc(0))
        ops.soft_ce_f32_fwd_bwd(self.mvrc_logits, C, e.in_mvrc_labels.view(e.BR, C), self.mvrc_tsum, e.counts[1:2], losses[1:2], gscale=gscale,
                                logits_copy=vcopy, row_loss=self.row_loss, **acc(2))

    def eval_check(self):
        raise ValueError("eval_step: not built for an fp32_full engine (the validation kernels of csrc/metrics.hip read 16-bit logits); "
                         "validate on an engine without fp32_full")

    # -- backward -----------------------------------------------------------------------------------------------------
    def heads_bwd(self):
        """d(logits) -> parameter gradients of the heads (accumulated) and the fp32 d X[L], which is returned."""
        e = self.eng
        H, V, C = e.cfg.hidden_size, e.cfg.vocab_size, e.cfg.visual_region_classes
        w, g = e.w32, e.g32
        compact, nr = self._mlm_rows()
        pm = "vlbert.mlm_head.predictions."
        dlog = self.mlm_logits      # [rows, Vp], pad columns zero
        ops.gemm_tn_f32(dlog, e.Vp, self.mlm_h, H, g["vlbert.word_embeddings.weight"], H, nr, V, H, atomic=True, colsum=g[pm + "bias"])
        nb, kc = self.dec_split, e.Vp // self.dec_split
        ops.gemm_nt_f32(dlog, e.Vp, self.WdecT, e.Vp, self.dec_slabs, nb * H, nr, H, kc, batch=(nb, 1), sA=(kc, 0), sB=(kc, 0), sC=(H, 0))
        ops.group_rowsum_f32(self.dec_slabs[:nr * nb], nb, self.d_mlm_h[:nr])
        ops.layernorm_f32_bwd(self.d_mlm_h[:nr], self.mlm_g[:nr], self.st_mlm[:nr], w[pm + "transform.LayerNorm.weight"], dx=self.d_mlm_g[:nr],
                              dgamma=g[pm + "transform.LayerNorm.weight"], dbeta=g[pm + "transform.LayerNorm.bias"])
        ops.mul_f32(self.d_mlm_g[:nr], self.mlm_dg[:nr], self.d_mlm_u[:nr])
        ops.gemm_tn_f32(self.d_mlm_u, H, self.text_out, H, g[pm + "transform.dense.weight"], H, nr, H, H, atomic=True,
                        colsum=g[pm + "transform.dense.bias"])
        if compact:      # gradient of the labelled rows back to their text positions; every other position gets exactly zero
            ops.gemm_nt_f32(self.d_mlm_u, H, self.WmT, H, self.d_text_out_c, H, nr, H, H)
            self.d_text_out.zero_()
            ops.scatter_rows_f32(self.d_text_out_c, self.sel_pos, self.d_text_out)
        else:
            ops.gemm_nt_f32(self.d_mlm_u, H, self.WmT, H, self.d_text_out, H, nr, H, H)
        pv = "vlbert.mvrc_head."
        dlog2 = self.mvrc_logits    # [BR, Cp]
        ops.gemm_tn_f32(dlog2, e.Cp, self.mvrc_g, H, g[pv + "region_cls_pred.weight"], H, e.BR, C, H, atomic=True,
                        colsum=g[pv + "region_cls_pred.bias"])
        ops.gemm_nt_f32(dlog2, e.Cp, self.WclsT, e.Cp, self.d_mvrc_u, H, e.BR, H, e.Cp, epi=3, aux=self.mvrc_dg, ldaux=H)
        ops.gemm_tn_f32(self.d_mvrc_u, H, self.obj_out, H, g[pv + "transform.dense.weight"], H, e.BR, H, H, atomic=True,
                        colsum=g[pv + "transform.dense.bias"])
        ops.gemm_nt_f32(self.d_mvrc_u, H, self.WvT, H, self.d_obj_out, H, e.BR, H, H)
        ops.head_grad_combine_f32(self.d_text_out, self.d_obj_out, e.lay["code"], self.dX, e.Bt, e.T, e.R, e.S, H)
        return self.dX

    def front_bwd(self, dx, p_h, p_ds, on_layer_done=None):
        """The fp32 d X[0] -> gradients of the embedding tables, the visual LayerNorms, obj_downsample and the mask embedding."""
        e = self.eng
        B, T, R, S, H = e.B, e.T, e.R, e.S, e.cfg.hidden_size
        w, g, seed = e.w32, e.g32, e.seed
        self.d_tv_tok.zero_()
        self.d_objvis.zero_()
        self.d_obj_ling.zero_()
        pe = "vlbert.embedding_LayerNorm."
        ops.embed_f32_bwd(dx, self.emb_pre, self.st_emb, w[pe + "weight"], e.lay, e.in_text, None, None, g["vlbert.word_embeddings.weight"],
                          g["vlbert.position_embeddings.weight"], g["vlbert.token_type_embeddings.weight"], g["vlbert.end_embedding.weight"],
                          g[pe + "weight"], g[pe + "bias"], self.d_tv_tok, (T * H, H), self.d_objvis, (R * H, H), self.d_obj_ling, (R * H, H),
                          B, T, R, S, H, drop_p=p_h, seed=seed, tag=TAG_EMBED)
        ops.group_rowsum_f32(self.d_tv_tok, T, self.d_textvis)                                   # d text_vis summed over a sample's tokens
        ops.table2_grad_f32(self.d_obj_ling, e.in_mvrc_ops.view(-1), self.g_ling_table)
        if on_layer_done:      # the tied word-embedding gradient (decoder weight gradient + this scatter-add) is complete
            on_layer_done("word_emb")
        ops.layernorm_f32_bwd(self.d_objvis, self.obj_reps, self.st_objvis, w["vlbert.visual_ln_object.weight"], dx=self.d_obj_reps,
                              dgamma=g["vlbert.visual_ln_object.weight"], dbeta=g["vlbert.visual_ln_object.bias"])
        reps0 = self.obj_reps.view(B, R * H)[:, :H]
        ops.layernorm_f32_bwd(self.d_textvis, reps0, self.st_textvis, w["vlbert.visual_ln_text.weight"], dx=self.d_reps0,
                              dgamma=g["vlbert.visual_ln_text.weight"], dbeta=g["vlbert.visual_ln_text.bias"])
        ops.add_rows_f32(self.d_obj_reps.view(B, R * H)[:, :H], self.d_reps0)
        ops.relu_bwd_f32(self.d_obj_reps, self.obj_reps, self.d_yds)
        pd = "image_feature_extractor.obj_downsample.1."
        ops.gemm_tn_f32(self.d_yds, H, self.a_ds, 2 * VIS_DIM, g[pd + "weight"], 2 * VIS_DIM, e.BR, H, 2 * VIS_DIM, atomic=True,
                        colsum=g[pd + "bias"])
        # gradient of the mask embedding: feature half of dA = dY W, masked regions only, through their dropout
        ops.gemm_nt_f32(self.d_yds, H, self.WdsT, H, self.d_afeat, VIS_DIM, e.BR, VIS_DIM, H)
        ops.masked_colsum_f32(self.d_afeat, e.in_mvrc_ops.view(-1), g["object_mask_visual_embedding.weight"].view(-1), drop_p=p_ds, seed=seed,
                              tag=TAG_DOWNSAMPLE, row_elems=2 * VIS_DIM, col_off=VIS_DIM)
