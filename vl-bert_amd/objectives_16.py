"""The heads of the objective variants (16-bit): the part the engine puts behind the encoder when a pre-training objective switch is
off its default -- NETWORK.WITH_MLM_LOSS / WITH_MVRC_LOSS false (one head and its loss left out) or MLM_LOSS_NORM_IN_BATCH_FIRST /
MVRC_LOSS_NORM_IN_BATCH_FIRST true (per-sample loss means).  The default objective never gets here: it runs ends_16.Heads16 as before.

An absent head owns no buffer beyond the zero rows of d(text_out) / d(obj_out) that head_grad_combine reads, launches nothing, and leaves
its loss, count and metric slots at zero; the rows of d X[L] that only it would have fed are therefore exactly zero.  With a norm switch
the loss of that head is the reference's per-sample mean (resnet_vlbert_for_pretraining.py:168-174, 183-190; multitask :219-231,
252-259): per-sample weights (vlb_sample_norm_weights) and the row-weighted losses of csrc/loss.hip, on the full rows or on the rows
mlm_compact listed.
"""
import torch

from . import ops
from .ends_16 import Heads16, _zeros
from .engine import F32

MLM_T = "vlbert.mlm_head.predictions.transform.dense.weight"
WORD = "vlbert.word_embeddings.weight"
MVRC_T = "vlbert.mvrc_head.transform.dense.weight"
MVRC_C = "vlbert.mvrc_head.region_cls_pred.weight"
POOL = "vlbert.pooler.dense.weight"
REL = "vlbert.relationsip_head.caption_image_relationship.weight"


class ObjectiveHeads16(Heads16):
    def __init__(self, eng):
        self.eng = eng
        cfg, keep = eng.cfg, eng.keep_logits
        B, Bt, BT, BR, H, Vp, Cp = eng.B, eng.Bt, eng.BT, eng.BR, cfg.hidden_size, eng.Vp, eng.Cp
        zb, zf = _zeros(eng, ops.BF16), _zeros(eng, F32)
        self.with_heads, self.seq_out = True, False
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
            if eng.mlm_cap is not None:
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
            self.wT[REL] = zb(H, 64)
            self.rel_logits = zb(B, 64)
            self.rel_logits_copy = zb(B, 64) if keep else None
        # what head_grad_combine reads: the rows of an absent head are never written and stay the zeros they are here
        self.d_text_out, self.d_obj_out = zb(BT, H), zb(BR, H)
        self.xl, self.dx = eng.encoder.x_out, eng.encoder.dx_in

    def _names(self):
        names = ([MLM_T, WORD] if self.mlm else []) + ([MVRC_T, MVRC_C] if self.mvrc else [])
        return names + [n for n in (POOL, REL) if n in self.wT]

    def transposes(self):
        return [(self.eng.w16[n], self.wT[n]) for n in self._names()]

    def overwritten(self):
        names = ([WORD, MLM_T] if self.mlm else []) + ([MVRC_T, MVRC_C] if self.mvrc else [])
        if self.eng.cfg.with_rel_loss:
            names += [POOL, REL]
        return names

    # -- forward ------------------------------------------------------------------------------------------------------
    def heads_fwd(self):
        e, cfg = self.eng, self.eng.cfg
        H, V, C, S, Bt = cfg.hidden_size, cfg.vocab_size, cfg.visual_region_classes, e.S, e.Bt
        w16, w32, xl = e.w16, e.w32, self.xl
        if cfg.with_pooler:
            x0 = xl.view(Bt, S * H)[:e.B, :H]
            ops.gemm_nt(x0, w16[POOL], self.pooled, bias=w32["vlbert.pooler.dense.bias"], act=ops.ACT_TANH)
        if cfg.with_rel_loss:
            pr = "vlbert.relationsip_head.caption_image_relationship."
            ops.gemm_nt(self.pooled, w16[pr + "weight"], self.rel_logits[:, :2], bias=w32[pr + "bias"])
        if self.mlm:
            nr = self._mlm_rows()
            if e._mlm_compact_now:
                ops.mlm_compact(e.in_mlm_labels.view(-1), e.lay["text_rows"].view(-1), e.B * e.T, V, self.sel_pos, self.sel_src,
                                self.labels_c, e.counts[0:1], e.counts[2:3], self.mlm_overflow)
                ops.gather_rows(xl, self.sel_src, self.text_out[:nr])
            else:
                ops.gather_rows(xl, e.lay["text_rows"].view(-1), self.text_out)
            pm = "vlbert.mlm_head.predictions."
            ops.gemm_nt(self.text_out[:nr], w16[pm + "transform.dense.weight"], self.mlm_g[:nr], bias=w32[pm + "transform.dense.bias"],
                        act=ops.ACT_GELU_D, pre=self.mlm_u[:nr])
            ops.layernorm_fwd(self.mlm_g[:nr], w32[pm + "transform.LayerNorm.weight"], w32[pm + "transform.LayerNorm.bias"],
                              self.mlm_h[:nr], self.st_mlm[:nr])
            ops.gemm_nt(self.mlm_h[:nr], w16[WORD], self.mlm_logits[:nr, :V], bias=w32[pm + "bias"])
        if self.mvrc:
            ops.gather_rows(xl, e.lay["obj_rows"].view(-1)[:e.BR], self.obj_out)
            ops.gemm_nt(self.obj_out, w16[MVRC_T], self.mvrc_g, bias=w32["vlbert.mvrc_head.transform.dense.bias"], act=ops.ACT_GELU_D,
                        pre=self.mvrc_u)
            ops.gemm_nt(self.mvrc_g, w16[MVRC_C], self.mvrc_logits[:, :C], bias=w32["vlbert.mvrc_head.region_cls_pred.bias"])

    def outputs(self):
        raise RuntimeError("the objective variants belong to the pre-training engine (no module-API outputs)")

    def _mlm_weights(self):
        """Per-sample MLM weights from the labels in the input buffer; on the full-row path also the labelled-row totals into the count
        slots (mlm_compact has written them on the other)."""
        e = self.eng
        c = (None, None) if e._mlm_compact_now else (e.counts[0:1], e.counts[2:3] if e.Ba else None)
        ops.sample_norm_weights(self.mlm_w, e.T, labels=e.in_mlm_labels.view(-1), V=e.cfg.vocab_size, B_split=e.B, count0=c[0], count1=c[1])

    def losses(self, gscale, keep):
        e = self.eng
        B, T, Ba, V, C = e.B, e.T, e.Ba, e.cfg.vocab_size, e.cfg.visual_region_classes
        if keep:
            losses = e.losses
            mcopy, vcopy = (self.mlm_logits_copy if self.mlm else None), (self.mvrc_logits_copy if self.mvrc else None)
        else:
            if self.mlm:
                self.mlm_logits.copy_(self.mlm_logits_copy)
            if self.mvrc:
                self.mvrc_logits.copy_(self.mvrc_logits_copy)
            losses, mcopy, vcopy = torch.zeros_like(e.losses), None, None
        nw = B * T
        ds = e.scaler.scale if e.scaler is not None else None
        tm = e.train_metric_acc if keep else None
        acc = (lambda *rows: dict(zip(("acc", "acc1"), (tm[r] for r in rows)))) if tm is not None else (lambda *rows: {})
        if self.mlm and self.mlm_norm:
            self._mlm_weights()
            two = dict(B_split=B, loss_out1=losses[2:3]) if Ba else {}
            if e._mlm_compact_now:
                ops.ce_rowweight_fwd_bwd(self.mlm_logits[:e.mlm_cap], V, self.labels_c, self.mlm_w, T, losses[0:1], sel_pos=self.sel_pos,
                                         gscale=gscale, dscale=ds, **two, **(acc(0, 1) if Ba else acc(0)))
            else:
                ops.ce_rowweight_fwd_bwd(self.mlm_logits, V, e.in_mlm_labels.view(-1), self.mlm_w, T, losses[0:1], gscale=gscale,
                                         logits_copy=mcopy, dscale=ds, **two, **(acc(0, 1) if Ba else acc(0)))
        elif self.mlm:
            if e._mlm_compact_now:
                ops.ce_fwd_bwd_compact(self.mlm_logits[:e.mlm_cap], V, self.labels_c, e.counts[0:1], e.counts[2:3], losses[0:1],
                                       losses[2:3], gscale=gscale, dscale=ds, **acc(0, 1))
            else:
                ops.ce_fwd_bwd(self.mlm_logits[:nw], V, e.in_mlm_labels.view(-1)[:nw], e.counts[0:1], losses[0:1], gscale=gscale,
                               logits_copy=mcopy[:nw] if mcopy is not None else None, dscale=ds, **acc(0))
                if Ba:
                    ops.ce_fwd_bwd(self.mlm_logits[nw:], V, e.in_mlm_labels.view(-1)[nw:], e.counts[2:3], losses[2:3],
                                   gscale=gscale, logits_copy=mcopy[nw:] if mcopy is not None else None, dscale=ds, **acc(1))
        if self.mvrc and self.mvrc_norm:
            ops.soft_ce_rowweight_fwd_bwd(self.mvrc_logits, C, e.in_mvrc_labels.view(e.BR, C), self.mvrc_tsum, self.mvrc_w, e.R,
                                          e.counts[1:2], losses[1:2], gscale=gscale, logits_copy=vcopy, dscale=ds, **acc(2))
        elif self.mvrc:
            ops.soft_ce_fwd_bwd(self.mvrc_logits, C, e.in_mvrc_labels.view(e.BR, C), self.mvrc_tsum, e.counts[1:2],
                                losses[1:2], gscale=gscale, logits_copy=vcopy, dscale=ds, **acc(2))
        if e.cfg.with_rel_loss:
            if not keep:
                self.rel_logits.copy_(self.rel_logits_copy)
            ops.ce_fwd_bwd(self.rel_logits, 2, e.in_rel_label, e.counts[3:4], losses[3:4], gscale=gscale,
                           logits_copy=self.rel_logits_copy if keep else None, dscale=ds, **acc(3))

    def eval_losses(self):
        e = self.eng
        B, T, Ba, V, C = e.B, e.T, e.Ba, e.cfg.vocab_size, e.cfg.visual_region_classes
        losses, acc, nw = e.losses, e.metric_acc, B * T
        if self.mlm and self.mlm_norm:
            self._mlm_weights()
            two = dict(B_split=B, loss_out1=losses[2:3], acc1=acc[1]) if Ba else {}
            if e._mlm_compact_now:
                ops.ce_rowweight_eval(self.mlm_logits[:e.mlm_cap], V, self.labels_c, self.mlm_w, T, losses[0:1], acc[0],
                                      sel_pos=self.sel_pos, **two)
            else:
                ops.ce_rowweight_eval(self.mlm_logits, V, e.in_mlm_labels.view(-1), self.mlm_w, T, losses[0:1], acc[0], **two)
        elif self.mlm:
            if e._mlm_compact_now:
                ops.ce_eval(self.mlm_logits[:e.mlm_cap], V, self.labels_c, losses[0:1], acc[0], count0=e.counts[0:1],
                            count1=e.counts[2:3], loss_out1=losses[2:3], acc1=acc[1])
            else:
                ops.ce_eval(self.mlm_logits[:nw], V, e.in_mlm_labels.view(-1)[:nw], losses[0:1], acc[0])
                if Ba:
                    ops.ce_eval(self.mlm_logits[nw:], V, e.in_mlm_labels.view(-1)[nw:], losses[2:3], acc[1])
        if self.mvrc and self.mvrc_norm:
            ops.soft_ce_rowweight_eval(self.mvrc_logits, C, e.in_mvrc_labels.view(e.BR, C), self.mvrc_tsum, self.mvrc_w, e.R,
                                       e.counts[1:2], losses[1:2], acc[2])
        elif self.mvrc:
            ops.soft_ce_eval(self.mvrc_logits, C, e.in_mvrc_labels.view(e.BR, C), losses[1:2], acc[2])
        if e.cfg.with_rel_loss:
            ops.ce_eval(self.rel_logits, 2, e.in_rel_label, losses[3:4], acc[3])

    # -- backward -----------------------------------------------------------------------------------------------------
    def heads_bwd(self):
        e, cfg = self.eng, self.eng.cfg
        H, V, C, T, R, S, Bt = cfg.hidden_size, cfg.vocab_size, cfg.visual_region_classes, e.T, e.R, e.S, e.Bt
        w32, g32, wT, dx = e.w32, e.g32, self.wT, self.dx
        if self.mlm:
            pm = "vlbert.mlm_head.predictions."
            compact, nr = e._mlm_compact_now, self._mlm_rows()
            dlog = self.mlm_logits[:nr]
            e._wgrad(dlog[:, :V], self.mlm_h[:nr], g32[WORD], g32[pm + "bias"])
            ops.gemm_nt_splitk(dlog, wT[WORD], self.d_mlm_h[:nr], workspace=e.wg_ws_main)
            e._ln_bwd(self.d_mlm_h[:nr], self.mlm_g[:nr], self.st_mlm[:nr], w32[pm + "transform.LayerNorm.weight"],
                      g32[pm + "transform.LayerNorm.weight"], g32[pm + "transform.LayerNorm.bias"], dx=self.d_mlm_g[:nr])
            ops.mul_bf16(self.d_mlm_g[:nr], self.mlm_u[:nr], self.d_mlm_u[:nr])
            e._wgrad(self.d_mlm_u[:nr], self.text_out[:nr], g32[pm + "transform.dense.weight"], g32[pm + "transform.dense.bias"])
            if compact:
                ops.gemm_nt(self.d_mlm_u[:nr], wT[MLM_T], self.d_text_out_c)
                self.d_text_out.zero_()
                ops.scatter_rows(self.d_text_out_c, self.sel_pos, self.d_text_out)
            else:
                ops.gemm_nt(self.d_mlm_u, wT[MLM_T], self.d_text_out)
        if self.mvrc:
            dlog2 = self.mvrc_logits
            e._wgrad(dlog2[:, :C], self.mvrc_g, g32[MVRC_C], g32["vlbert.mvrc_head.region_cls_pred.bias"])
            ops.gemm_nt(dlog2, wT[MVRC_C], self.d_mvrc_u, act=ops.ACT_MULAUX, aux=self.mvrc_u)
            e._wgrad(self.d_mvrc_u, self.obj_out, g32[MVRC_T], g32["vlbert.mvrc_head.transform.dense.bias"])
            ops.gemm_nt(self.d_mvrc_u, wT[MVRC_T], self.d_obj_out)
        if cfg.with_rel_loss:
            pr = "vlbert.relationsip_head.caption_image_relationship."
            e._wgrad(self.rel_logits[:, :2], self.pooled, g32[pr + "weight"], g32[pr + "bias"])
            ops.gemm_nt(self.rel_logits, wT[pr + "weight"], self.d_pooled)
        ops.head_grad_combine(self.d_text_out, self.d_obj_out, e.lay["code"], dx, Bt, T, R, S, H)
        if cfg.with_pooler and cfg.with_rel_loss:
            ops.tanh_bwd(self.d_pooled, self.pooled, self.d_pool_pre)
            x0 = self.xl.view(Bt, S * H)[:e.B, :H]
            e._wgrad(self.d_pool_pre, x0, g32[POOL], g32["vlbert.pooler.dense.bias"])
            dx0 = dx.view(Bt, S * H)[:e.B, :H]
            ops.gemm_nt(self.d_pool_pre, wT[POOL], dx0, res=dx0)
        return dx
