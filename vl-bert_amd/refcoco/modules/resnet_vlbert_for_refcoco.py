"""Drop-in `ResNetVLBERT` for RefCOCO+ fine-tuning (refcoco/modules/resnet_vlbert_for_refcoco.py:13-227) on the HIP library: same
constructor argument (the config tree of refcoco/function/config.py), same `train_forward(image, boxes, im_info, expression, label) ->
(outputs, loss)` and `inference_forward(image, boxes, im_info, expression) -> outputs`, same parameter names
(`image_feature_extractor.*`, `object_linguistic_embeddings.weight`, `vlbert.*`, `final_mlp.0.dense.*`, `final_mlp.2.*`), so the
reference's trainer and checkpoints work unchanged.

Composition, as in the reference:  boxes trimmed to the batch's longest valid run (:80-86) -> FastRCNN mirror (precomputed features or
images) -> text = [CLS] expression [SEP], token types 0, every token sees obj_reps[:, 0] (:97-107, index plumbing in torch) ->
VisualLinguisticBert mirror with the text and object outputs separated (:118-125; its object output is zero at padded boxes, as
the reference's) -> `final_mlp` on every object row -> masked BCE (:132-135).  The head and the loss are ONE autograd node on the
library: the transform on the bf16 GEMM with the fused GELU epilogue (gelu' kept), then csrc/grounding.hip -- the Linear(H, 1) score
as a row dot product with the classifier dropout applied on the fly, the masked BCE with its gradient, the score backward, and the
inference box pick.  No host synchronisation inside the node.
Unsupported (NotImplementedError, as in the VQA mirror): BLIND, NO_GROUNDING, ENABLE_CNN_REG_LOSS, object_word_embed_mode != 2.
"""
import torch
import torch.nn as nn

from ... import ops
from ...common.heads import Linear16, cfg_get
from ...common.module import Module

F32 = torch.float32
CLS, SEP = 101, 102          # ids of '[CLS]', '[SEP]' in the BERT vocabularies (tokenizer lookups in the reference, :96)
_TAG = 2003                  # dropout site of final_mlp.1


class _HeadFn(torch.autograd.Function):
    """hs [B, max_len, H] fp32 -> (label_logits [B, origin_len] fp32, loss): final_mlp + masked BCE on the device, hand-scheduled
    backward.  boxes [B, origin_len, >=4] fp32 gives the box mask and origin_len; label None = inference (no loss)."""

    @staticmethod
    def forward(ctx, hs, boxes, label, module, train, w1, b1, w2, b2):
        B, R, H = hs.shape
        st = module._head_state(B * R, hs.device)
        module._w1.sync()
        p = module.cls_drop if train else 0.0
        ops.cast_f32_bf16(hs.detach().contiguous(), st["x"])
        ops.gemm_nt(st["x"], module._w1.W, st["g"], bias=b1.detach(), act=ops.ACT_GELU_D, pre=st["dg"])
        logits = torch.empty((B, boxes.shape[1]), dtype=F32, device=hs.device)
        ops.ground_score_fwd(st["g"], w2.detach().view(-1), b2.detach(), logits, B, R, drop_p=p, seed=module._seed, tag=_TAG)
        loss = torch.empty((), dtype=F32, device=hs.device)
        if label is not None:
            ops.ground_bce(logits, boxes, label, R, loss, st["dlogit"])
        else:
            loss.zero_()
        ctx.module, ctx.st, ctx.p, ctx.shape = module, st, p, (B, R, H)
        ctx.mark_non_differentiable(logits)
        return logits, loss

    @staticmethod
    def backward(ctx, _g_logits, g_loss):
        module, st, p = ctx.module, ctx.st, ctx.p
        B, R, H = ctx.shape
        w1, b1, w2, b2 = module._head_params()
        gw1, gb1 = torch.zeros_like(w1, dtype=F32), torch.zeros_like(b1, dtype=F32)
        gw2, gb2 = torch.empty_like(w2, dtype=F32), torch.empty_like(b2, dtype=F32)
        gl = g_loss.detach().to(F32).reshape(1).contiguous()           # upstream scale read on the device (no float(g_loss))
        ops.ground_score_bwd(gl, st["dlogit"], st["g"], st["dg"], w2.detach().view(-1), st["du"], gw2.view(-1), gb2, drop_p=p,
                             seed=module._seed, tag=_TAG)
        ops.wgrad_tn(st["du"], st["x"], gw1, colsum=gb1, workspace=None)
        ops.gemm_nt(st["du"], module._w1.Wt, st["dx"])
        d_hs = torch.empty((B * R, H), dtype=F32, device=gl.device)
        ops.cast_bf16_f32(st["dx"], d_hs)
        if p > 0:
            ops.rng_advance(module._seed)
        return d_hs.view(B, R, H), None, None, None, None, gw1, gb1, gw2, gb2


class ResNetVLBERT(Module):
    SEED = 40013

    def _check_config(self, net, vl):
        if cfg_get(net, "BLIND", False) or cfg_get(net, "NO_GROUNDING", False) or cfg_get(net, "ENABLE_CNN_REG_LOSS", False):
            raise NotImplementedError("BLIND / NO_GROUNDING / ENABLE_CNN_REG_LOSS are not supported")
        if cfg_get(vl, "object_word_embed_mode", 2) != 2:
            raise NotImplementedError("object_word_embed_mode must be 2 (one shared object word embedding)")

    def _build_heads(self, net, vl):
        if self.H % 64:
            raise NotImplementedError("hidden_size must be a multiple of 64 (GEMM tile width)")
        self.initializer_range = float(cfg_get(vl, "initializer_range", 0.02))
        mlp = nn.Module()                      # Sequential(VisualLinguisticBertMVRCHeadTransform, Dropout, Linear(H, 1))  (:41-47)
        mlp.add_module("0", self._transform())
        mlp.add_module("2", self._lin(1, self.H))
        self.final_mlp = mlp
        self._w1 = Linear16(getattr(mlp, "0").dense)          # the transform's dense weight; the Linear(H, 1) runs in csrc/grounding.hip
        self._states = {}

    # -- parameters ---------------------------------------------------------------------------------
    def _head_params(self):
        t, b = getattr(self.final_mlp, "0"), getattr(self.final_mlp, "2")
        return [t.dense.weight, t.dense.bias, b.weight, b.bias]

    def init_weight(self):
        """:52-61: xavier-uniform Linears with zero biases, N(0, initializer_range) object word embedding."""
        with torch.no_grad():
            self.image_feature_extractor.init_weight()
            self.object_linguistic_embeddings.weight.normal_(0.0, self.initializer_range)
            for q in self._head_params():
                if q.dim() == 2:
                    nn.init.xavier_uniform_(q)
                else:
                    q.zero_()

    def _head_state(self, n, dev):
        if n not in self._states:
            zb = lambda *s: torch.zeros(s, dtype=ops.BF16, device=dev)
            H = self.H
            self._states[n] = dict(x=zb(n, H), g=zb(n, H), dg=zb(n, H), du=zb(n, H), dx=zb(n, H),
                                   dlogit=torch.zeros((max(n, 1),), dtype=F32, device=dev))
        return self._states[n]

    # -- text preparation: index plumbing (:96-107) --------------------------------------------------
    @staticmethod
    def _prepare_text(expression):
        B = expression.shape[0]
        ids = expression.new_zeros((B, expression.shape[1] + 2))
        ids[:, 0] = CLS
        ids[:, 1:-1] = expression
        sep_pos = (ids > 0).sum(1)
        ids[torch.arange(B, device=ids.device), sep_pos] = SEP
        return ids, ids.new_zeros(ids.shape), ids > 0

    def _features(self, image, boxes, im_info, expression):
        reps, obj_vl, box_mask, max_len = self._object_inputs(image, boxes, im_info, copy_boxes=True)      # (:80-86)
        ids, types, text_mask = self._prepare_text(expression)
        text_visual = reps[:, 0:1].expand(-1, ids.shape[1], -1)
        _, hs, _ = self.vlbert(ids, types, text_visual, text_mask, obj_vl, box_mask, output_all_encoded_layers=False,
                               output_text_and_object_separately=True)
        return hs, max_len

    @staticmethod
    def _boxes_f32(boxes):
        return boxes if (boxes.dtype == F32 and boxes.is_contiguous()) else boxes.float().contiguous()

    def train_forward(self, image, boxes, im_info, expression, label):
        boxes = self._boxes_f32(boxes)
        hs, max_len = self._features(image, boxes, im_info, expression)
        lab = label.to(F32).contiguous()
        logits, loss = _HeadFn.apply(hs, boxes, lab, self, self.training, *self._head_params())
        label_out = label.clone()                                  # padded back to origin_len with -1 (:150-152)
        label_out[:, max_len:] = -1
        return {"label_logits": logits, "label": label_out, "cls_loss": loss}, loss

    def inference_forward(self, image, boxes, im_info, expression):
        boxes = self._boxes_f32(boxes)
        hs, _ = self._features(image, boxes, im_info, expression)
        logits, _ = _HeadFn.apply(hs, boxes, None, self, False, *self._head_params())
        # argmax over all origin_len columns, as the reference (:219): a padded row inside max_len (logit final_mlp(0)) can win
        pred = torch.empty((boxes.shape[0], 4), dtype=F32, device=boxes.device)
        idx = torch.empty((boxes.shape[0],), dtype=torch.int64, device=boxes.device)
        ops.ground_pick_box(logits, boxes, im_info.to(F32).contiguous(), pred, idx)
        return {"label_logits": logits, "pred_boxes": pred, "pred_index": idx}
