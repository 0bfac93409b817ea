"""fp32 ends of the module-API engine on the fp32 encoder (`PretrainEngine(..., fp32_ends=True)`, the VQA fine-tuning route): with
them no 16-bit tensor lies between the caller's embeddings and the sequence output, nor on the way back.

CoreFrontF32: VisualLinguisticBert.embedding (common/visual_linguistic_bert.py:173-241) on the caller's fp32 embeddings and the fp32
MASTER tables (csrc/f32_ends.hip), written straight into the encoder's X[0].  SequenceOutF32: the caller reads the encoder's own X[L]
and hands an fp32 d X[L] in; there is nothing to compute in between.
"""
import torch

from . import ops
from .engine import F32, TAG_EMBED
from .ends_16 import EMBED_GRADS


class CoreFrontF32:
    def __init__(self, eng):
        self.eng = eng
        T, Bt, BT, BR, M, H = eng.T, eng.Bt, eng.BT, eng.BR, eng.M, eng.cfg.hidden_size
        z = lambda *s: torch.zeros(s, dtype=F32, device=eng.dev)
        self.in_text_type = torch.zeros((Bt, T), dtype=torch.int64, device=eng.dev)
        self.tv_in32, self.ovl_in32 = z(BT, H), z(BR, 2 * H)        # the caller's embeddings stay fp32
        self.tv_n32, self.st_tv = z(BT, H), z(BT, 2)
        self.objvis32, self.st_objvis = z(BR, H), z(BR, 2)
        self.emb_pre32, self.st_emb = z(M, H), z(M, 2)
        self.d_tv_n, self.d_objvis = z(BT, H), z(BR, H)
        self.d_tv_in32, self.d_ovl_in32 = z(BT, H), z(BR, 2 * H)    # gradients handed back to autograd
        self.x0 = eng.encoder.x_in

    def transposes(self):
        return []

    def refresh(self):
        pass

    def overwritten(self):
        return None      # as CoreFront16: the module mirrors accumulate

    def grads(self):
        return [self.eng.g32[n] for n in EMBED_GRADS]

    def set_inputs(self, text_token_type_ids, text_visual_embeddings, object_vl_embeddings):
        e = self.eng
        self.in_text_type.copy_(text_token_type_ids)
        self.tv_in32.view(e.Bt, e.T, -1).copy_(text_visual_embeddings)
        self.ovl_in32.view(e.Bt, e.R, -1).copy_(object_vl_embeddings)

    def input_grads(self):
        e, H = self.eng, self.eng.cfg.hidden_size
        return self.d_tv_in32.view(e.Bt, e.T, H), self.d_ovl_in32.view(e.Bt, e.R, 2 * H)

    def front_fwd(self, p_h, p_ds):
        e = self.eng
        T, R, S, Bt, H = e.T, e.R, e.S, e.Bt, e.cfg.hidden_size
        w32 = e.w32
        ops.layernorm_f32_fwd(self.tv_in32, w32["vlbert.visual_ln_text.weight"], w32["vlbert.visual_ln_text.bias"], self.tv_n32,
                              self.st_tv)
        ops.layernorm_f32_fwd(self.ovl_in32[:, :H], w32["vlbert.visual_ln_object.weight"], w32["vlbert.visual_ln_object.bias"],
                              self.objvis32, self.st_objvis)
        ops.embed_f32_fwd(e.lay, e.in_text, self.in_text_type, w32["vlbert.word_embeddings.weight"],
                          w32["vlbert.position_embeddings.weight"], w32["vlbert.token_type_embeddings.weight"],
                          w32["vlbert.end_embedding.weight"], self.tv_n32, (T * H, H), self.objvis32, (R * H, H),
                          (self.ovl_in32, H), (R * 2 * H, 2 * H), None, w32["vlbert.embedding_LayerNorm.weight"],
                          w32["vlbert.embedding_LayerNorm.bias"], self.emb_pre32, self.st_emb, self.x0, Bt, T, R, S, H,
                          drop_p=p_h, seed=e.seed, tag=TAG_EMBED)

    def front_bwd(self, dx, p_h, p_ds, on_layer_done=None):
        """dx: the fp32 d X[0]; d(object linguistic half) is written straight into the handed-back gradient."""
        e = self.eng
        T, R, S, Bt, H = e.T, e.R, e.S, e.Bt, e.cfg.hidden_size
        w32, g32 = e.w32, e.g32
        self.d_tv_n.zero_()
        self.d_objvis.zero_()
        self.d_ovl_in32.zero_()
        pe = "vlbert.embedding_LayerNorm."
        ops.embed_f32_bwd(dx, self.emb_pre32, self.st_emb, w32[pe + "weight"], e.lay, e.in_text, self.in_text_type, None,
                          g32["vlbert.word_embeddings.weight"], g32["vlbert.position_embeddings.weight"],
                          g32["vlbert.token_type_embeddings.weight"], g32["vlbert.end_embedding.weight"], g32[pe + "weight"],
                          g32[pe + "bias"], self.d_tv_n, (T * H, H), self.d_objvis, (R * H, H), (self.d_ovl_in32, H),
                          (R * 2 * H, 2 * H), Bt, T, R, S, H, drop_p=p_h, seed=e.seed, tag=TAG_EMBED)
        ops.layernorm_f32_bwd(self.d_tv_n, self.tv_in32, self.st_tv, w32["vlbert.visual_ln_text.weight"], dx=self.d_tv_in32,
                              dgamma=g32["vlbert.visual_ln_text.weight"], dbeta=g32["vlbert.visual_ln_text.bias"])
        ops.layernorm_f32_bwd(self.d_objvis, self.ovl_in32[:, :H], self.st_objvis, w32["vlbert.visual_ln_object.weight"],
                              dx=self.d_ovl_in32[:, :H], dgamma=g32["vlbert.visual_ln_object.weight"],
                              dbeta=g32["vlbert.visual_ln_object.bias"])


class SequenceOutF32:
    """The caller reads X[L] (engine.sequence_output) and writes d X[L] into `dx` (engine.backward_core_sequence)."""

    def __init__(self, eng):
        self.dx = torch.zeros((eng.M, eng.cfg.hidden_size), dtype=F32, device=eng.dev)

    def transposes(self):
        return []

    def refresh(self):
        pass

    def overwritten(self):
        return None      # no heads run: nothing overwrites their gradients

    def heads_fwd(self):
        pass

    def outputs(self):
        return (None,) * 6

    def heads_bwd(self):
        return self.dx
