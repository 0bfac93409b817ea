"""Drop-in `ResNetVLBERT` for VQA fine-tuning (vqa/modules/resnet_vlbert_for_vqa.py:14-300) on the HIP library: same constructor
argument (the config tree of vqa/function/config.py), same `train_forward(image, boxes, im_info, question, label) -> (outputs, loss)`
and `inference_forward(image, boxes, im_info, question) -> outputs`, same parameter names (`image_feature_extractor.*`,
`object_linguistic_embeddings.weight`, `vlbert.*`, `final_mlp.*`), so the reference's trainer and checkpoints work unchanged.

Composition, as in the reference:  FastRCNN mirror (precomputed features or images) -> text = [CLS] question [SEP] [MASK] [SEP]
(index plumbing in torch, :142-167) -> VisualLinguisticBert mirror (packed sequence output) -> hidden state at the [MASK] position ->
`final_mlp` -> BCE-with-logits x answers (:226).  The classifier and the loss are ONE autograd node running on the library: bf16 GEMMs
with fused bias / ReLU / GELU epilogues, LayerNorm, counter-RNG dropout (vlb_dropout_bf16), vlb_bce_logits_fwd_bwd (loss and its
gradient in one pass), TN weight-gradient GEMMs.  CLASSIFIER_TYPE "2fc" (config default) and "mlm" (the shipped cfgs/vqa/*.yaml)
are built; "1fc", BLIND, NO_GROUNDING, CLASSIFIER_SIGMOID, cnn_reg_loss raise NotImplementedError.

`fp32_ends` (VLBERT config key, or VLB_FP32_ENDS=1; needs `fp32_encoder`): the whole route in fp32 -- the FastRCNN mirror's fp32
precomputed branch, the fp32 embedding and encoder, the classifier built from the fp32 stages of common/heads.py on the master weights,
vlb_bce_logits_f32_fwd_bwd.  No 16-bit tensor between the inputs and the loss, forward or backward.
"""
import torch
import torch.nn as nn

from ... import ops
from ...common import language_pretrained as _lp
from ...common.heads import Drop, Drop32, Head, Head32, LayerNorm, LayerNorm32, Linear, Linear16, Linear32, Weight32, cfg_get, run_head
from ...common.module import Module

CLS, SEP, MASK = 101, 102, 103          # ids of '[CLS]', '[SEP]', '[MASK]' in the BERT vocabularies (tokenizer lookups in the reference)
_TAG0, _TAG1 = 2001, 2002


class ResNetVLBERT(Module):
    SEED = 30011
    FP32_ENDS = True

    def _check_config(self, net, vl):
        if cfg_get(net, "BLIND", False) or cfg_get(net, "NO_GROUNDING", False) or cfg_get(net, "ENABLE_CNN_REG_LOSS", False):
            raise NotImplementedError("BLIND / NO_GROUNDING / ENABLE_CNN_REG_LOSS are not supported")
        # (CLASSIFIER_SIGMOID is a key of the shared config schema that the reference's VQA module never reads: the answer loss is
        #  always the sigmoid BCE of :226)
        if cfg_get(vl, "object_word_embed_mode", 2) != 2:
            raise NotImplementedError("object_word_embed_mode must be 2 (one shared object word embedding)")
        self.classifier = cfg_get(net, "CLASSIFIER_TYPE", "2fc")
        if self.classifier not in ("2fc", "1fc", "mlm"):
            raise ValueError("Not support classifier type: %s!" % self.classifier)       # (the reference's message, :75-76)

    def _build_heads(self, net, vl):
        H = self.H
        self.answers = int(cfg_get(cfg_get(self.config, "DATASET"), "ANSWER_VOCAB_SIZE", 3129))
        self.hc = int(cfg_get(net, "CLASSIFIER_HIDDEN_SIZE", 1024)) if self.classifier == "2fc" else H
        mlp = nn.Module()
        last = lambda lin: Linear(Linear16(lin, pad_k=True))          # its input rows are padded to a multiple of 64 columns
        Drop_, LayerNorm_, Head_ = Drop, LayerNorm, Head
        if self.fp32_ends:                        # the same stages in fp32, on the master weights
            Linear_ = lambda lin, act=None: Linear32(Weight32(lin), act)
            last, Drop_, LayerNorm_, Head_ = Linear_, Drop32, LayerNorm32, Head32
        else:
            Linear_ = lambda lin, act=None: Linear(Linear16(lin), act)
        if self.classifier == "2fc":              # Dropout -> Linear(H, hc) -> ReLU -> Dropout -> Linear(hc, answers)  (:54-63)
            mlp.add_module("1", self._lin(self.hc, H))
            mlp.add_module("4", self._lin(self.answers, self.hc))
            stages = [Drop_(_TAG0), Linear_(getattr(mlp, "1"), "relu"), Drop_(_TAG1), last(getattr(mlp, "4"))]
        elif self.classifier == "1fc":            # Dropout -> Linear(H, answers)  (:64-68)
            mlp.add_module("1", self._lin(self.answers, H))
            stages = [Drop_(_TAG0), last(getattr(mlp, "1"))]
        else:                                     # BertPredictionHeadTransform (dense + gelu + LayerNorm) -> Dropout -> Linear  (:69-74)
            mlp.add_module("0", self._transform(layer_norm=True))
            mlp.add_module("2", self._lin(self.answers, H))
            tr = getattr(mlp, "0")
            stages = [Linear_(tr.dense, "gelu"), LayerNorm_(tr.LayerNorm), Drop_(_TAG1), last(getattr(mlp, "2"))]
        self.final_mlp = mlp
        self._head = Head_(stages, self._seed)

    def init_weight(self):
        """resnet_vlbert_for_vqa.py:84-110: xavier-uniform classifier Linears, zero biases, N(0, 0.02) object word embedding."""
        with torch.no_grad():
            self.image_feature_extractor.init_weight()
            self.object_linguistic_embeddings.weight.normal_(0.0, 0.02)
            for q in self._head.params():
                if q.dim() == 2:
                    nn.init.xavier_uniform_(q)
            if self.classifier == "mlm":
                t = getattr(self.final_mlp, "0")
                t.dense.bias.zero_()
                if self.language_pretrained_model_path is not None:
                    # the classifier's transform starts from the language model's MLM transform (:97-110).  (Without a checkpoint the
                    # reference dies in torch.load(None); the mirror keeps the random init so that synthetic benches can run.)
                    sd = torch.load(self.language_pretrained_model_path, map_location="cpu")
                    tsd, keys = _lp.mlm_transform_state_dict(sd)
                    print("loading pretrained classifier transform keys: {}.".format(keys))
                    _lp.apply([(k, v, None) for k, v in tsd.items()],
                              {"dense.weight": t.dense.weight, "dense.bias": t.dense.bias, "LayerNorm.weight": t.LayerNorm.weight,
                               "LayerNorm.bias": t.LayerNorm.bias}, strict_keys=True)

    # -- text preparation: index plumbing (prepare_text_from_qa, :142-167, with the single [MASK] answer token of :192-196) ----------
    @staticmethod
    def _prepare_text(question):
        B = question.shape[0]
        qmask = question > 0
        qlen = qmask.sum(1)
        L = int(qlen.max()) + 4
        q_end = (1 + qlen)[:, None]
        a_end = q_end + 2
        j = torch.arange(L, device=question.device)[None, :]
        ids = torch.zeros((B, L), dtype=question.dtype, device=question.device)
        types = ((j > q_end) & (j <= a_end)).to(question.dtype)
        mask = j <= a_end
        ids[:, 0] = CLS
        ids[(j > 0) & (j < q_end)] = question[qmask]
        ids[j == q_end] = SEP
        ids[j == q_end + 1] = MASK
        ids[j == a_end] = SEP
        return ids, types, mask, (a_end - 1).squeeze(1)

    def _classify(self, image, boxes, im_info, question, label, train):
        """-> (label_logits [B, answers] fp32, loss): the hidden state at the [MASK] position through final_mlp + BCE, one autograd node"""
        reps, obj_vl, box_mask, _ = self._object_inputs(image, boxes, im_info)
        ids, types, text_mask, ans_pos = self._prepare_text(question)
        text_visual = reps[:, 0:1].expand(-1, ids.shape[1], -1)                 # text tags are all 0 (:198-209)
        seq, _ = self.vlbert(ids, types, text_visual, text_mask, obj_vl, box_mask, output_all_encoded_layers=False)
        hm = seq[torch.arange(seq.shape[0], device=seq.device), ans_pos]
        A = self.answers

        def bce(logits, logits_copy, loss, g, fresh):
            fn = ops.bce_logits_f32_fwd_bwd if self.fp32_ends else ops.bce_logits_fwd_bwd
            fn(logits, A, label.detach().float().contiguous(), loss, gscale=g, logits_copy=logits_copy if fresh else None)
        logits, loss = run_head(self._head, hm, self.cls_drop if train else 0.0, bce if label is not None else None)
        # (fp32_ends: the head's own fp32 buffer, rewritten by its next pass -- the caller gets a copy)
        return (logits[:, :A].clone() if logits.dtype == torch.float32 else logits[:, :A].float()), loss

    def train_forward(self, image, boxes, im_info, question, label):
        logits, loss = self._classify(image, boxes, im_info, question, label, self.training)
        return {"label_logits": logits, "label": label, "ans_loss": loss}, loss

    def inference_forward(self, image, boxes, im_info, question):
        return {"label_logits": self._classify(image, boxes, im_info, question, None, False)[0]}
