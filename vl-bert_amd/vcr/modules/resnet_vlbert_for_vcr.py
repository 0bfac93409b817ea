"""Drop-in `ResNetVLBERT` for VCR fine-tuning (vcr/modules/resnet_vlbert_for_vcr.py:15-560) on the HIP library: same constructor
argument (the config tree of vcr/function/config.py), same `train_forward(image, boxes, masks, question, question_align_matrix,
answer_choices, answer_align_matrix, answer_label, im_info) -> (outputs, loss)` / `inference_forward(...) -> outputs`, same
parameter names (`image_feature_extractor.*`, `object_linguistic_embeddings.weight`, `vlbert._module.*`, `final_mlp.*`,
`cnn_loss_reg.*`), so the reference's trainer (vcr/function/train.py, SGD + gradient accumulation) and checkpoints work unchanged.

Composition, as in the reference (:226-399):
  FastRCNN mirror, image branch with the per-object masks (`segms`)                       -> obj_reps [B,R,H]
  per answer choice `[CLS] q [SEP] a [SEP]`, each token's visual embedding = the object its tag points at (index plumbing in
  torch, :116-167), object linguistic embedding = row clamp(class) of the 1-row / 81-row table (:303-308)
  `TimeDistributed` (common/nlp/time_distributed.py): the C answer choices fold into the batch -- the SAME engine rows, B*C
  sequences of up to 512 positions (beyond 256 on the streaming attention kernels) -- around the VisualLinguisticBert mirror with the pooler
  `final_mlp` on the pooled [CLS] -> logits [B,C]; sigmoid BCE with the positive-class weight (:344-356) or softmax CE (:358)
  ENABLE_CNN_REG_LOSS + CNN_LOSS_TOP (the shipped cfgs/vcr/*.yaml): every valid object's final hidden state -> transform
  (Linear + GELU) -> Dropout -> Linear(H, 81) -> CE against its detector class, one autograd node on the library (bf16 GEMMs with
  fused bias / GELU epilogues, vlb_ce_fwd_bwd, TN weight gradients).
The answer classifier (Dropout -> Linear(H,1) | 2fc) and the answer loss (weighted sigmoid BCE with the (w+1)/(2w) rescale, or softmax CE
over the choices) are one autograd node on the library as well (`_AnswerFn`).
Built as input plumbing: BLIND, NO_GROUNDING, NO_OBJ_ATTENTION, ANSWER_FIRST, QA_ONE_SENT.  Not built: object_word_embed_mode 3, IMAGE_SEMANTIC, the
bottom-of-the-CNN form of the regulariser (CNN_LOSS_TOP false), mask_position / mask_label (asserted off in the reference too).
"""
import torch
import torch.nn as nn

from ... import ops
from ...common.heads import Drop, Head, Linear, Linear16, cfg_get, run_head
from ...common.module import Module

F32 = torch.float32
CLS, SEP = 101, 102          # ids of '[CLS]', '[SEP]' in the BERT vocabularies (tokenizer lookups in the reference)
_TAG_REG, _TAG_A0, _TAG_A1 = 3001, 3002, 3003
NUM_OBJ_CLASSES = 81         # COCO detector classes of the VCR annotations (:26,38)


class TimeDistributed(nn.Module):
    """common/nlp/time_distributed.py:10-50: fold dimension 1 into dimension 0, apply, unfold every returned tensor."""

    def __init__(self, module):
        super().__init__()
        self._module = module

    def forward(self, *inputs, **kwargs):
        folded = []
        for t in inputs:
            if t.dim() <= 2:
                raise RuntimeError("No dimension to distribute: " + str(tuple(t.shape)))
            folded.append(t.contiguous().view(-1, *t.shape[2:]))
        lead = inputs[-1].shape[:2]
        out = self._module(*folded, **kwargs)
        unfold = lambda o: o.contiguous().view(*lead, *o.shape[1:])
        if isinstance(out, torch.Tensor):
            return unfold(out)
        if isinstance(out, tuple):
            return tuple(unfold(o) for o in out)
        raise ValueError("Not support!")


def one_column_wgrad(K, dev):
    """TN weight gradient of a Linear(<=K, 1) whose d(logits) lives in column 0 of a [rows, 64] buffer (the rest exactly zero): the GEMM
    runs on all 64 columns into fp32 staging, row 0 is the gradient."""
    gwp, gbp = torch.zeros((64, K), dtype=F32, device=dev), torch.zeros((64,), dtype=F32, device=dev)

    def wgrad(dz, x, gw, gb):
        gwp.zero_()
        gbp.zero_()
        ops.wgrad_tn(dz, x, gwp[:, :gw.shape[1]], colsum=gbp, workspace=None)
        gw.copy_(gwp[:1, :gw.shape[1]]); gb.copy_(gbp[:1])
    return wgrad


def answer_loss(answer_label, B, C, sigmoid, pos_weight, count):
    """The answer loss over the [B*C, 64] logits buffer of the classifier (column 0 live), as a Head loss: the weighted sigmoid BCE
    with the (w+1)/(2w) rescale, mean over the B*C logits (:344-356), or the softmax CE over the C choices of a sample (:358) through a
    [B, 64] staging buffer.  count: fp32 [1] scratch of vlb_ce_fwd_bwd."""
    n = B * C

    def loss_fn(z, z_copy, loss, g, fresh):
        if sigmoid:
            rescale = (pos_weight + 1.0) / (2.0 * pos_weight)
            lab = torch.zeros((n,), dtype=F32, device=z.device)
            lab.view(B, C).scatter_(1, answer_label.long().view(B, 1), 1.0)          # one-hot of the right answer (index plumbing)
            ops.bce_logits_fwd_bwd(z, 1, lab.view(n, 1), loss, gscale=g * rescale, logits_copy=z_copy, pos_weight=pos_weight)
            loss.mul_(rescale)
        else:
            z_copy.copy_(z)
            zc = torch.zeros((B, 64), dtype=z.dtype, device=z.device)
            zc[:, :C].copy_(z[:, 0].view(B, C))
            ops.ce_fwd_bwd(zc, C, answer_label.long().contiguous().view(-1), count, loss, gscale=g)
            z.zero_()
            z[:, 0].copy_(zc[:, :C].reshape(-1))
    return loss_fn


class ResNetVLBERT(Module):
    SEED = 40011

    def _check_config(self, net, vl):
        for flag in ("FOR_MASK_VL_MODELING_PRETRAIN", "IMAGE_SEMANTIC"):
            if cfg_get(net, flag, False):
                raise NotImplementedError("NETWORK.%s is not supported" % flag)
        # ablation switches of the reference's forward (:253-330): all of them are input plumbing in front of the same encoder
        self.blind = bool(cfg_get(net, "BLIND", False))                      # no visual input at all: zero features, no object positions
        self.no_grounding = bool(cfg_get(net, "NO_GROUNDING", False))        # every token tagged with box 0 (the whole image)
        self.no_obj_attention = bool(cfg_get(net, "NO_OBJ_ATTENTION", False))      # objects feed the token embeddings but are not attended
        self.answer_first = bool(cfg_get(net, "ANSWER_FIRST", False))        # [CLS] answer [SEP] question [SEP]
        self.qa_one_sent = bool(cfg_get(net, "QA_ONE_SENT", False))          # [CLS] question answer [SEP], one segment
        if self.answer_first and self.qa_one_sent:
            raise NotImplementedError("ANSWER_FIRST with QA_ONE_SENT (the reference raises as well, :276-277)")
        if self.blind and cfg_get(net, "ENABLE_CNN_REG_LOSS", False):
            raise NotImplementedError("BLIND with ENABLE_CNN_REG_LOSS: there are no object positions to classify")
        self.embed_mode = int(cfg_get(vl, "object_word_embed_mode", 2))
        if self.embed_mode not in (1, 2):
            raise NotImplementedError("object_word_embed_mode must be 1 (81 class embeddings) or 2 (one shared embedding)")
        self.NUM_OBJECT_WORDS = NUM_OBJ_CLASSES if self.embed_mode == 1 else 1
        self.enable_cnn_reg_loss = bool(cfg_get(net, "ENABLE_CNN_REG_LOSS", False))
        self.cnn_loss_top = bool(cfg_get(net, "CNN_LOSS_TOP", False))
        if self.enable_cnn_reg_loss and not self.cnn_loss_top:
            raise NotImplementedError("ENABLE_CNN_REG_LOSS needs CNN_LOSS_TOP (the form of the shipped cfgs/vcr/*.yaml)")
        self.classifier = cfg_get(net, "CLASSIFIER_TYPE", "2fc")
        if self.classifier not in ("1fc", "2fc"):
            raise ValueError("Not support classifier type: {}!".format(self.classifier))

    def _wrap_encoder(self, vlbert):
        return TimeDistributed(vlbert)

    def _build_heads(self, net, vl):
        H = self.H
        self.sigmoid = bool(cfg_get(net, "CLASSIFIER_SIGMOID", False))
        self.pos_weight = float(cfg_get(net, "CLASSIFIER_SIGMOID_LOSS_POSITIVE_WEIGHT", 1.0))
        self.reg_drop = float(cfg_get(net, "CNN_REG_DROPOUT", 0.0))
        self.ans_loss_weight = float(cfg_get(net, "ANS_LOSS_WEIGHT", 1.0))
        self.cnn_loss_weight = float(cfg_get(net, "CNN_LOSS_WEIGHT", 1.0))
        self.hc = int(cfg_get(net, "CLASSIFIER_HIDDEN_SIZE", 1024)) if self.classifier != "1fc" else H
        if self.hc % 64:
            raise NotImplementedError("CLASSIFIER_HIDDEN_SIZE must be a multiple of 64")
        # final_mlp (:62-82): Dropout -> Linear(H,1) | Dropout -> Linear(H,hc) -> ReLU -> Dropout -> Linear(hc,1); the 1-output Linear's
        # W^T is [hc, 64] with one live column
        mlp = nn.Module()
        wgrad = one_column_wgrad(max(H, self.hc), self.device_)
        self._count = torch.zeros((1,), dtype=F32, device=self.device_)
        if self.classifier == "1fc":
            mlp.add_module("1", self._lin(1, H))
            stages = [Drop(_TAG_A0), Linear(Linear16(getattr(mlp, "1")), wgrad=wgrad)]
        else:
            mlp.add_module("1", self._lin(self.hc, H))
            mlp.add_module("4", self._lin(1, self.hc))
            stages = [Drop(_TAG_A0), Linear(Linear16(getattr(mlp, "1")), "relu"), Drop(_TAG_A1), Linear(Linear16(getattr(mlp, "4")), wgrad=wgrad)]
        self.final_mlp = mlp
        self._cls_head = Head(stages, self._seed)
        if self.enable_cnn_reg_loss:              # transform (Linear + GELU) -> Dropout -> Linear(H, 81)  (:33-37); n changes per batch
            reg = nn.Module()
            reg.add_module("0", self._transform())
            reg.add_module("2", self._lin(NUM_OBJ_CLASSES, H))
            self.cnn_loss_reg = reg
            self._reg_head = Head([Linear(Linear16(getattr(reg, "0").dense), "gelu"), Drop(_TAG_REG), Linear(Linear16(getattr(reg, "2")))],
                                  self._seed, row_cap=64)
    def init_weight(self):
        """:84-97: N(0, 0.02) object word embeddings and regulariser head, xavier-uniform classifier, zero biases."""
        with torch.no_grad():
            self.image_feature_extractor.init_weight()
            self.object_linguistic_embeddings.weight.normal_(0.0, 0.02)
            if self.enable_cnn_reg_loss:
                for q in self._reg_head.params():
                    if q.dim() == 2:
                        q.normal_(0.0, 0.02)
                    else:
                        q.zero_()
            for m in self.final_mlp.children():
                nn.init.xavier_uniform_(m.weight)
                m.bias.zero_()

    def train(self, mode=True):
        super().train(mode)
        self.image_feature_extractor.bn_eval()            # frozen BatchNorm (:99-104); the HIP vision stack folds it anyway
        return self

    def load_state_dict(self, state_dict, strict=True):
        """the FastRCNN mirror converts its convolution layout ([O,KH,KW,I] <-> the reference's [O,I,KH,KW]) and drops the reference's
        `head.0.*` alias keys in its own load_state_dict, which nn.Module's recursion does not call for sub-modules (state_dict's
        recursion does): hand it its slice directly, load the rest here"""
        pre = "image_feature_extractor."
        self.image_feature_extractor.load_state_dict({k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}, strict=strict)
        rest = {k: v for k, v in state_dict.items() if not k.startswith(pre)}
        res = super().load_state_dict(rest, strict=False)
        missing = [k for k in res.missing_keys if not k.startswith(pre)]
        if strict and (missing or res.unexpected_keys):
            raise RuntimeError("Error(s) in loading state_dict for ResNetVLBERT: missing %s, unexpected %s" % (missing, res.unexpected_keys))
        return res

    # -- text preparation: index plumbing (prepare_text_from_qa / _qa_onesent / _aq, :136-224) ------------------------
    @staticmethod
    def _prepare_text(question, question_tags, question_mask, answers, answers_tags, answers_mask, order="qa"):
        """order: "qa"  [CLS] q [SEP] a [SEP] (segment 1 = answer + its [SEP]) | "qa_onesent"  [CLS] q a [SEP] (one segment) |
        "aq"  [CLS] a [SEP] q [SEP] (segment 1 = question + its [SEP])"""
        B, Lq = question.shape
        _, C, La = answers.shape
        n_sep = 1 if order == "qa_onesent" else 2
        L = int((question_mask.sum(1) + answers_mask.sum(2).max(1)[0]).max()) + 1 + n_sep
        d = question.device
        question = question[:, None, :].expand(B, C, Lq)
        qmask = question_mask[:, None, :].expand(B, C, Lq)
        nq, na = qmask.sum(2, keepdim=True), answers_mask.sum(2, keepdim=True)
        k = torch.arange(L, device=d)[None, None, :].expand(B, C, L)
        ids = torch.zeros((B, C, L), dtype=question.dtype, device=d)
        tags = torch.zeros((B, C, L), dtype=question.dtype, device=d)
        if order == "qa":
            first_end, last_end = 1 + nq, 2 + nq + na                 # positions of the two [SEP]
            q_in, a_in = (k > 0) & (k < first_end), (k > first_end) & (k < last_end)
        elif order == "aq":
            first_end, last_end = 1 + na, 2 + na + nq
            a_in, q_in = (k > 0) & (k < first_end), (k > first_end) & (k < last_end)
        else:
            first_end, last_end = 1 + nq, 1 + nq + na                 # no separator between question and answer
            q_in, a_in = (k > 0) & (k < first_end), (k >= first_end) & (k < last_end)
        mask = k <= last_end
        types = ((k > first_end) & (k <= last_end)).to(question.dtype) if order != "qa_onesent" else torch.zeros_like(ids)
        ids[:, :, 0] = CLS
        if order != "qa_onesent":
            ids[k == first_end] = SEP
        ids[k == last_end] = SEP
        ids[q_in] = question[qmask]
        ids[a_in] = answers[answers_mask]
        tags[q_in] = question_tags[qmask]
        tags[a_in] = answers_tags[answers_mask]
        return ids, types, tags, mask

    def _encode(self, image, boxes, masks, question, answer_choices, im_info):
        objects = boxes[:, :, -1]
        boxes4 = boxes[:, :, :4]
        box_mask = boxes4[:, :, -1] > -0.5
        max_len = int(box_mask.sum(1).max())
        objects, box_mask, boxes4, segms = objects[:, :max_len], box_mask[:, :max_len], boxes4[:, :max_len], masks[:, :max_len]
        B, R = box_mask.shape
        if self.blind:
            reps = torch.zeros((B, R, self.H), dtype=F32, device=boxes4.device)
        else:
            reps = self.image_feature_extractor(images=image, boxes=boxes4, box_mask=box_mask, im_info=im_info, classes=objects,
                                                segms=segms)["obj_reps"]
        C = answer_choices.shape[1]
        q_ids, q_tags = question[:, :, 0], question[:, :, 1]
        q_tags = q_tags[:, None, :].expand(-1, C, -1)
        q_mask = question[:, :, 0] > 0.5
        a_ids, a_tags = answer_choices[:, :, :, 0], answer_choices[:, :, :, 1]
        a_mask = answer_choices[:, :, :, 0] > 0.5
        order = "aq" if self.answer_first else ("qa_onesent" if self.qa_one_sent else "qa")
        ids, types, tags, text_mask = self._prepare_text(q_ids, q_tags, q_mask, a_ids, a_tags, a_mask, order=order)
        if self.no_grounding:
            tags = torch.zeros_like(tags)
        L = ids.shape[2]
        rows = torch.arange(B, device=ids.device)[:, None, None].expand(B, C, L)
        text_visual = reps[rows.reshape(-1), tags.clamp(min=0).reshape(-1)].view(B, C, L, -1)          # _collect_obj_reps (:116-134)
        if self.blind:
            ling = torch.zeros_like(reps)
        else:
            table = self.object_linguistic_embeddings.weight
            ling = table[objects.long().clamp(min=0, max=table.shape[0] - 1)]
        obj_vl = torch.cat((reps, ling), -1)[:, None].expand(B, C, R, -1)
        attend = torch.zeros_like(box_mask) if (self.no_obj_attention or self.blind) else box_mask
        text_out, obj_out, pooled = self.vlbert(ids, types, text_visual, text_mask, obj_vl, attend[:, None].expand(B, C, R),
                                                output_all_encoded_layers=False, output_text_and_object_separately=True)
        return pooled, obj_out, objects, box_mask

    def _classify(self, pooled, answer_label=None):
        """-> (label_logits [B,C], ans_loss | None): `final_mlp` and the answer loss, one autograd node on the library."""
        B, C, H = pooled.shape
        loss_fn = answer_loss(answer_label, B, C, self.sigmoid, self.pos_weight, self._count) if answer_label is not None else None
        z, loss = run_head(self._cls_head, pooled.float().reshape(B * C, H), self.cls_drop if self.training else 0.0, loss_fn)
        logits = z[:, 0].float().view(B, C)                 # (glue: the [B,C] fp32 tensor the outputs dict carries)
        return logits, (loss if answer_label is not None else None)

    def _regularize(self, x, labels):
        """x [n,H] fp32 (final hidden states of the valid objects), labels [n] -> CE loss of `cnn_loss_reg` (:391-394), one autograd node"""
        def ce(logits, logits_copy, loss, g, fresh):
            ops.ce_fwd_bwd(logits, NUM_OBJ_CLASSES, labels.contiguous(), self._count, loss, gscale=g, logits_copy=logits_copy if fresh else None)
        return run_head(self._reg_head, x, self.reg_drop if self.training else 0.0, ce)[1]

    def train_forward(self, image, boxes, masks, question, question_align_matrix, answer_choices, answer_align_matrix, answer_label,
                      im_info, mask_position=None, mask_type=None, mask_label=None):
        if mask_position is not None:
            raise NotImplementedError("mask_position (asserted off in the reference, :365)")
        pooled, obj_out, objects, box_mask = self._encode(image, boxes, masks, question, answer_choices, im_info)
        logits, ans_loss = self._classify(pooled, answer_label)
        B, C = logits.shape
        outputs = {}
        if self.sigmoid:
            outputs["positive_fraction"] = torch.full((), 1.0 / C, dtype=logits.dtype, device=logits.device)     # one right answer per sample
        outputs.update({"label_logits": logits, "label": answer_label.long().view(-1), "ans_loss": ans_loss})
        loss = ans_loss.mean() * self.ans_loss_weight
        if self.enable_cnn_reg_loss:
            R = box_mask.shape[1]
            sel = box_mask[:, None].expand(B, C, R)
            labels = objects[:, None].expand(B, C, R)[sel].long()
            reg_loss = self._regularize(obj_out[sel].float(), labels)
            loss = loss + reg_loss * self.cnn_loss_weight
            outputs["cnn_regularization_loss"] = reg_loss
        return outputs, loss

    def inference_forward(self, image, boxes, masks, question, question_align_matrix, answer_choices, answer_align_matrix, *args):
        im_info = args[-1]
        pooled, _, _, _ = self._encode(image, boxes, masks, question, answer_choices, im_info)
        return {"label_logits": self._classify(pooled)[0]}
