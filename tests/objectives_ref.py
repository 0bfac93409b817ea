"""Torch CPU restatement of the four pre-training objective switches -- NETWORK.WITH_MLM_LOSS, WITH_MVRC_LOSS,
MLM_LOSS_NORM_IN_BATCH_FIRST, MVRC_LOSS_NORM_IN_BATCH_FIRST (pretrain/modules/resnet_vlbert_for_pretraining.py:26-27, 140-141, 164-200;
multitask :205-271) -- composed from the oracle's public pieces (oracle/vlbert_oracle.py).  Test infrastructure: what the engine's
objective variants and the row-weighted loss kernels are compared against."""
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import vlbert_oracle as O


@dataclass(frozen=True)
class Switches:
    with_mlm_loss: bool = True
    with_mvrc_loss: bool = True
    mlm_norm_in_batch_first: bool = False
    mvrc_norm_in_batch_first: bool = False

    def engine_kw(self):
        return dict(with_mlm_loss=self.with_mlm_loss, with_mvrc_loss=self.with_mvrc_loss,
                    mlm_norm_in_batch_first=self.mlm_norm_in_batch_first, mvrc_norm_in_batch_first=self.mvrc_norm_in_batch_first)


ABSENT_MLM = "vlbert.mlm_head."
ABSENT_MVRC = ("vlbert.mvrc_head.", "object_mask_word_embedding.")


def absent(name, sw):
    return (not sw.with_mlm_loss and name.startswith(ABSENT_MLM)) or (not sw.with_mvrc_loss and name.startswith(ABSENT_MVRC))


def init_params(cfg, seed, sw):
    """init_params(seed) of the oracle with the keys of the absent heads deleted (the present tensors keep their values)."""
    return {k: v for k, v in O.init_params(cfg, seed=seed).items() if not absent(k, sw)}


def norm_first_ce(logits, labels):
    """:168-174 -- per-sample means, then the mean over the samples that have a label.  logits [B, T, V], labels [B, T]."""
    l = F.cross_entropy(logits.transpose(1, 2), labels, ignore_index=-1, reduction="none")
    n = (labels != -1).sum(1, keepdim=True).to(l.dtype)
    n_has = (n != 0).sum().to(l.dtype)
    return (l / (n + 1e-4)).sum() / (n_has + 1e-4)


def norm_first_soft_ce(logits, target):
    """:183-190.  logits / target [B, R, C]; a batch without a valid row gives 0 (common/utils/misc.py:140-141)."""
    C = logits.shape[-1]
    x, t = logits.reshape(-1, C), target.reshape(-1, C)
    valid = (t.sum(1) - 1).abs() < 1.0e-1
    if int(valid.sum()) == 0:
        return logits.sum() * 0.0
    l = torch.zeros(x.shape[0], dtype=x.dtype)
    l = l.masked_scatter(valid, (-F.log_softmax(x[valid], 1) * t[valid]).sum(1)).view(logits.shape[:-1])
    v = valid.view(logits.shape[:-1])
    return (l / (v.sum(1, keepdim=True).to(l.dtype) + 1e-4)).sum() / ((v.sum(1) != 0).sum().to(l.dtype) + 1e-4)


def weighted_ce(logits, labels, B, T, B_split=None, gscale=1.0):
    """Stand-alone per-sample-normalised CE over rows [B * T, V] (labelled iff 0 <= label < V) -> (loss0, loss1, d(logits)):
    samples [0, B_split) form the first group, the rest the second, each with its own count of samples that have a label."""
    B_split = B if B_split is None else B_split
    x = logits.detach().double().clone().requires_grad_(True)
    V = x.shape[1]
    lab = labels.view(B, T).clone()
    lab[(lab < 0) | (lab >= V)] = -1
    xs = x.view(B, T, V)
    zero = x.sum() * 0.0
    l0 = norm_first_ce(xs[:B_split], lab[:B_split]) if B_split > 0 else zero
    l1 = norm_first_ce(xs[B_split:], lab[B_split:]) if B_split < B else zero
    ((l0 + l1) * gscale).backward()
    return float(l0), float(l1), x.grad.float()


def weighted_soft_ce(logits, target, B, R, gscale=1.0):
    """Stand-alone per-sample-normalised soft-label CE over rows [B * R, C] -> (loss, d(logits))."""
    x = logits.detach().double().clone().requires_grad_(True)
    C = x.shape[1]
    l = norm_first_soft_ce(x.view(B, R, C), target.double().view(B, R, C))
    (l * gscale).backward()
    return float(l), x.grad.float()


def forward(p, cfg, batch, sw, train=False, drop_hook=None):
    """The plain (7 tensors) or multitask (9 tensors) wrapper's forward under the switches `sw` -> (outputs, loss)."""
    multitask = len(batch) == 9
    boxes, im_info, text, rel_label, mlm_labels, mvrc_ops, mvrc_labels = batch[:7]
    boxes = boxes.clone()
    box_mask = boxes[:, :, 0] > -1.5
    max_len = int(box_mask.sum(1).max())
    box_mask, boxes = box_mask[:, :max_len], boxes[:, :max_len]
    mvrc_ops, mvrc_labels = mvrc_ops[:, :max_len], mvrc_labels[:, :max_len]
    feats = boxes[:, :, 4:].clone()
    feats[mvrc_ops == 1] = p["object_mask_visual_embedding.weight"][0]      # :114-117, whatever the switches say
    boxes = torch.cat((boxes[:, :, :4], feats), -1)
    obj_reps = O.fast_rcnn_precomputed(p, cfg, boxes, box_mask, im_info, train, drop_hook=drop_hook)
    B, R = box_mask.shape
    H = cfg.hidden_size
    ling = p["object_linguistic_embeddings.weight"][0].expand(B, R, -1).clone()
    if sw.with_mvrc_loss:                                                    # :140-141
        ling[mvrc_ops == 1] = p["object_mask_word_embedding.weight"][0]
    obj_vl = torch.cat((obj_reps, ling), -1)
    if multitask:
        aux_text, aux_labels = batch[7], batch[8]
        Ba, T = aux_text.shape[0], max(text.shape[1], aux_text.shape[1])
        text_m = text.new_zeros((B + Ba, T))
        text_m[:B, :text.shape[1]] = text
        text_m[B:, :aux_text.shape[1]] = aux_text
        tv = obj_reps.new_zeros((B + Ba, T, H))
        tv[:B, :text.shape[1]] = obj_reps[:, 0:1].expand(-1, text.shape[1], -1)
        tv[B:] = p["aux_text_visual_embedding.weight"][0]
        ovl = obj_vl.new_zeros((B + Ba, R, 2 * H))
        ovl[:B] = obj_vl
        bm = box_mask.new_zeros((B + Ba, R))
        bm[:B] = box_mask
        labels = mlm_labels.new_full((B + Ba, T), -1)
        labels[:B, :mlm_labels.shape[1]] = mlm_labels
        labels[B:, :aux_labels.shape[1]] = aux_labels
    else:
        Ba, text_m, tv, ovl, bm, labels = 0, text, obj_reps[:, 0:1].expand(-1, text.shape[1], -1), obj_vl, box_mask, mlm_labels
    text_out, obj_out, pooled, seq = O.vlbert_forward(p, cfg, text_m, torch.zeros_like(text_m), tv, text_m > 0, ovl, bm, train, drop_hook)
    zero = seq.sum() * 0.0
    out = {"sequence_output": seq, "mlm_logits": None, "mvrc_logits": None}
    l_wvc = l_aux = l_mvrc = zero
    if sw.with_mlm_loss:
        logits = O.mlm_head(p, text_out)
        out["mlm_logits"] = logits
        V = logits.shape[-1]
        if sw.mlm_norm_in_batch_first:
            l_wvc = norm_first_ce(logits[:B], labels[:B])
            l_aux = norm_first_ce(logits[B:], labels[B:]) if Ba else zero
        else:
            l_wvc = F.cross_entropy(logits[:B].reshape(-1, V), labels[:B].reshape(-1), ignore_index=-1)
            l_aux = F.cross_entropy(logits[B:].reshape(-1, V), labels[B:].reshape(-1), ignore_index=-1) if Ba else zero
    if sw.with_mvrc_loss:
        logits = O.mvrc_head(p, obj_out)[:B]
        out["mvrc_logits"] = logits
        C = logits.shape[-1]
        if sw.mvrc_norm_in_batch_first:
            l_mvrc = norm_first_soft_ce(logits, mvrc_labels)
        else:
            l_mvrc = O.soft_cross_entropy(logits.reshape(-1, C), mvrc_labels.reshape(-1, C)) + zero
    out.update(mlm_loss=l_wvc, mlm_loss_wvc=l_wvc, mlm_loss_aux=l_aux, mvrc_loss=l_mvrc)
    return out, l_wvc + l_aux + l_mvrc


def loss_and_grads(p, cfg, batch, sw, train=False, drop_hook=None):
    """-> (outputs, loss, {name: grad}, global gradient norm), as O.loss_and_grads."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    outputs, loss = forward(leaves, cfg, batch, sw, train=train, drop_hook=drop_hook)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).item()
    return outputs, loss.detach(), grads, norm
