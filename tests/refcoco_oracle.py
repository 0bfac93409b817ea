"""CPU restatement of the RefCOCO+ fine-tuning wrapper (refcoco/modules/resnet_vlbert_for_refcoco.py:71-227) on precomputed region
features, on top of oracle/vlbert_oracle.py.  Test infrastructure only; pinned by tests/golden/refcoco/refcoco_small.npz, which
tools/make_refcoco_golden.py produces from the reference's own module.

  boxes trimmed to max_len = the longest valid run (:80-86) -> obj_reps -> text [CLS] expression [SEP], token types 0, every token
  sees obj_reps[:, 0] (:96-107) -> object linguistic embedding row 0 -> vlbert_forward's object output (zero at padded rows) ->
  final_mlp = dense -> erf-GELU (no LayerNorm) -> Dropout -> Linear(H, 1) on EVERY row -> BCE over the valid boxes (:132-135) ->
  logits padded back to origin_len with -10000; inference: argmax over all origin_len columns -> box / (w_ratio, h_ratio) (:206-222).
"""
import torch
import torch.nn.functional as F

from oracle import vlbert_oracle as O

CLS, SEP = 101, 102


def prepare_text(expression):
    B = expression.shape[0]
    ids = expression.new_zeros((B, expression.shape[1] + 2))
    ids[:, 0] = CLS
    ids[:, 1:-1] = expression
    ids[torch.arange(B), (ids > 0).sum(1)] = SEP
    return ids, ids.new_zeros(ids.shape), ids > 0


def final_mlp(p, x, train=False, drop_p=0.0):
    h = O.gelu(O.linear(x, p, "final_mlp.0.dense"))
    h = F.dropout(h, drop_p, True) if (train and drop_p > 0) else h
    return O.linear(h, p, "final_mlp.2")


def refcoco_forward(p, cfg, boxes, im_info, expression, label=None, classifier_dropout=0.0, train=False):
    """-> (outputs, loss): train_forward when `label` is given, else inference_forward (loss None, outputs carry pred_boxes)."""
    box_mask = boxes[:, :, 0] > -1.5
    max_len, origin_len = int(box_mask.sum(1).max()), boxes.shape[1]
    box_mask, tb = box_mask[:, :max_len], boxes[:, :max_len]
    obj_reps = O.fast_rcnn_precomputed(p, cfg, tb, box_mask, im_info, train)
    ids, types, text_mask = prepare_text(expression)
    text_visual = obj_reps[:, 0:1].expand(-1, ids.shape[1], -1)
    B, R = box_mask.shape
    obj_vl = torch.cat((obj_reps, p["object_linguistic_embeddings.weight"][0].expand(B, R, -1)), -1)
    _, obj_out, _, _ = O.vlbert_forward(p, cfg, ids, types, text_visual, text_mask, obj_vl, box_mask, train)
    logits = final_mlp(p, obj_out, train, classifier_dropout).squeeze(-1)
    full = logits.new_full((B, origin_len), -10000.0)
    full[:, :max_len] = logits
    out = {"label_logits": full}
    if label is None:
        idx = full.argmax(1)
        pred = tb[torch.arange(B), idx, :4].clone()
        pred[:, [0, 2]] /= im_info[:, 2:3]
        pred[:, [1, 3]] /= im_info[:, 3:4]
        out.update(pred_boxes=pred, pred_index=idx)
        return out, None
    lab = label[:, :max_len].float()
    loss = F.binary_cross_entropy_with_logits(logits[box_mask], lab[box_mask])
    out.update(cls_loss=loss)
    return out, loss


def init_refcoco_params(cfg, seed):
    """vlbert_oracle.init_params without the pre-training heads / mask embeddings + final_mlp.0.dense [H, H] and final_mlp.2 [1, H]."""
    base = O.init_params(cfg, seed=seed)
    p = {k: v for k, v in base.items() if "mlm_head" not in k and "mvrc_head" not in k and "object_mask_" not in k
         and "relationsip_head" not in k and "aux_text_visual" not in k}
    g = torch.Generator().manual_seed(seed + 211)
    H = cfg.hidden_size
    for name, o in (("final_mlp.0.dense", H), ("final_mlp.2", 1)):
        p[name + ".weight"] = torch.randn(o, H, generator=g) * (2.0 / (o + H)) ** 0.5
        p[name + ".bias"] = 0.05 * torch.randn(o, generator=g)
    return p


def small_config():
    return O.VLBertConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, vocab_size=512,
                          max_position_embeddings=64, visual_region_classes=50, hidden_dropout_prob=0.0,
                          attention_probs_dropout_prob=0.0, obj_downsample_dropout=0.0)
