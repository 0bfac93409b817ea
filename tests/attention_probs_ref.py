"""References for the attention-probability tests (tests/test_attention_probs_gpu.py, tests/test_attention_vis_gpu.py): the float64
restatement of what vlb_attention_probs writes, the dropout keep x scale tensor of the forward, and the oracle's per-layer outputs and
probabilities assembled from oracle/vlbert_oracle.py's public functions.  CPU only; nothing here touches the library."""
import math

import numpy as np
import torch

from oracle import vlbert_oracle as O
from tests import embed_attn_refs as R
from tests.gpu_util import drop_scale, drop_thr, keep_mask


def ceil_to(n, m):
    return (n + m - 1) // m * m


def probs_ref(qkv, mask, B, S, H, nh, use_mask=True):
    """float64 softmax(Q K^T / 8 + (1 - mask) * -10000) [B, nh, S, S] from the (already 16-bit-rounded) qkv [B*S, 3H] -- every query,
    padded ones included.  use_mask=False: the mutant without the additive mask."""
    d = H // nh
    q, k, _ = [t.view(B, S, nh, d).permute(0, 2, 1, 3) for t in qkv.double().view(B, S, 3, H).unbind(2)]
    sc = q @ k.transpose(-1, -2) / math.sqrt(d)
    if use_mask:
        sc = sc + ((1 - mask.double()) * -10000.0)[:, None, None, :]
    return torch.softmax(sc, -1)


def keep_scale(seed, tag, B, nh, S, p):
    """float64 [B, nh, S, S]: keep mask x 1 / (1 - p_eff) the forward applies under (seed, tag) at element ((b*nh + h)*S + q)*S + k."""
    thr = drop_thr(p)
    keep = keep_mask(seed, tag, R.attn_drop_index(B, nh, S), thr).reshape(B, nh, S, S)
    return torch.from_numpy(keep.astype(np.float64)) * drop_scale(thr)


def oracle_core_inputs(p, cfg, batch):
    """The six VisualLinguisticBert arguments of a pre-training batch (boxes, im_info, text, ..., mvrc_ops, ...) in eval mode, as
    pretrain_forward builds them: masked features and words overwritten, every text token sees the whole-image box."""
    boxes, im_info, text, _, _, mvrc_ops, _ = batch[:7]
    boxes = boxes.clone()
    box_mask = boxes[:, :, 0] > -1.5
    max_len = int(box_mask.sum(1).max())
    box_mask, boxes, mvrc_ops = box_mask[:, :max_len], boxes[:, :max_len], mvrc_ops[:, :max_len]
    feats = boxes[:, :, 4:].clone()
    feats[mvrc_ops == 1] = p["object_mask_visual_embedding.weight"][0]
    boxes = torch.cat((boxes[:, :, :4], feats), -1)
    obj_reps = O.fast_rcnn_precomputed(p, cfg, boxes, box_mask, im_info, False)
    text_visual = obj_reps[:, 0:1].expand(-1, text.shape[1], -1)
    B, Rm = box_mask.shape
    ling = p["object_linguistic_embeddings.weight"][0].expand(B, Rm, -1).clone()
    ling[mvrc_ops == 1] = p["object_mask_word_embedding.weight"][0]
    return text, torch.zeros_like(text), text_visual, text > 0, torch.cat((obj_reps, ling), -1), box_mask


def oracle_layers_and_probs(p, cfg, core_inputs):
    """-> ([x_1 .. x_L] each [B, n, H], [P_0 .. P_{L-1}] each [B, nh, n, n]) in fp32, eval mode: O.vl_embedding, then O.bert_layer per
    layer; layer l's probabilities from its input x_l with the layer's own query / key weights."""
    with torch.no_grad():
        emb, mask, _, _ = O.vl_embedding(p, cfg, *core_inputs, False)
        ext = (1.0 - mask.to(emb.dtype)).unsqueeze(1).unsqueeze(2) * -10000.0
        B, n, H = emb.shape
        nh = cfg.num_attention_heads
        d = H // nh

        def heads(t):
            return t.view(B, n, nh, d).permute(0, 2, 1, 3)

        x, layers, probs = emb, [], []
        for l in range(cfg.num_hidden_layers):
            pre = "vlbert.encoder.layer.%d." % l
            q, k = heads(O.linear(x, p, pre + "attention.self.query")), heads(O.linear(x, p, pre + "attention.self.key"))
            probs.append(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d) + ext, -1))
            x = O.bert_layer(p, cfg, pre, x, ext, False)
            layers.append(x)
    return layers, probs, mask
