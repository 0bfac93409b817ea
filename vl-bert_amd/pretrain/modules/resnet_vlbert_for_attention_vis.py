"""Drop-in `ResNetVLBERTForAttentionVis` (pretrain/modules/resnet_vlbert_for_attention_vis.py:14-197), the module behind
cfgs/pretrain/vis_attention_maps_coco.yaml and pretrain/vis_attention_maps.py: same constructor argument (the config tree of
pretrain/function/config.py), same `forward(image, boxes, im_info, text, relationship_label, mlm_labels, mvrc_ops, mvrc_labels, *aux)
-> {'attention_probs': [B, layers, heads, n, n], 'hidden_states': [B, layers, n, H]}` (fp32, n = the batch's longest packed sequence),
same parameter names, so the reference's checkpoints load unchanged.

Composition, as in the reference: boxes trimmed to the batch's longest valid run (:122-128) -> precomputed features of masked regions
overwritten by `object_mask_visual_embedding` (:130-133) -> FastRCNN mirror -> every text token sees obj_reps[:, 0] (:150-152) ->
object word embedding, masked regions overwritten by `object_mask_word_embedding` under WITH_MVRC_LOSS (:154-159) -> text-only
auxiliary samples appended with `aux_text_visual_embedding` as their visual half (:161-178) -> VisualLinguisticBert mirror with
`inspect_fused=True`: the fused 16-bit forward the model is trained and deployed with, every layer's output from its X buffers and
every layer's attention probabilities recomputed from the saved QKV and lse (csrc/attention_probs.hip), up to 512 positions.
Forward only: the outputs carry no autograd history.  What the building blocks refuse (IMAGE_SEMANTIC, `mask_visual_embed` on the
image branch -- MASK_RAW_PIXELS false there --, visual_size != hidden_size, frozen embeddings) raises their NotImplementedError.
"""
import sys

import torch
import torch.nn as nn

from ...common import language_pretrained as _lp
from ...common.fast_rcnn import FastRCNN
from ...common.heads import cfg_get as _get
from ...common.visual_linguistic_bert import VisualLinguisticBert


def parameter_names(config):
    """The parameter names of ResNetVLBERTForAttentionVis(config) -- the reference module's state-dict keys -- without building the
    module (no GPU needed): what a checkpoint must name to fill it."""
    from ... import engine as _engine
    from ...common.checkpoint import reference_vision_param_names
    net = _get(config, "NETWORK")
    vl = _get(net, "VLBERT")
    precomputed = bool(_get(net, "IMAGE_FEAT_PRECOMPUTED", False))
    pre = "image_feature_extractor."
    if precomputed:
        names = [pre + "obj_downsample.1.weight", pre + "obj_downsample.1.bias"]
    else:
        names = [pre + n for n in reference_vision_param_names(int(_get(net, "IMAGE_NUM_LAYERS", 101)))]
    names.append("object_linguistic_embeddings.weight")
    if precomputed or not _get(net, "MASK_RAW_PIXELS", True):
        names.append("object_mask_visual_embedding.weight")
    if _get(net, "WITH_MVRC_LOSS", True):
        names.append("object_mask_word_embedding.weight")
    names.append("aux_text_visual_embedding.weight")
    mc = _engine.ModelConfig(hidden_size=_get(vl, "hidden_size"), num_hidden_layers=_get(vl, "num_hidden_layers"),
                             num_attention_heads=_get(vl, "num_attention_heads"), intermediate_size=_get(vl, "intermediate_size"),
                             with_pooler=bool(_get(vl, "with_pooler", False)))
    heads = ("vlbert.mlm_head.", "vlbert.mvrc_head.", "vlbert.relationsip_head.")
    names += [n for n in _engine.param_layout(mc) if n.startswith("vlbert.") and not n.startswith(heads)]
    return names


class ResNetVLBERTForAttentionVis(nn.Module):
    def __init__(self, config, device=None):
        super().__init__()
        self.config = config
        net = _get(config, "NETWORK")
        vl = _get(net, "VLBERT")
        if not torch.cuda.is_available():
            raise RuntimeError("ResNetVLBERTForAttentionVis (HIP) needs an MI355X: there is no CPU fallback")
        dev = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
        self.device_ = dev
        H = int(_get(vl, "hidden_size"))
        self.precomputed = bool(_get(net, "IMAGE_FEAT_PRECOMPUTED", False))
        self.mask_raw_pixels = bool(_get(net, "MASK_RAW_PIXELS", True))
        self.with_mvrc = bool(_get(net, "WITH_MVRC_LOSS", True))
        self.initializer_range = float(_get(vl, "initializer_range", 0.02))
        self.image_feature_extractor = FastRCNN(config, average_pool=True, final_dim=_get(net, "IMAGE_FINAL_DIM", 768),
                                                enable_cnn_reg_loss=False, device=dev)
        self.object_linguistic_embeddings = nn.Embedding(1, H).to(dev)
        if self.precomputed or not self.mask_raw_pixels:
            self.object_mask_visual_embedding = nn.Embedding(1, 2048).to(dev)
        if self.with_mvrc:
            self.object_mask_word_embedding = nn.Embedding(1, H).to(dev)
        self.aux_text_visual_embedding = nn.Embedding(1, H).to(dev)
        path = _lp.resolve_path(net)
        if path is None:
            print("Warning: no pretrained language model found, training from scratch!!!", file=sys.stderr)
        self.vlbert = VisualLinguisticBert(vl, language_pretrained_model_path=None if _get(vl, "from_scratch", False) else path,
                                           device=dev, inspect_fused=True)
        self.init_weight()

    def init_weight(self):
        """:53-62"""
        with torch.no_grad():
            if self.precomputed or not self.mask_raw_pixels:
                self.object_mask_visual_embedding.weight.zero_()
            if self.with_mvrc:
                self.object_mask_word_embedding.weight.normal_(0.0, self.initializer_range)
            self.aux_text_visual_embedding.weight.normal_(0.0, self.initializer_range)
            self.image_feature_extractor.init_weight()
            self.object_linguistic_embeddings.weight.normal_(0.0, self.initializer_range)

    def fix_params(self):
        pass

    def train(self, mode=True):
        super().train(mode)
        self.image_feature_extractor.bn_eval()            # frozen BatchNorm (:64-68); the HIP vision stack folds it anyway
        return self

    def load_state_dict(self, state_dict, strict=True):
        """the FastRCNN mirror converts its convolution layout and drops the reference's `head.0.*` alias keys in its own
        load_state_dict, which nn.Module's recursion does not call for sub-modules: hand it its slice directly, load the rest here"""
        pre = "image_feature_extractor."
        self.image_feature_extractor.load_state_dict({k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}, strict=strict)
        rest = {k: v for k, v in state_dict.items() if not k.startswith(pre)}
        res = super().load_state_dict(rest, strict=False)
        missing = [k for k in res.missing_keys if not k.startswith(pre)]
        if strict and (missing or res.unexpected_keys):
            raise RuntimeError("Error(s) in loading state_dict for ResNetVLBERTForAttentionVis: missing %s, unexpected %s"
                               % (missing, res.unexpected_keys))
        return res

    @torch.no_grad()
    def embeddings(self, image, boxes, im_info, text, mvrc_ops, *aux):
        """The six arguments of VisualLinguisticBert.forward for this batch (:103-178)."""
        aux_texts = aux[0::2]
        Ba = sum(t.shape[0] for t in aux_texts)
        Ta = max([t.shape[1] for t in aux_texts]) if len(aux_texts) > 0 else 0
        aux_text = text.new_zeros((Ba, Ta))
        cur = 0
        for t in aux_texts:                                       # the corpora concatenated, right-padded (:111-116)
            aux_text[cur:cur + t.shape[0], :t.shape[1]] = t
            cur += t.shape[0]
        box_mask = boxes[:, :, 0] > -1.5
        max_len = int(box_mask.sum(1).max())                       # (the one host read in front of the encoder, as in the reference)
        box_mask, boxes, mvrc_ops = box_mask[:, :max_len], boxes[:, :max_len].clone(), mvrc_ops[:, :max_len]
        if self.precomputed:                                       # data movement only (:130-133)
            feats = boxes[:, :, 4:]
            feats[mvrc_ops == 1] = self.object_mask_visual_embedding.weight[0].to(feats.dtype)
        mve = self.object_mask_visual_embedding.weight[0] if (not self.precomputed and not self.mask_raw_pixels) else None
        obj_reps = self.image_feature_extractor(images=image, boxes=boxes, box_mask=box_mask, im_info=im_info, classes=None, segms=None,
                                                mvrc_ops=mvrc_ops, mask_visual_embed=mve)["obj_reps"]
        B, T = text.shape
        R, H = obj_reps.shape[1], obj_reps.shape[2]
        ling = self.object_linguistic_embeddings.weight[0].expand(B, R, H).clone()
        if self.with_mvrc:
            ling[mvrc_ops == 1] = self.object_mask_word_embedding.weight[0]
        Bt, Tm = B + Ba, max(T, Ta)
        ids = text.new_zeros((Bt, Tm))
        ids[:B, :T] = text
        ids[B:, :Ta] = aux_text
        text_vis = obj_reps.new_zeros((Bt, Tm, H))
        text_vis[:B, :T] = obj_reps[:, 0:1]                        # text tags are all 0: every token sees the whole-image box
        text_vis[B:] = self.aux_text_visual_embedding.weight[0]
        obj_vl = obj_reps.new_zeros((Bt, R, 2 * H))
        obj_vl[:B] = torch.cat((obj_reps, ling), -1)
        mask = box_mask.new_zeros((Bt, R))
        mask[:B] = box_mask
        return ids, ids.new_zeros(ids.shape), text_vis, ids > 0, obj_vl, mask

    @torch.no_grad()
    def forward(self, image, boxes, im_info, text, relationship_label, mlm_labels, mvrc_ops, mvrc_labels, *aux):
        if len(aux) % 2:
            raise ValueError("aux must be (text, mlm_labels) pairs")
        layers, _, probs = self.vlbert(*self.embeddings(image, boxes, im_info, text, mvrc_ops, *aux),
                                       output_all_encoded_layers=True, output_attention_probs=True)
        return {"attention_probs": torch.stack(probs, 0).transpose(0, 1).contiguous(),
                "hidden_states": torch.stack(layers, 0).transpose(0, 1).contiguous()}
