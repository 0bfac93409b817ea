"""Base of the fine-tuning `ResNetVLBERT` mirrors (the part of common/module.py:8-33): the constructor's shared run -- FastRCNN mirror,
object word embedding, VisualLinguisticBert mirror, dropout seed, heads, init_weight, in the reference's registration order -- the
train / inference dispatch, and the builders and input plumbing more than one task uses."""
import sys

import torch
import torch.nn as nn

from .. import ops
from . import language_pretrained as _lp
from .fast_rcnn import FastRCNN
from .heads import cfg_get
from .visual_linguistic_bert import VisualLinguisticBert, check_fp32_ends, fp32_flags


class Module(nn.Module):
    SEED = None                      # base of the per-rank dropout seed (ops.rank_seed)
    NUM_OBJECT_WORDS = 1             # rows of object_linguistic_embeddings
    FP32_ENDS = False                # whether the task's route is built with an fp32 front and back end (`fp32_ends`)

    def __init__(self, config, device=None):
        super().__init__()
        self.config = config
        net = cfg_get(config, "NETWORK")
        vl = cfg_get(net, "VLBERT")
        self._check_config(net, vl)
        # `fp32_ends` (config key of the VLBERT node / VLB_FP32_ENDS=1): fp32 region projection, embedding, classifier and loss around
        # the fp32 encoder -- checked before anything touches the device
        self.fp32_encoder, self.fp32_ends = fp32_flags(vl)
        check_fp32_ends(self.fp32_ends, self.fp32_encoder, with_pooler=bool(cfg_get(vl, "with_pooler", False)))
        if self.fp32_ends and not self.FP32_ENDS:
            raise NotImplementedError("fp32_ends is built for the VQA fine-tuning route only, not for %s.%s"
                                      % (type(self).__module__.split(".")[-1], type(self).__name__))
        if self.fp32_ends and not cfg_get(net, "IMAGE_FEAT_PRECOMPUTED", False):
            raise NotImplementedError("fp32_ends: the image branch (CNN, ROIAlign) is not built in fp32; use IMAGE_FEAT_PRECOMPUTED")
        if not torch.cuda.is_available():
            raise RuntimeError("ResNetVLBERT (HIP) needs an MI355X: there is no CPU fallback")
        dev = torch.device(device or ("cuda:%d" % torch.cuda.current_device()))
        self.device_ = dev
        self.H = H = int(cfg_get(vl, "hidden_size"))
        self.cls_drop = float(cfg_get(net, "CLASSIFIER_DROPOUT", 0.1))
        self.image_feature_extractor = FastRCNN(config, average_pool=True, final_dim=cfg_get(net, "IMAGE_FINAL_DIM", 768),
                                                enable_cnn_reg_loss=False, device=dev, **({"fp32_ends": True} if self.fp32_ends else {}))
        self.object_linguistic_embeddings = nn.Embedding(self.NUM_OBJECT_WORDS, H).to(dev)
        self.language_pretrained_model_path = _lp.resolve_path(net)
        if self.language_pretrained_model_path is None:
            print("Warning: no pretrained language model found, training from scratch!!!", file=sys.stderr)   # (the reference prints to stdout; bench.py owns stdout)
        self.vlbert = self._wrap_encoder(VisualLinguisticBert(vl, language_pretrained_model_path=self.language_pretrained_model_path, device=dev))
        self._seed = torch.tensor([ops.rank_seed(self.SEED)], dtype=torch.int32, device=dev)
        self._build_heads(net, vl)
        self.init_weight()

    # -- what a task fills in ------------------------------------------------------------------------
    def _check_config(self, net, vl):
        """the constructor guards; may keep the switches it reads as attributes"""

    def _wrap_encoder(self, vlbert):
        return vlbert

    def _build_heads(self, net, vl):
        """registers final_mlp (and whatever follows it) and builds the HIP heads"""
        raise NotImplementedError

    def fix_params(self):
        pass

    def forward(self, *inputs, **kwargs):
        """common/module.py:19-24"""
        return self.train_forward(*inputs, **kwargs) if self.training else self.inference_forward(*inputs, **kwargs)

    # -- builders --------------------------------------------------------------------------------------
    def _lin(self, o, i):
        m = nn.Module()
        m.register_parameter("weight", nn.Parameter(torch.empty((o, i), device=self.device_)))
        m.register_parameter("bias", nn.Parameter(torch.zeros((o,), device=self.device_)))
        return m

    def _transform(self, layer_norm=False):
        """BertPredictionHeadTransform (dense + GELU + LayerNorm) / VisualLinguisticBertMVRCHeadTransform (dense + GELU)"""
        tr = nn.Module()
        tr.add_module("dense", self._lin(self.H, self.H))
        if layer_norm:
            ln = nn.Module()
            ln.register_parameter("weight", nn.Parameter(torch.ones((self.H,), device=self.device_)))
            ln.register_parameter("bias", nn.Parameter(torch.zeros((self.H,), device=self.device_)))
            tr.add_module("LayerNorm", ln)
        return tr

    # -- object inputs of the tasks whose text carries no object tags (VQA, RefCOCO+) ----------------------
    def _object_inputs(self, image, boxes, im_info, copy_boxes=False):
        """-> (obj_reps [B,R,H], obj_reps || object word embedding [B,R,2H], box_mask [B,R], R = the batch's longest valid run);
        every text token sees obj_reps[:, 0], the whole image"""
        box_mask = boxes[:, :, 0] > -1.5
        max_len = int(box_mask.sum(1).max())                       # (the one host read of the step, as in the reference)
        box_mask, boxes = box_mask[:, :max_len], boxes[:, :max_len]
        reps = self.image_feature_extractor(images=image, boxes=boxes.contiguous() if copy_boxes else boxes, box_mask=box_mask,
                                            im_info=im_info, classes=None, segms=None)["obj_reps"]
        B, R = box_mask.shape
        ling = self.object_linguistic_embeddings.weight[0].expand(B, R, -1)
        return reps, torch.cat((reps, ling), -1), box_mask, max_len
