from .resnet_vlbert_for_pretraining import ResNetVLBERTForPretraining, ResNetVLBERTForPretrainingMultitask  # noqa: F401
from .resnet_vlbert_for_attention_vis import ResNetVLBERTForAttentionVis  # noqa: F401
