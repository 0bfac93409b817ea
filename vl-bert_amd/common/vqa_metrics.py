"""common/metrics/vqa_metrics.py on the device: same class names, display names and constructor arguments; update(outputs) takes
the reference's `outputs` dict (`label_logits` fp32 [B, answers], `label` soft scores [B, answers]) and never synchronises."""
import torch

from .. import ops
from .metrics import OutputLossLogger as LossLogger  # noqa: F401
from .metrics import OutputsMetric


class SoftAccuracy(OutputsMetric):
    """sum += label[b, argmax(logits[b])] over the batch / rows (:20-31).  The sum is a float64 on the device, added in row order
    (vlb_argmax_eval mode 2), where the reference adds the fp32 `.sum()` of every batch to an fp32 scalar."""
    display = "SoftAcc"
    _sum_dtype = torch.float64

    def update(self, outputs):
        logits = self._logits(outputs)
        self._on(logits.device)
        rows = logits.shape[0]
        if getattr(self, "_score", None) is None or self._score.numel() < rows or self._score.device != logits.device:
            self._score = torch.empty((rows,), dtype=torch.float32, device=logits.device)       # scratch of the ordered sum
        ops.argmax_eval(logits, ops.ARGMAX_GATHER, label=self._soft_label(outputs["label"]), score=self._score,
                        sum=self.sum_metric, count=self.num_inst)
