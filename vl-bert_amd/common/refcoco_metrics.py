"""common/metrics/refcoco_metrics.py on the device: same class names, display names and constructor arguments; update(outputs)
takes the reference's `outputs` dict (`label_logits` fp32 [B, boxes], `label` 0 / 1 per box, -1 padding) and never synchronises."""
import torch

from .. import ops
from .metrics import OutputLossLogger as LossLogger  # noqa: F401
from .metrics import OutputsMetric


class RefAccuracy(OutputsMetric):
    """#(label[b, argmax(logits[b])] > 0.5) / rows (:20-31)"""
    display = "RefAcc"

    def update(self, outputs):
        logits = self._logits(outputs)
        self._on(logits.device)
        ops.argmax_eval(logits, ops.ARGMAX_GATHER_GT, label=self._soft_label(outputs["label"]), sum=self.sum_metric, count=self.num_inst)


class _Cls(OutputsMetric):
    """One pass of vlb_binary_cls_eval into the metric's own int64 [4] = [correct among valid, valid, correct among positive,
    positive]; sum_metric / num_inst are views of the two entries the class reports (:34-72)."""
    num, den = None, None

    def reset(self):
        self._acc = torch.zeros((4,), dtype=torch.int64)
        self.sum_metric, self.num_inst = self._acc[self.num], self._acc[self.den]

    def _on(self, device):
        if self._acc.device != device:
            self._acc = self._acc.to(device)
            self.sum_metric, self.num_inst = self._acc[self.num], self._acc[self.den]

    def update(self, outputs):
        logits = self._logits(outputs)
        self._on(logits.device)
        ops.binary_cls_eval(logits, self._soft_label(outputs["label"]), self._acc)


class ClsAccuracy(_Cls):
    display, num, den = "ClsAcc", 0, 1


class ClsPosAccuracy(_Cls):
    display, num, den = "ClsPosAcc", 2, 3


class ClsPosFraction(_Cls):
    display, num, den = "ClsPosFrac", 3, 1
