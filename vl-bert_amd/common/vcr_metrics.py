"""common/metrics/vcr_metrics.py on the device: same class names, display names and constructor arguments; update(outputs) takes
the reference's `outputs` dict and never synchronises."""
import torch

from .. import ops
from .metrics import OutputLossLogger as LossLogger  # noqa: F401
from .metrics import OutputMean, OutputsMetric


def _hard_label(label):
    label = label.detach().reshape(-1)
    return (label if label.dtype == torch.int64 else label.long()).contiguous()


class Accuracy(OutputsMetric):
    """hits / rows with label != -1 (:20-33).  The reference's 1-D branch (`view(-1, 4)`) is not built: the mirror always returns
    [B, C] logits."""
    display = "Acc"

    def update(self, outputs):
        if outputs["label_logits"].dim() == 1:
            raise NotImplementedError("vcr_metrics.Accuracy on 1-D logits (the reference's view(-1, 4) branch): the mirror returns [B, C]")
        logits = self._logits(outputs)
        self._on(logits.device)
        ops.argmax_eval(logits, ops.ARGMAX_HARD, label=_hard_label(outputs["label"]), sum=self.sum_metric, count=self.num_inst)


class AnsLoss(OutputMean):
    display, output_name, optional = "AnsLoss", "ans_loss", False


class CNNRegLoss(OutputMean):
    display, output_name = "CNNRegLoss", "cnn_regularization_loss"


class PositiveFraction(OutputMean):
    display, output_name, optional = "PosFraction", "positive_fraction", False


class JointAccuracy(OutputsMetric):
    """#(answer right and rationale right) / rows, no -1 filter (:69-81).  Reads `answer_pred` / `rationale_pred` (int32, left by
    finetune_eval.joint_validation) when the dict carries them, else takes the two argmaxes itself."""
    display = "JointAcc"

    def _pred(self, outputs, which):
        pred = outputs.get(which + "_pred")
        if pred is None:
            logits = self._logits(outputs, which + "_label_logits")
            pred = torch.empty((logits.shape[0],), dtype=torch.int32, device=logits.device)
            ops.argmax_eval(logits, ops.ARGMAX_PREDICT, pred=pred)
        return pred

    def update(self, outputs):
        pa, pr = self._pred(outputs, "answer"), self._pred(outputs, "rationale")
        self._on(pa.device)
        ops.joint_hits(pa, _hard_label(outputs["answer_label"]), pr, _hard_label(outputs["rationale_label"]), self._acc)

    # sum_metric / num_inst are the two halves of one int64 [2] the kernel adds to
    def reset(self):
        self._acc = torch.zeros((2,), dtype=torch.int64)
        self.sum_metric, self.num_inst = self._acc[0], self._acc[1]

    def _on(self, device):
        if self._acc.device != device:
            self._acc = self._acc.to(device)
            self.sum_metric, self.num_inst = self._acc[0], self._acc[1]
