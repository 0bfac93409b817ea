"""Pre-training metrics, validation and the validation monitor over the engine's device counters.

The reference computes its metrics on the host from the logits of every batch (common/metrics/pretrain_metrics.py:20-85: an
argmax over [rows, 30522] per metric, then `.item()`).  Here `PretrainEngine.eval_step()` leaves [hits, counted rows] per head in
`engine.metric_acc` (csrc/metrics.hip) and the mean losses in `engine.losses`; the classes below keep the reference's `EvalMetric`
contract (common/metrics/eval_metric.py:5-68: update / reset / get / get_name_value, display names, nan for an empty metric,
sum-then-divide all-reduce) and its `CompositeEvalMetric` (composite_eval_metric.py), but `update()` takes the counters instead of
an outputs dict:

    metrics = pretrain_metrics(with_rel_loss=..., multitask=..., allreduce=args.dist)
    do_validation(engine, val_loader, metrics)        # reset; per batch: set_batch, eval_step, metrics.update(engine)
    names, values = metrics.get()

`update(source)` works on anything with `metric_acc` (int64 [4, 2], rows = PretrainEngine.METRIC_ROWS), `losses` (fp32 [4]) and
`reset_metrics()` -- CPU tensors included, so the module is usable (and tested) without a GPU.  It MOVES the counters: they are
added to the metric's own tensors on the source's device and zeroed, with no host synchronisation; `get()` synchronises.
"""
import logging

import torch

ROW_MLM, ROW_MLM_AUX, ROW_MVRC, ROW_REL = 0, 1, 2, 3                    # rows of metric_acc (PretrainEngine.METRIC_ROWS)
SLOT_MLM, SLOT_MVRC, SLOT_MLM_AUX, SLOT_REL = 0, 1, 2, 3                # slots of engine.losses
# TRAIN.LOSS_LOGGERS of pretrain/function/config.py:159 and of the shipped multitask YAMLs
DEFAULT_LOSS_LOGGERS = (("relationship_loss", "RelLoss"), ("mlm_loss", "MLMLoss"), ("mvrc_loss", "MVRCLoss"))


def loss_slots(multitask):
    """Output name of the reference module's `outputs` dict -> slot of engine.losses (resnet_vlbert_for_pretraining.py:202-212,
    resnet_vlbert_for_pretraining_multitask.py:273-286).  A LossLogger whose name the module does not output adds nothing."""
    if multitask:
        return {"relationship_loss": SLOT_REL, "mlm_loss_wvc": SLOT_MLM, "mlm_loss_aux": SLOT_MLM_AUX, "mvrc_loss": SLOT_MVRC}
    return {"relationship_loss": SLOT_REL, "mlm_loss": SLOT_MLM, "mvrc_loss": SLOT_MVRC}


class EvalMetric(object):
    """sum_metric / num_inst -> (name, value); value = nan while num_inst == 0.  allreduce: numerator and denominator are summed over
    the process group BEFORE the division (eval_metric.py:44-56) -- every rank must call get()."""

    def __init__(self, name, allreduce=False, num_replicas=1, group=None):
        self.name = str(name)
        self.allreduce, self.num_replicas, self.group = allreduce, num_replicas, group
        self.reset()

    def __str__(self):
        return "EvalMetric: {}".format(dict(self.get_name_value()))

    def update(self, source):
        raise NotImplementedError()

    def reset(self):
        self.num_inst = torch.zeros((), dtype=torch.int64)
        self.sum_metric = torch.zeros((), dtype=self._sum_dtype)

    _sum_dtype = torch.int64

    def _add(self, num, den):
        if self.sum_metric.device != num.device:
            self.sum_metric, self.num_inst = self.sum_metric.to(num.device), self.num_inst.to(num.device)
        self.sum_metric += num
        self.num_inst += den

    def get(self):
        num, den = self.sum_metric, self.num_inst
        if self.allreduce:
            import torch.distributed as dist
            num, den = num.clone(), den.clone()
            dist.all_reduce(num, op=dist.ReduceOp.SUM, group=self.group)
            dist.all_reduce(den, op=dist.ReduceOp.SUM, group=self.group)
        if int(den.item()) == 0:
            return (self.name, float("nan"))
        return (self.name, (num.to(torch.float32) / den.to(torch.float32)).item())      # (the reference divides fp32 tensors)

    def get_name_value(self):
        name, value = self.get()
        if not isinstance(name, list):
            name = [name]
        if not isinstance(value, list):
            value = [value]
        return list(zip(name, value))


class _CounterAccuracy(EvalMetric):
    row, display = None, None

    def __init__(self, allreduce=False, num_replicas=1, group=None):
        super(_CounterAccuracy, self).__init__(self.display, allreduce, num_replicas, group)

    def update(self, source):
        acc = source.metric_acc if hasattr(source, "metric_acc") else source
        self._add(acc[self.row, 0], acc[self.row, 1])


class RelationshipAccuracy(_CounterAccuracy):
    row, display = ROW_REL, "RelAcc"


class MLMAccuracy(_CounterAccuracy):
    row, display = ROW_MLM, "MLMAcc"


class MLMAccuracyWVC(_CounterAccuracy):
    row, display = ROW_MLM, "MLMAccWVC"


class MLMAccuracyAUX(_CounterAccuracy):
    row, display = ROW_MLM_AUX, "MLMAccAUX"


class MVRCAccuracy(_CounterAccuracy):
    row, display = ROW_MVRC, "MVRCAccuracy"


class LossLogger(EvalMetric):
    """Sum of the per-batch mean losses / number of batches (pretrain_metrics.py:5-17); slot = index into the source's `losses`, None
    for an output the module does not produce (the batch is counted, nothing is added)."""
    _sum_dtype = torch.float32

    def __init__(self, output_name, display_name=None, allreduce=False, num_replicas=1, group=None, slot=None):
        self.output_name, self.slot = output_name, slot
        super(LossLogger, self).__init__(output_name if display_name is None else display_name, allreduce, num_replicas, group)

    def update(self, source):
        losses = source.losses
        one = torch.ones((), dtype=torch.int64, device=losses.device)
        self._add(losses[self.slot] if self.slot is not None else torch.zeros((), dtype=torch.float32, device=losses.device), one)


class OutputsMetric(EvalMetric):
    """Base of the fine-tuning metrics (common/{vqa,vcr,refcoco}_metrics.py): update(outputs) takes the reference's `outputs` dict and
    launches a kernel of csrc/finetune_metrics.hip straight into sum_metric / num_inst, which move to the logits' device at the first
    update and stay there -- no host synchronisation before get().  CPU tensors raise (ops._p): there is no CPU path."""

    def __init__(self, allreduce=False, num_replicas=1, group=None):
        super(OutputsMetric, self).__init__(self.display, allreduce, num_replicas, group)

    display = None

    def _on(self, device):
        if self.sum_metric.device != device:
            self.sum_metric, self.num_inst = self.sum_metric.to(device), self.num_inst.to(device)

    @staticmethod
    def _logits(outputs, key="label_logits"):
        x = outputs[key].detach()
        if not x.is_cuda:
            raise RuntimeError("fine-tuning metrics need GPU tensors (got %s); there is no CPU path" % x.device)
        if x.dtype != torch.float32:
            x = x.float()
        return x if (x.dim() != 2 or x.stride(1) == 1) else x.contiguous()

    @staticmethod
    def _soft_label(label):
        label = label.detach()
        if label.dtype != torch.float32:
            label = label.float()
        return label if label.stride(1) == 1 else label.contiguous()


class OutputMean(OutputsMetric):
    """sum += outputs[name].mean() on the device (fp32, torch ops), num_inst += 1: the reference's LossLogger / AnsLoss / CNNRegLoss /
    PositiveFraction.  optional: a name the module does not output still counts the batch."""
    _sum_dtype = torch.float32
    output_name, optional = None, True

    def update(self, outputs):
        if self.output_name in outputs or not self.optional:
            v = outputs[self.output_name].detach()
            if not v.is_cuda:
                raise RuntimeError("fine-tuning metrics need GPU tensors (got %s); there is no CPU path" % v.device)
            self._on(v.device)
            self.sum_metric += v.float().mean()
        self.num_inst += 1


class OutputLossLogger(OutputMean):
    """LossLogger(output_name, display_name) of the three fine-tuning metric modules."""

    def __init__(self, output_name, display_name=None, allreduce=False, num_replicas=1, group=None):
        self.output_name = output_name
        self.display = output_name if display_name is None else display_name
        super(OutputLossLogger, self).__init__(allreduce, num_replicas, group)


class CompositeEvalMetric(EvalMetric):
    """The reference's composite (composite_eval_metric.py:5-69); update(source) feeds every child from the source's counters and
    losses, then zeroes the source's counters (they have been moved into the metrics)."""

    def __init__(self, metrics=None, name="composite"):
        self.metrics = [] if metrics is None else metrics
        super(CompositeEvalMetric, self).__init__(name)

    def add(self, metric):
        self.metrics.append(metric)

    def get_metric(self, index):
        return self.metrics[index]

    def update(self, source):
        for metric in self.metrics:
            metric.update(source)
        if hasattr(source, "reset_metrics"):              # (an `outputs` dict of the fine-tuning metrics carries no counters to clear)
            source.reset_metrics()

    def reset(self):
        for metric in self.metrics:
            metric.reset()

    def get(self):
        names, values = [], []
        for metric in self.metrics:
            name, value = metric.get()
            names.append(name)
            values.append(value)
        return names, values


def pretrain_metrics(with_rel_loss=False, with_mlm_loss=True, with_mvrc_loss=True, multitask=False, loss_loggers=None,
                     allreduce=False, num_replicas=1, group=None):
    """The validation metric list of pretrain/function/train.py:244-273 in its order: relationship first (WITH_REL_LOSS), MLM
    (MLMAccWVC + MLMAccAUX for the multitask module), MVRC, then one LossLogger per (output name, display name)."""
    kw = dict(allreduce=allreduce, num_replicas=num_replicas, group=group)
    out = CompositeEvalMetric()
    if with_rel_loss:
        out.add(RelationshipAccuracy(**kw))
    if with_mlm_loss:
        if multitask:
            out.add(MLMAccuracyWVC(**kw))
            out.add(MLMAccuracyAUX(**kw))
        else:
            out.add(MLMAccuracy(**kw))
    if with_mvrc_loss:
        out.add(MVRCAccuracy(**kw))
    slots = loss_slots(multitask)
    for output_name, display_name in (DEFAULT_LOSS_LOGGERS if loss_loggers is None else loss_loggers):
        out.add(LossLogger(output_name, display_name=display_name, slot=slots.get(output_name), **kw))
    return out


def parse_loss_loggers(value):
    """TRAIN.LOSS_LOGGERS as the YAMLs write it ("name,Display" strings, pretrain/function/config.py:192-193) or as pairs."""
    if value is None:
        return None
    return [tuple(str(s) for s in (v.split(",") if isinstance(v, str) else v)) for v in value]


def host_metric_name(multitask):
    return "MLMAccWVC" if multitask else "MLMAcc"          # pretrain/function/train.py:279


@torch.no_grad()
def do_validation(engine, val_loader, metrics, load_batch=None):
    """pretrain/function/val.py:6-13 on the engine: reset, then per batch set_batch -> eval_step -> metrics.update.  load_batch(batch)
    puts one item of val_loader into the engine's static buffers (default: engine.set_batch(*batch))."""
    metrics.reset()
    engine.reset_metrics()
    for batch in val_loader:
        if load_batch is not None:
            load_batch(batch)
        else:
            engine.set_batch(*batch)
        engine.eval_step()
        metrics.update(engine)


class ValidationMonitor(object):
    """common/callbacks/epoch_end_callbacks/validation_monitor.py:5-46: runs val_func at an epoch's end, keeps best_epoch / best_val of
    the host metric (strictly greater wins) and prints the reference's lines."""

    def __init__(self, val_func, val_loader, metrics, host_metric_name="Acc", load_batch=None, verbose=True, label_index_in_batch=None):
        # label_index_in_batch: the reference's name of the fourth argument of the fine-tuning val_func (common/finetune_eval.py)
        assert load_batch is None or label_index_in_batch is None
        self.val_func, self.val_loader, self.metrics = val_func, val_loader, metrics
        self.load_batch = label_index_in_batch if load_batch is None else load_batch
        self.host_metric_name = host_metric_name
        self.best_epoch = -1
        self.best_val = -1.0
        self.verbose = verbose

    def state_dict(self):
        return {"best_epoch": self.best_epoch, "best_val": self.best_val}

    def load_state_dict(self, state_dict):
        assert "best_epoch" in state_dict, "miss key 'best_epoch'"
        assert "best_val" in state_dict, "miss key 'best_val'"
        self.best_epoch = state_dict["best_epoch"]
        self.best_val = state_dict["best_val"]

    def _say(self, s):
        logging.info(s)
        if self.verbose:
            print(s, flush=True)

    def __call__(self, epoch_num, net, optimizer=None, writer=None):
        self.val_func(net, self.val_loader, self.metrics, self.load_batch)
        name, value = self.metrics.get()
        s = "Epoch[%d] \tVal-" % (epoch_num)
        for n, v in zip(name, value):
            if n == self.host_metric_name and v > self.best_val:
                self.best_epoch = epoch_num
                self.best_val = v
                self._say("New Best Val {}: {}, Epoch: {}".format(self.host_metric_name, self.best_val, self.best_epoch))
            s += "%s=%f,\t" % (n, v)
            if writer is not None:
                writer.add_scalar(tag="Val-" + n, scalar_value=v, global_step=epoch_num + 1)
        self._say(s)
        self._say("Best Val {}: {}, Epoch: {}".format(self.host_metric_name, self.best_val, self.best_epoch))
