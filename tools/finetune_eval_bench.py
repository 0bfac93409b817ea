#!/usr/bin/env python
"""VQA validation loop at the shipped shape (cfgs/vqa/large_4x16G_fp32.yaml: 24 x 1024, 16 samples per batch, 124 question tokens +
100 regions, 3129 answers), 10 batches after 3 warm-ups between two stream events:
  * host metric: the reference's SoftAccuracy.update on the returned logits -- torch argmax, advanced-index gather, `.sum().item()`
    and a host-side `+=` per batch (common/metrics/vqa_metrics.py:20-31);
  * device metric: common/vqa_metrics.SoftAccuracy (vlb_argmax_eval mode 2), no host read until get();
  * the metric alone on one batch's logits, both ways.
Usage: python tools/finetune_eval_bench.py [batch]"""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = importlib.import_module("vl-bert_amd.common.finetune_entry")
FE = importlib.import_module("vl-bert_amd.common.finetune_eval")
MT = importlib.import_module("vl-bert_amd.common.metrics")
VM = importlib.import_module("vl-bert_amd.common.vqa_metrics")
syn = importlib.import_module("vl-bert_amd.synthetic")
from tools.clock_probe import sclk_sysfs  # noqa: E402
from tools.eval_bench import timed  # noqa: E402

N_BATCH, WARM = 10, 3


class HostSoftAccuracy(object):
    """the reference's class, verbatim arithmetic"""

    def reset(self):
        self.sum_metric, self.num_inst = torch.tensor(0.), torch.tensor(0.)

    def update(self, outputs):
        cls_logits, label = outputs["label_logits"], outputs["label"]
        bs, num_classes = cls_logits.shape
        batch_inds = torch.arange(bs, device=cls_logits.device)
        self.sum_metric += float(label[batch_inds, cls_logits.argmax(1)].sum().item())
        self.num_inst += cls_logits.shape[0]


def loop_ms(net, batches, metrics):
    """ms per validation pass of len(batches) batches, end to end (stream events around do_validation)"""
    for _ in range(WARM):
        FE.do_validation(net, batches[:1], metrics, 4)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    FE.do_validation(net, batches, metrics, 4)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    dev = torch.device("cuda:0")
    config = F.load_config("vqa", None)
    config.NETWORK["IMAGE_FINAL_DIM"] = 1024
    config.NETWORK["CLASSIFIER_TYPE"] = "mlm"
    config.NETWORK.VLBERT.update(hidden_size=1024, visual_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)
    torch.manual_seed(0)
    net = importlib.import_module("vl-bert_amd.vqa.modules.resnet_vlbert_for_vqa").ResNetVLBERT(config, device=dev)
    batches = []
    for i in range(N_BATCH):
        boxes, im_info, question, label = syn.make_vqa_batch(B, 100, 124, 900 + i, dev)
        batches.append((None, boxes, im_info, question, label))
    host, device = HostSoftAccuracy(), VM.SoftAccuracy()
    res = {}
    for name, m in (("host metric (argmax + gather + .item() per batch)", host), ("device metric (vlb_argmax_eval mode 2)", device),
                    ("host metric, second pass", host), ("device metric, second pass", device)):
        res["validation loop, %d batches: %s" % (N_BATCH, name)] = loop_ms(net, batches, m) * 1e3
    print("finetune_eval_bench: batch %d, %d answers, sclk %s MHz" % (B, 3129, sclk_sysfs()))
    print("SoftAcc host %.6f device %.6f" % (float(host.sum_metric / host.num_inst), device.get()[1]))
    net.eval()
    with torch.no_grad():
        out = net(*batches[0][:4])
    out["label"] = batches[0][4]
    host.reset()
    device.reset()
    res["metric alone, one batch: host (argmax + gather + .sum().item())"] = timed(lambda: host.update(out))
    res["metric alone, one batch: device update() (two launches, no host read)"] = timed(lambda: device.update(out))
    for k, v in res.items():
        print("%12.1f us  %s" % (v, k))


if __name__ == "__main__":
    main()
