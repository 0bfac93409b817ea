"""`python -m vl-bert_amd.refcoco.train_end2end --cfg cfgs/refcoco/base_gt_boxes_4x16G.yaml [--dist]` -- the reference's
refcoco/train_end2end.py over the MI355X module mirror (vl-bert_amd/refcoco/modules/resnet_vlbert_for_refcoco.py); the loop is
vl-bert_amd/common/finetune_entry.py."""
import sys

from ..common.finetune_entry import main as _main


def main(argv=None):
    return _main("refcoco", argv)


if __name__ == "__main__":
    main(sys.argv[1:])
