"""Attention maps of a pre-trained VL-BERT, with the reference's command line (pretrain/vis_attention_maps.py:11-41 over
pretrain/function/vis.py:24-143):

    python -m vl-bert_amd.pretrain.vis_attention_maps --cfg cfgs/pretrain/vis_attention_maps_coco.yaml --save-dir D [--dist] [--slurm]
           [--data] [--steps N] [--batch-images B] [--text-len T] [--regions R] [--compute bf16|fp16] [--dry-run]

It builds the module the YAML names (MODULE: ResNetVLBERTForAttentionVis, modules/resnet_vlbert_for_attention_vis.py), loads
NETWORK.PARTIAL_PRETRAIN with PARTIAL_PRETRAIN_PREFIX_CHANGES through the partial loader of common/checkpoint.py (a configured file that
does not exist is an error), switches the model to
eval, runs the loader and writes for every sample `D/attention_probs/{image_id}.npy`: float32 [layers, heads, n, n], n = the longest
packed sequence (text + boxes + END) of the sample's batch, the probabilities of the fused 16-bit attention path (csrc/attention_probs.hip).
`image_id` = dataset.ids[index], else the file stem of dataset.database[index]['image'], index = the last element of the sample's
im_info (vis.py:129-134).
Batches: with --data the validation loader of the YAML (vl-bert_amd/pretrain/data: make_dataloader(config, mode='val'),
Conceptual-Captions style sets); without it --steps N synthetic batches (synthetic.make_batch) of VAL.BATCH_IMAGES samples with ids
`synthetic_{i:06d}` (i counts over the ranks' samples under --dist).  The COCO-captions dataset class is not replaced (it needs pycocotools): `--data` with DATASET.DATASET:
coco_captions raises NotImplementedError.  --dry-run resolves and prints the configuration without touching a GPU.
"""
import argparse
import importlib
import json
import os
import sys

from .train_end2end import load_config

MODULES = ("ResNetVLBERTForAttentionVis",)
COCO_MESSAGE = ("DATASET.DATASET coco_captions: the COCO-captions dataset class is not replaced (it reads its annotations through "
                "pycocotools); point DATASET at a Conceptual-Captions style set (DATASET: conceptual_captions) or run without --data "
                "on synthetic batches")


def parse_args(argv=None):
    ap = argparse.ArgumentParser("Visualize Attention Maps")
    ap.add_argument("--cfg", type=str, help="path to a reference-style config file (cfgs/pretrain/vis_attention_maps_coco.yaml)")
    ap.add_argument("--dist", action="store_true", help="one process per GPU (torch.distributed.run / SLURM environment)")
    ap.add_argument("--slurm", action="store_true")
    ap.add_argument("--save-dir", type=str, default="./attention_maps", help="directory to save attention maps")
    ap.add_argument("--data", action="store_true", help="read the validation set the YAML names (DATASET.*) instead of synthetic batches")
    ap.add_argument("--steps", type=int, default=2, help="synthetic batches to run without --data")
    ap.add_argument("--batch-images", type=int, default=0, help="override VAL.BATCH_IMAGES (per GPU)")
    ap.add_argument("--text-len", type=int, default=64, help="text length of the synthetic batches")
    ap.add_argument("--regions", type=int, default=36, help="box count of the synthetic batches")
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp16"], help="the 16-bit type of the fused path (build of the library)")
    ap.add_argument("--dry-run", action="store_true", help="resolve and print the configuration, touch no GPU")
    return ap.parse_args(argv)


def resolve(config, world, args):
    if config.MODULE not in MODULES:
        raise NotImplementedError("MODULE %s: vis_attention_maps runs %s (train with pretrain.train_end2end)" % (config.MODULE, MODULES[0]))
    ds = config.get("DATASET", None)
    name = ds.get("DATASET", None) if hasattr(ds, "get") else None
    if args.data:
        if ds is None:
            raise ValueError("--data: the configuration has no DATASET section")
        if isinstance(ds, (list, tuple)):
            raise NotImplementedError("--data with a DATASET list: attention maps are written per image-caption sample of ONE set")
        if name == "coco_captions":
            raise NotImplementedError(COCO_MESSAGE)
    val = config.get("VAL", {}) or {}
    batch = int(args.batch_images or val.get("BATCH_IMAGES", 1))
    vl = config.NETWORK.VLBERT
    return dict(module=config.MODULE, world=world, per_gpu_batch=batch, data=bool(args.data), dataset=name,
                steps=None if args.data else int(args.steps), text_len=int(args.text_len), regions=int(args.regions),
                e2e=not config.NETWORK.IMAGE_FEAT_PRECOMPUTED, image_size=tuple(config.SCALES), compute=args.compute,
                layers=int(vl.get("num_hidden_layers", 12)), heads=int(vl.get("num_attention_heads", 12)),
                hidden_size=int(vl.get("hidden_size", 768)), seed=int(config.RNG_SEED),
                partial_pretrain=str(config.NETWORK.get("PARTIAL_PRETRAIN", "") or ""),
                prefix_changes=list(config.NETWORK.get("PARTIAL_PRETRAIN_PREFIX_CHANGES", []) or []),
                save_dir=os.path.join(args.save_dir, "attention_probs"))


class _SyntheticSet:
    """Stands in for loader.dataset: ids[index] names sample `index` (im_info's last element)."""

    def __init__(self, n):
        self.ids = ["synthetic_%06d" % i for i in range(n)]


def _synthetic_batches(r, rank, syn, torch):
    B, T, R = r["per_gpu_batch"], r["text_len"], r["regions"]
    for step in range(r["steps"]):
        batch = list(syn.make_batch(B, T, R, seed=1000 * rank + step, ragged=True))
        first = (rank * r["steps"] + step) * B          # every rank names its own samples
        batch[1][:, 4] = torch.arange(first, first + B)
        image = None
        if r["e2e"]:            # boxes inside a random image of SCALES, as the synthetic batches of train_end2end
            Hi, Wi = r["image_size"]
            gi = torch.Generator().manual_seed(7000 * (rank + 1) + step)
            image = torch.randn(B, 3, Hi, Wi, generator=gi) * 50.0
            valid = batch[0][:, :, 0] > -1.5
            box = batch[0][:, :, :4]
            box[:, :, 0].clamp_(0, Wi - 170)
            box[:, :, 1].clamp_(0, Hi - 170)
            box[:, :, 2] = torch.minimum(box[:, :, 2], torch.full_like(box[:, :, 2], Wi - 1.0))
            box[:, :, 3] = torch.minimum(box[:, :, 3], torch.full_like(box[:, :, 3], Hi - 1.0))
            batch[0] = torch.where(valid.unsqueeze(-1), box, torch.full_like(box, -2.0))
            batch[1][:, 0], batch[1][:, 1] = Wi, Hi
        yield [image] + batch


def image_id_of(dataset, index):
    """vis.py:130-133"""
    if hasattr(dataset, "ids"):
        return dataset.ids[index]
    return dataset.database[index]["image"].split("/")[1].split(".")[0]


def main(argv=None):
    args = parse_args(argv)
    config = load_config(args.cfg)
    if args.slurm:
        os.environ.setdefault("RANK", os.environ.get("SLURM_PROCID", "0"))
        os.environ.setdefault("WORLD_SIZE", os.environ.get("SLURM_NTASKS", "1"))
    world = int(os.environ.get("WORLD_SIZE", "1")) if args.dist else 1
    rank = int(os.environ.get("RANK", "0")) if args.dist else 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if args.dist else 0
    r = resolve(config, world, args)
    if args.dry_run:
        if rank == 0:
            print(json.dumps({"resolved": r, "NETWORK.VLBERT": dict(config.NETWORK.VLBERT)}, indent=1, default=str))
        return r
    # NETWORK.PARTIAL_PRETRAIN (vis.py:84-100): maps of a checkpoint that was not found would be maps of the random initialisation
    pp = r["partial_pretrain"]
    if pp and not os.path.isfile(pp):
        raise FileNotFoundError("NETWORK.PARTIAL_PRETRAIN %s not found (leave it empty to map the random initialisation)" % pp)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("vis_attention_maps: no GPU visible.  The MI355X engine has no CPU execution path (use --dry-run to check a "
                           "configuration without a GPU)")
    pkg = __package__.rsplit(".", 1)[0]
    if r["compute"] == "fp16":
        importlib.import_module(pkg + "._lib").set_precision("f16")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    log = print if rank == 0 else (lambda *a, **k: None)
    torch.manual_seed(r["seed"])
    modules = importlib.import_module(__package__ + ".modules")
    model = getattr(modules, config.MODULE)(config)
    if args.data:
        if "VAL" not in config or "BATCH_IMAGES" not in config.VAL or args.batch_images:
            config["VAL"] = type(config).wrap(dict(config.get("VAL", {}) or {}, BATCH_IMAGES=r["per_gpu_batch"]))
        data = importlib.import_module(__package__ + ".data")
        loader = data.make_dataloader(config, mode="val", distributed=world > 1, num_replicas=world, rank=rank)
        dataset, batches = loader.dataset, loader
    else:
        syn = importlib.import_module(pkg + ".synthetic")
        dataset = _SyntheticSet(world * r["steps"] * r["per_gpu_batch"])
        batches = _synthetic_batches(r, rank, syn, torch)
    if pp:          # (+ PARTIAL_PRETRAIN_PREFIX_CHANGES)
        ckpt = importlib.import_module(pkg + ".common.checkpoint")
        sd = torch.load(pp, map_location="cpu", weights_only=False)
        sd = ckpt.partial_pretrain_state_dict(sd.get("state_dict", sd), r["prefix_changes"])
        sd, _ = ckpt.drop_shape_mismatches(sd, model.state_dict(), log=log)
        ckpt.smart_partial_load(model, sd, log=log)
    if dist is not None:          # rank 0's parameters everywhere (vis.py:103-105)
        for v in model.state_dict().values():
            dist.broadcast(v, src=0)
    out_dir = r["save_dir"]
    os.makedirs(out_dir, exist_ok=True)
    model.eval()
    written = []
    for batch in batches:
        batch = [t.cuda(non_blocking=True) if t is not None else None for t in batch]
        if r["e2e"] and batch[0] is not None:
            batch[0] = batch[0].float()
        probs = model(*batch)["attention_probs"]
        probs = probs.cpu().numpy()          # one copy per batch; the synchronisation point of the loop
        im_info = batch[2].cpu()
        for i in range(im_info.shape[0]):    # (auxiliary text-only samples, if any, follow the image-caption ones and carry no image id)
            image_id = image_id_of(dataset, int(im_info[i][-1]))
            path = os.path.join(out_dir, "%s.npy" % image_id)
            np.save(path, probs[i].astype(np.float32, copy=False))
            written.append(path)
    log("vis_attention_maps: %d map(s) [%d layers, %d heads] written to %s" % (len(written), r["layers"], r["heads"], out_dir), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return written


if __name__ == "__main__":
    main(sys.argv[1:])
