#!/usr/bin/env python
"""bench.py -- samples/sec of the VL-BERT-base pre-training step on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" = one optimizer step of the whole hot path (zero-grad, forward, backward, RCCL gradient
all-reduce overlapped with backward, global-norm clip, AdamW, weight refresh) on one synthetic batch
that is already resident in HBM.  Workload = BASELINE.json configs[1]: VL-BERT-base, 12 layers,
64 text + 36 regions (S=101), bf16, precomputed 2048-d region features, dropout ON (train mode),
global batch 256 split over the N ranks (strong scaling: 256/N samples per GPU).
Prints ONE JSON line on rank 0 (see the driver contract in the task statement).

A plain run sets up, warms up, times --steps steps and prints that line (`ms_per_step` = wall time of the timed steps / --steps).
--full adds, after the timed steps, every figure that needs runs of its own (roofline, clock probe, phase times, exposed
communication, CPU baseline, BASELINE configs 3-5).  --dump-outputs DIR writes the last timed step's results as float32 .npy files;
the inputs are seeded, so two builds run with the same arguments can be compared output for output.  The step's fp32 atomic
reductions (bias column sums, LayerNorm parameter sums, embedding scatter) are not bit-reproducible: compare with a tolerance.
"""
import argparse
import importlib
import json
import os
import sys
import time

import os as _os
_os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # (multi-process GPU work: the host driver only supports dmabuf IPC; before the HIP runtime loads)
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0


def flops_per_sample(cfg, T, R):
    """SURVEY.md §8d algorithmic FLOPs (multiply-add = 2): fwd; fwd+bwd = 3x."""
    H, I, V, C, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.visual_region_classes, cfg.num_hidden_layers
    S = T + R + 1
    per_layer = 8 * S * H * H + 4 * S * H * I + 4 * S * S * H
    fwd = L * per_layer + 2 * T * H * H + 2 * T * H * V + 2 * R * H * H + 2 * R * H * C + 2 * R * 4096 * H
    return fwd, 3 * fwd


def host_threads():
    """Thread count of the CPU baselines, reported as `cores`: the CPUs this process may run on, no more than OMP_NUM_THREADS when that
    is set, at most 64.  More torch threads than CPUs oversubscribe badly (256 threads on a large host measured 0.02 samples/s)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, min(n, 64))


def cpu_baseline(cfg_kw, T, R, budget_s=25.0, full=False):
    """The oracle ("port" of the reference modules, oracle/vlbert_oracle.py) timed on this box's host cores:
    forward + backward + AdamW of the same 12-layer model on a bounded sample (small batch, few iterations).
    full=True (--cpu-baseline-full): SURVEY.md 8d's form -- batch 32, 3 warm-up + 5 timed iterations, median (minutes of CPU time)."""
    from oracle import vlbert_oracle as O
    syn = importlib.import_module("vl-bert_amd.synthetic")
    cores = host_threads()
    torch.set_num_threads(cores)
    cfg = O.VLBertConfig(**cfg_kw)
    ref = _cpu_baseline_reference(cfg, T, R, cores, budget_s, full)      # the reference's OWN modules where its tree exists
    if ref is not None:
        return ref
    params = O.init_params(cfg, seed=0, randomize_all=False)
    Bc = 32 if full else 8
    batch = syn.make_batch(Bc, T, R, seed=0)
    m = {k: torch.zeros_like(v) for k, v in params.items()}
    v = {k: torch.zeros_like(v) for k, v in params.items()}
    times = []
    t_start = time.time()
    it = 0
    while it < (8 if full else 4) and (full or (time.time() - t_start) < budget_s):
        t0 = time.time()
        _, _, grads, _ = O.loss_and_grads(params, cfg, batch, train=True)
        for k in params:
            O.adamw_step(params[k], grads[k], m[k], v[k], it + 1, 1e-4, eps=1e-6, weight_decay=1e-4)
        times.append(time.time() - t0)
        it += 1
    if full:
        t = sorted(times[3:])[len(times[3:]) // 2]
        how = "3 warm-up + %d timed iterations, median %.2f s" % (len(times) - 3, t)
    else:
        t = min(times[1:]) if len(times) > 1 else times[0]
        how = "%d iterations (best of last %d)" % (len(times), max(1, len(times) - 1))
    return {"value": round(Bc / t, 3), "unit": "samples/s", "cores": cores, "kind": "port",
            "sample": "oracle fwd+bwd+AdamW, %d-layer hidden %d, batch %d x (%d+%d), fp32, dropout on, %s"
                      % (cfg.num_hidden_layers, cfg.hidden_size, Bc, T, R, how)}


def _cpu_baseline_reference(cfg, T, R, cores, budget_s, full):
    """`"kind": "reference"`: forward + backward + AdamW of the REFERENCE's ResNetVLBERTForPretraining (pretrain/modules/
    resnet_vlbert_for_pretraining.py:93-216) and its own AdamW (common/nlp/bert/optimization.py:107-187), imported from the reference
    tree through oracle/ref_import.py, on the same synthetic batch and the same bounded sample as the port -- only where that tree
    exists (the build container; VLBERT_REFERENCE_ROOT).  The GPU box has no reference tree: there this returns None and the caller
    times the oracle ("port", pinned to the reference at 1e-5 by tests/test_oracle_golden.py)."""
    import tempfile
    try:
        from oracle import ref_import
        if not os.path.isdir(ref_import.REFERENCE_ROOT):
            return None
        import contextlib
        with contextlib.redirect_stdout(sys.stderr):      # (the reference prints while it builds: stdout carries the ONE JSON line)
            RefModel, RefAdamW = ref_import.import_reference()
            vocab_dir = ref_import.make_vocab_dir(os.path.join(tempfile.gettempdir(), "vlb_vocab_bench"), cfg.vocab_size)
            torch.manual_seed(0)
            model = RefModel(ref_import.make_reference_config(cfg, vocab_dir))
    except Exception as e:            # (a reference tree that does not import here: say so, fall back to the port)
        print("bench.py: cpu_baseline: reference modules not usable (%s: %s) -- timing the oracle port" % (type(e).__name__, e), file=sys.stderr)
        return None
    syn = importlib.import_module("vl-bert_amd.synthetic")
    model.train()
    Bc = 32 if full else 8
    batch = syn.make_batch(Bc, T, R, seed=0)
    opt = RefAdamW([{"params": [p for _, p in model.named_parameters()]}], lr=1e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4,
                   correct_bias=True)
    times, t_start, it = [], time.time(), 0
    while it < (8 if full else 4) and (full or (time.time() - t_start) < budget_s):
        t0 = time.time()
        _, loss = model(None, *[t.clone() for t in batch])
        opt.zero_grad()
        loss.backward()
        opt.step()
        times.append(time.time() - t0)
        it += 1
    if full:
        t = sorted(times[3:])[len(times[3:]) // 2]
        how = "3 warm-up + %d timed iterations, median %.2f s" % (len(times) - 3, t)
    else:
        t = min(times[1:]) if len(times) > 1 else times[0]
        how = "%d iterations (best of last %d)" % (len(times), max(1, len(times) - 1))
    return {"value": round(Bc / t, 3), "unit": "samples/s", "cores": cores, "kind": "reference",
            "sample": "the reference's ResNetVLBERTForPretraining + its AdamW (imported from the reference tree), fwd+bwd+step, %d-layer hidden %d, "
                      "batch %d x (%d+%d), fp32, dropout on, %s" % (cfg.num_hidden_layers, cfg.hidden_size, Bc, T, R, how)}


def gemm_sources_sha():
    """Content hash of the GEMM kernel sources: stamps profiles/<tag>_gemm_traffic.json (tools/profile_report.py) and decides whether
    bench.py may quote that file as `roofline.traffic` -- PMC traffic of OTHER kernels is not this run's traffic."""
    import hashlib
    h = hashlib.sha1()
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vl-bert_amd", "csrc")
    for n in ("gemm.hip", "gemm_p8.hip", "gemm_tn8.hip", "gemm_params.h", "vlb_common.h"):
        with open(os.path.join(d, n), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:12]


DUMP_SAMPLE = 1 << 22      # elements per sampled --dump-outputs array: 16 MB of float32 (the limit for all arrays is 64 MB)


def sample_flat(tensors, n=DUMP_SAMPLE, seed=0):
    """A fixed, seeded sample of `n` elements of the concatenation of `tensors` (all of it when it holds no more than `n`), as one
    float32 tensor.  The positions depend only on the total size and the seed, so two runs with the same arguments sample alike."""
    flat = [t.detach().reshape(-1) for t in tensors]
    total = sum(t.numel() for t in flat)
    if total <= n:
        return torch.cat([t.float() for t in flat])
    idx = torch.randint(0, total, (n,), generator=torch.Generator().manual_seed(seed)).sort().values
    starts = torch.tensor([0] + [t.numel() for t in flat]).cumsum(0)
    cut = torch.searchsorted(idx, starts).tolist()          # idx is sorted: the positions inside tensor i are idx[cut[i]:cut[i + 1]]
    out = torch.empty(n, dtype=torch.float32, device=flat[0].device)
    for i, t in enumerate(flat):
        a, b = cut[i], cut[i + 1]
        if b > a:
            out[a:b] = t[(idx[a:b] - int(starts[i])).to(t.device)].float()
    return out


def dump_outputs(out_dir, arrays):
    """--dump-outputs DIR: the arrays the timed path computed in its last step, one float32 <DIR>/<name>.npy each."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())


def cpu_baseline_e2e(cfg_kw, T, R, image_size, vlbert):
    """e2e leg: the vision oracle (oracle/vision_oracle.py: ResNet-101 trunk + dilated layer4 head, torch CPU fp32, frozen stages
    and BatchNorm as in the reference) forward + backward on ONE image of the bench's size and its 36 RoI maps, combined with the
    VL-BERT oracle's per-sample time.  ROIAlign itself is left out of the CPU timing (the numpy oracle is loop-level test code;
    it is < 0.1 % of the FLOPs)."""
    from oracle import vision_oracle as VO
    cores = vlbert["cores"]
    torch.set_num_threads(cores)
    P = VO.init_vision_params(0, 101)
    frozen = VO.frozen_names(P)
    Po = {k: v.clone().requires_grad_(k not in frozen) for k, v in P.items()}
    img = torch.randn(1, 3, image_size[0], image_size[1]) * 50.0
    rois = torch.randn(R, 1024, 14, 14)
    best = None
    for _ in range(2):
        t0 = time.time()
        body4 = VO.backbone(img, Po, 101)
        feats = VO.roi_head(rois + body4.mean() * 0, Po, 101)
        (feats.sum() + body4.sum()).backward()
        dt = time.time() - t0
        best = dt if best is None else min(best, dt)
    per_sample = best + 1.0 / vlbert["value"]
    return {"value": round(1.0 / per_sample, 4), "unit": "samples/s", "cores": cores, "kind": "port",
            "sample": "vision oracle fwd+bwd on 1 image %dx%d + %d RoI maps (%.1f s, best of 2) + VL-BERT oracle step per sample (%s)"
                      % (image_size[0], image_size[1], R, best, vlbert["sample"])}


def vcr_config(large=True, num_layers=101):
    """cfgs/vcr/large_q2a_4x16G_fp16.yaml as the attribute tree the module mirror reads (NETWORK.*)."""
    class A(dict):
        __getattr__ = dict.__getitem__
    H, L, nh, I = (1024, 24, 16, 4096) if large else (768, 12, 12, 3072)
    return A(NETWORK=A(IMAGE_FEAT_PRECOMPUTED=False, IMAGE_SEMANTIC=False, IMAGE_STRIDE_IN_1x1=True, IMAGE_C5_DILATED=True,
                       IMAGE_NUM_LAYERS=num_layers, OUTPUT_CONV5=False, IMAGE_FROZEN_BN=True, IMAGE_FROZEN_BACKBONE_STAGES=[1, 2],
                       IMAGE_FINAL_DIM=H, BLIND=False, NO_GROUNDING=False, NO_OBJ_ATTENTION=False, ANSWER_FIRST=False, QA_ONE_SENT=False,
                       FOR_MASK_VL_MODELING_PRETRAIN=False, ENABLE_CNN_REG_LOSS=True, CNN_LOSS_TOP=True, CNN_REG_DROPOUT=0.0,
                       CNN_LOSS_WEIGHT=1.0, ANS_LOSS_WEIGHT=1.0, CLASSIFIER_TYPE="1fc", CLASSIFIER_HIDDEN_SIZE=1024,
                       CLASSIFIER_DROPOUT=0.1, CLASSIFIER_SIGMOID=True, CLASSIFIER_SIGMOID_LOSS_POSITIVE_WEIGHT=1.0,
                       VLBERT=A(hidden_size=H, visual_size=H, num_hidden_layers=L, num_attention_heads=nh, intermediate_size=I,
                                vocab_size=30522, max_position_embeddings=512, type_vocab_size=3, visual_ln=True, with_pooler=True,
                                hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, initializer_range=0.02,
                                visual_scale_text_init=0.0, visual_scale_object_init=0.0, object_word_embed_mode=2)))


def vcr_batch(*a, **kw):
    """vl-bert_amd/synthetic.py::make_vcr_batch (shared with the vcr/train_end2end entry point)."""
    return importlib.import_module("vl-bert_amd.synthetic").make_vcr_batch(*a, **kw)


def _mirror_gemm_roofline(ops, step, head_start, dev):
    """roofline of the dominant kernels of a module-mirror step (the bf16 MFMA GEMM launches of one optimizer step): every GEMM entry of
    `ops` is wrapped in a HIP event pair for ONE extra step, behind a head start of unrelated torch.mm work so that no pair contains a
    wait for the host.  -> (records, total GEMM ms, achieved TFLOP/s)"""
    rec = []
    names = ("gemm_nt", "gemm_nt_splitk", "wgrad_nt", "wgrad_tn")
    orig = {n: getattr(ops, n) for n in names}

    def timed(name):
        fn = orig[name]

        def wrapper(A, Bm, Cm, *a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(A, Bm, Cm, *a, **kw)
            e1.record()
            K = A.shape[0] if name == "wgrad_tn" else A.shape[1]
            rec.append((e0, e1, 2.0 * Cm.shape[0] * Cm.shape[1] * K))
            return out
        return wrapper
    orig_group = ops.wgrad_tn_group

    def timed_group(items, *a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_group(items, *a, **kw)
        e1.record()
        rec.append((e0, e1, sum(2.0 * dy.shape[0] * dy.shape[1] * x.shape[1] for dy, x, _, _ in items)))
        return out
    orig_f32 = ops.gemm_nt_f32

    def timed_f32(A, lda, B, ldb, C, ldc, M, N, K, *a, **kw):      # the fp32 encoder's GEMMs (linear layers, attention products, weight gradients)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_f32(A, lda, B, ldb, C, ldc, M, N, K, *a, **kw)
        e1.record()
        nb = kw.get("batch", (1, 1))
        rec.append((e0, e1, 2.0 * M * N * K * nb[0] * nb[1], "f32"))
        return out
    ops.gemm_nt_f32 = timed_f32
    for n in names:
        setattr(ops, n, timed(n))
    ops.wgrad_tn_group = timed_group
    hs_a = torch.zeros((8192, 4096), dtype=torch.bfloat16, device=dev)
    hs_b = torch.zeros((4096, 8192), dtype=torch.bfloat16, device=dev)
    hs_c = torch.empty((8192, 8192), dtype=torch.bfloat16, device=dev)
    for _ in range(head_start * 4):
        torch.mm(hs_a, hs_b, out=hs_c)
    step()
    torch.cuda.synchronize()
    for n in names:
        setattr(ops, n, orig[n])
    ops.wgrad_tn_group = orig_group
    ops.gemm_nt_f32 = orig_f32
    gemm_ms = sum(r[0].elapsed_time(r[1]) for r in rec)
    achieved = sum(r[2] for r in rec) / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
    return rec, gemm_ms, achieved


def _timed_mirror_steps(step, args, per_gpu_samples):
    """warm-up, then args.steps optimizer steps between barriers; MAX over the ranks -> (ms per step, whole-job samples/s, last loss)"""
    dist, world = args.dist, args.world

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
    last = None
    for _ in range(max(1, args.warmup)):
        last = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt)
    return elapsed / args.steps * 1e3, per_gpu_samples * world / (elapsed / args.steps), last


def vqa_config(answers=3129):
    """cfgs/vqa/large_4x16G_fp32.yaml as the attribute tree the module mirror reads."""
    class A(dict):
        __getattr__ = dict.__getitem__
    H, L, nh, I = 1024, 24, 16, 4096
    return A(DATASET=A(ANSWER_VOCAB_SIZE=answers),
             NETWORK=A(IMAGE_FEAT_PRECOMPUTED=True, IMAGE_SEMANTIC=False, IMAGE_STRIDE_IN_1x1=True, IMAGE_C5_DILATED=True, IMAGE_NUM_LAYERS=101,
                       OUTPUT_CONV5=False, IMAGE_FROZEN_BN=True, IMAGE_FROZEN_BACKBONE_STAGES=[1, 2], IMAGE_FINAL_DIM=H, BLIND=False,
                       NO_GROUNDING=False, ENABLE_CNN_REG_LOSS=False, CLASSIFIER_TYPE="mlm", CLASSIFIER_HIDDEN_SIZE=1024, CLASSIFIER_DROPOUT=0.1,
                       CLASSIFIER_SIGMOID=False,
                       VLBERT=A(hidden_size=H, visual_size=H, num_hidden_layers=L, num_attention_heads=nh, intermediate_size=I,
                                vocab_size=30522, max_position_embeddings=512, type_vocab_size=3, visual_ln=True, with_pooler=False,
                                hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, initializer_range=0.02,
                                visual_scale_text_init=0.0, visual_scale_object_init=0.0, object_word_embed_mode=2)))


def vqa_batch(*a, **kw):
    """vl-bert_amd/synthetic.py::make_vqa_batch (shared with the vqa/train_end2end entry point)."""
    return importlib.import_module("vl-bert_amd.synthetic").make_vqa_batch(*a, **kw)


def bench_vqa(args):
    """BASELINE config 4's workload through the module mirror: VL-BERT-large VQA fine-tuning, 128 text positions + 100 regions
    (precomputed features), 16 samples per micro-batch, 4 micro-batches per optimizer step, clip_grad_norm_ 1.0, the reference's AdamW.
    bf16 compute: the fp32 compute mode that config names is NOT built, which `dtype` and `config.note` say."""
    ops = importlib.import_module("vl-bert_amd.ops")
    lib = importlib.import_module("vl-bert_amd._lib")
    M = importlib.import_module("vl-bert_amd.vqa.modules.resnet_vlbert_for_vqa")
    OPT = importlib.import_module("vl-bert_amd.optim")
    arch, cus = lib.device_info(0)
    dev = torch.device("cuda:0")
    B, R, Lq, accum = 16, 100, 124, 4                              # text = [CLS] q [SEP] [MASK] [SEP] = Lq + 4 = 128 positions
    torch.manual_seed(0)
    net = M.ResNetVLBERT(vqa_config(), device=dev)
    with torch.no_grad():                                          # the shipped init leaves the visual LayerNorm gains at 0: open the visual path
        for n, p in net.named_parameters():
            if n.endswith("visual_ln_text.weight") or n.endswith("visual_ln_object.weight"):
                p.fill_(1.0)
    net.train()
    world, rank = args.world, args.rank
    if world > 1:      # vqa/function/train.py:327 wraps the model in DistributedDataParallel: 16 samples per GPU per micro-batch (weak scaling)
        net = importlib.import_module("vl-bert_amd.parallel").DistributedDataParallel(net)
    opt = OPT.FusedAdamW(net.parameters(), lr=6.25e-7 * B * accum * world, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4)
    batches = [vqa_batch(B, R, Lq, 700 + i + 100 * rank, dev) for i in range(accum)]

    def step():
        opt.zero_grad(set_to_none=False)
        total = 0.0
        for boxes, im_info, question, label in batches:
            outputs, loss = net(None, boxes, im_info, question, label)
            (loss / accum).backward()
            total = loss.detach()
        OPT.clip_grad_norm_(net.parameters(), 1.0, opt)          # fused into the step kernel (device-side norm, no rescale pass)
        opt.step()
        return total

    ms, value, last = _timed_mirror_steps(step, args, B * accum)
    if args.dump_outputs and rank == 0:
        _dump_mirror_outputs(args.dump_outputs, net, last)
    roofline = None
    if args.full:
        rec, gemm_ms, achieved = _mirror_gemm_roofline(ops, step, args.head_start, dev)
        roofline = _vqa_roofline(rec, achieved, gemm_ms, ms, args)
    if rank != 0:
        return
    out = {
        "metric": "samples/sec VL-BERT-large VQA fine-tuning step (128 text + 100 regions, precomputed features, AdamW, gradient accumulation 4)",
        "value": round(value, 2), "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype_name,
        "data": "synthetic (random-init weights, random boxes / features / tokens / answer scores, resident in HBM)",
        "config": {"workload": "BASELINE config 4's shape through the module mirror vl-bert_amd/vqa (cfgs/vqa/large_4x16G_fp32.yaml): 24 x 1024 "
                               "encoder, %d samples per micro-batch, %d text + %d regions + END = %d positions, 'mlm' classifier over %d answers + "
                               "BCE, clip 1.0, AdamW, %d micro-batches per optimizer step; a step = one optimizer step"
                               % (B, Lq + 4, R, Lq + 4 + R + 1, 3129, accum),
                   "note": ("config 4 at its named precision: fp32 encoder (24 layers: GEMMs, LayerNorm, softmax, residual stream, weights, "
                            "gradients in fp32; parity 6.9e-4 on logits at 24 layers, tests/test_f32_encoder_gpu.py), fp16 kernels for the "
                            "embedding side and the classifier" if args.fp32 else
                            "16-bit compute with fp32 master weights -- run with --precision fp32 for config 4's named precision"),
                   "global_batch": B * accum * world, "per_gpu_batch": B * accum, "seq_len": Lq + 4 + R + 1, "parallelism": "dp%d" % world,
                   "dp_exchange": "parallel.DistributedDataParallel: flat-gradient buckets from the engine's backward hooks + one coalesced "
                                  "all-reduce of the remaining parameters" if world > 1 else None, "arch": arch, "cus": cus},
        "roofline": roofline,
        "loss": round(float(last), 4),
    }
    if args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_vqa(B, R, Lq)
    print(json.dumps(out), flush=True)


def _dump_mirror_outputs(out_dir, net, loss):
    """--dump-outputs of a module-mirror step: the loss of its last micro-batch and a sample of the updated parameters."""
    dump_outputs(out_dir, {"loss": torch.as_tensor(loss).reshape(1), "weights_sample": sample_flat(list(net.parameters()))})


def _vqa_roofline(rec, achieved, gemm_ms, ms, args):
    if not args.fp32:
        return {"bound": "mfma", "kernel": "all %d 16-bit GEMM launches of one optimizer step (large-tile NT / TN cores + the 128x128 kernels "
                                           "on the classifier shapes)" % len(rec),
                "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                "traffic": None, "gemm_ms_per_step": round(gemm_ms, 3), "gemm_share_of_step": round(gemm_ms / ms, 3)}
    f32 = [r for r in rec if len(r) > 3]
    ms32 = sum(r[0].elapsed_time(r[1]) for r in f32)
    a32 = sum(r[2] for r in f32) / (ms32 * 1e-3) / 1e12 if ms32 > 0 else 0.0
    # an fp32 product = 3 bf16 MFMAs in gemm_f32_split_kernel: its ceiling is a third of the dense bf16 MFMA peak; gfx950's NATIVE fp32
    # MFMA peak (157.3 TFLOP/s, MI355X_MICROARCH.md) is given beside it
    return {"bound": "mfma", "kernel": "gemm_f32_split_kernel: the %d fp32 GEMM launches of one optimizer step (encoder linear layers, attention "
                                       "products, weight gradients); fp32 FLOPs = 2 M N K" % len(f32),
            "achieved": round(a32, 2), "peak": round(PEAK_BF16_TFLOPS / 3.0, 1), "unit": "TFLOP/s (fp32-equivalent)",
            "frac": round(a32 / (PEAK_BF16_TFLOPS / 3.0), 4), "native_fp32_mfma_peak": 157.3, "vs_native_fp32_mfma_peak": round(a32 / 157.3, 3),
            "traffic": None, "gemm_ms_per_step": round(ms32, 3), "gemm_share_of_step": round(ms32 / ms, 3),
            "all_gemm_launches": len(rec), "all_gemm_tflops": round(achieved, 2)}


def cpu_baseline_vqa(B, R, Lq):
    """the pinned VQA oracle (oracle/vqa_oracle.py: the restatement of the reference's own VQA module) on this box's host cores: forward +
    backward of ONE sample of the same shape, bounded sample."""
    from oracle import vlbert_oracle as O
    from oracle import vqa_oracle as VQ
    cores = host_threads()
    torch.set_num_threads(cores)
    cfg = O.VLBertConfig(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, with_pooler=False)
    params = VQ.init_vqa_params(cfg, 3, 3129, "mlm")
    batch = vqa_batch(1, R, Lq, 800, "cpu")
    best = None
    for _ in range(2):
        leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        t0 = time.time()
        out, loss = VQ.vqa_forward(leaves, cfg, *batch, classifier="mlm", classifier_dropout=0.1, train=True)
        loss.backward()
        dt = time.time() - t0
        best = dt if best is None else min(best, dt)
    return {"value": round(1.0 / best, 3), "unit": "samples/s", "cores": cores, "kind": "port",
            "sample": "VQA oracle fwd+bwd of 1 sample (24 x 1024, %d text + %d regions, fp32, dropout on), best of 2: %.2f s" % (Lq + 4, R, best)}


def bench_vcr(args):
    """BASELINE config 5: one optimizer step = 4 accumulated micro-batches of 4 samples x 4 answer choices (16 sequences of 256
    positions through the 24 x 1024 encoder + 4 images of 600x1000 through the ResNet-101 path), clip_grad_norm_ 10, SGD momentum."""
    ops = importlib.import_module("vl-bert_amd.ops")
    lib = importlib.import_module("vl-bert_amd._lib")
    M = importlib.import_module("vl-bert_amd.vcr.modules.resnet_vlbert_for_vcr")
    OPT = importlib.import_module("vl-bert_amd.optim")
    arch, cus = lib.device_info(0)
    dev = torch.device("cuda:0")
    B, C, R, Lq, La, accum = 4, 4, 55, 80, 117, 4                 # T = Lq + La + 3 = 200 text positions, S = T + R + 1 = 256
    Hi, Wi = args.image_size
    torch.manual_seed(0)
    net = M.ResNetVLBERT(vcr_config(), device=dev)
    with torch.no_grad():                                          # the shipped init leaves the visual LayerNorm gains at 0: open the visual path
        for n, p in net.named_parameters():
            if n.endswith("visual_ln_text.weight") or n.endswith("visual_ln_object.weight"):
                p.fill_(1.0)
        # No checkpoints exist offline: the ResNet runs on its random initialisation, where identity BatchNorms let the residual stream
        # double per block (33 blocks: beyond fp16's 65504 -- `--precision f16` gave loss = nan -- harmless in bf16).  The same 0.2 gain
        # on the BatchNorm that closes each residual branch (and the stem) as engine.init_random / vision.VisionStack.init_random use
        # keeps random-init activations O(1); timing does not depend on it.
        sd = net.state_dict()
        gains = {k: torch.full_like(v, 0.2) for k, v in sd.items() if k.endswith(".bn3.weight") or k.endswith("backbone.bn1.weight")}
        if gains:
            sd.update(gains)
            net.load_state_dict(sd)
    net.train()
    world, rank = args.world, args.rank
    if world > 1:      # vcr/function/train.py:330 wraps the model in DistributedDataParallel: 4 samples per GPU per micro-batch (weak scaling)
        net = importlib.import_module("vl-bert_amd.parallel").DistributedDataParallel(net)
    opt = OPT.FusedSGD(net.parameters(), lr=7.0e-5 * B * accum * world, momentum=0.9, weight_decay=1e-4)
    batches = [vcr_batch(B, C, R, Lq, La, Hi, Wi, 500 + i + 100 * rank, dev) for i in range(accum)]

    def step():
        opt.zero_grad(set_to_none=False)
        total = 0.0
        for image, boxes, masks, question, answers, label, im_info in batches:
            outputs, loss = net(image, boxes, masks, question, None, answers, None, label, im_info)
            (loss / accum).backward()
            total = loss.detach()
        OPT.clip_grad_norm_(net.parameters(), 10.0, opt)         # fused into the step kernel (device-side norm, no rescale pass)
        opt.step()
        return total

    ms, value, last = _timed_mirror_steps(step, args, B * accum)
    if args.dump_outputs and rank == 0:
        _dump_mirror_outputs(args.dump_outputs, net, last)
    roofline = None
    if args.full:
        rec, gemm_ms, achieved = _mirror_gemm_roofline(ops, step, args.head_start, dev)
        roofline = {"bound": "mfma", "kernel": "all %d bf16 GEMM launches of one optimizer step (encoder: large-tile NT / TN cores; vision "
                                               "path: implicit-GEMM convolutions)" % len(rec),
                    "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                    "traffic": None, "gemm_ms_per_step": round(gemm_ms, 3), "gemm_share_of_step": round(gemm_ms / ms, 3)}
    if rank != 0:
        return
    out = {
        "metric": "samples/sec VL-BERT-large VCR Q->A fine-tuning step (4 answer choices, 256-position sequences, ResNet-101 image path, "
                  "SGD, gradient accumulation 4)",
        "value": round(value, 2), "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype_name,
        "data": "synthetic (random-init weights, random images / boxes / masks / tokens / tags, resident in HBM)",
        "config": {"workload": "BASELINE config 5 through the module mirror vl-bert_amd/vcr (cfgs/vcr/large_q2a_4x16G_fp16.yaml): 24 x 1024 encoder, "
                               "%d samples x %d choices per micro-batch, %d text + %d regions + END = %d positions, %dx%d images, "
                               "1fc sigmoid classifier + top-of-BERT CNN regulariser, clip 10, SGD momentum 0.9, %d micro-batches per "
                               "optimizer step; a step = one optimizer step" % (B, C, Lq + La + 3, R, Lq + La + 3 + R + 1, Hi, Wi, accum),
                   "global_batch": B * accum * world, "per_gpu_batch": B * accum, "seq_len": Lq + La + 3 + R + 1, "parallelism": "dp%d" % world,
                   "arch": arch, "cus": cus},
        "roofline": roofline,
        "loss": round(float(last), 4),
    }
    if args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_vcr(Lq, La, R, (Hi, Wi))
    print(json.dumps(out), flush=True)


def cpu_baseline_vcr(Lq, La, R, image_size):
    """the pinned VCR oracle (oracle/vcr_oracle.py + vision_oracle.py: the restatement of the reference's own VCR module) on this box's
    host cores: forward + backward of ONE sample (4 choices, same sequence length, one 600x1000 image), bounded sample."""
    from oracle import vcr_oracle as VC
    from oracle import vision_oracle as VO
    from oracle import vlbert_oracle as O
    cores = host_threads()
    torch.set_num_threads(cores)
    cfg = O.VLBertConfig(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, with_pooler=True)
    params = VC.init_vcr_params(cfg, 3, classifier="1fc", embed_mode=2, cnn_reg_top=True)
    P = VO.init_vision_params(4, 101)
    frozen = VO.frozen_names(P)
    image, boxes, masks, question, answers, label, im_info = vcr_batch(1, 4, R, Lq, La, image_size[0], image_size[1], 600, "cpu")
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    Po = {k: v.clone().requires_grad_(k not in frozen) for k, v in P.items()}
    t0 = time.time()
    out, loss = VC.vcr_forward(leaves, cfg, image, boxes, masks, question, answers, label, im_info, Po, 101, classifier="1fc",
                               classifier_dropout=0.1, sigmoid=True, cnn_reg_top=True, train=True)
    loss.backward()
    t = time.time() - t0
    return {"value": round(1.0 / t, 4), "unit": "samples/s", "cores": cores, "kind": "port",
            "sample": "VCR oracle fwd+bwd, 1 sample x 4 choices, 256 positions, one %dx%d image through ResNet-101, fp32, dropout on, 1 iteration"
                      % image_size}


def other_configs():
    """BASELINE.json configs 3 (e2e: ResNet-101 + ROIAlign in front of the step, the shipped multitask yaml), 4 (VL-BERT-large VQA at its
    named precision, fp32) and 5 (VL-BERT-large VCR Q->A, mixed precision = the fp16 build) on this GPU, each as its own `bench.py --full`
    process (fresh engine, same flags a user would type; --full for their roofline figures); failures and
    time-outs are reported as such, never raised: the headline line must still print."""
    import subprocess
    here = os.path.abspath(__file__)
    # each config at the precision BASELINE.json names for it: config 3 bf16, config 4 fp32, config 5 "mixed precision" = the reference's
    # Apex fp16 mode = the fp16 build (the bf16 build's 24-layer numbers are an aside: its parity at that depth is 1.1e-2)
    runs = {"config3_e2e": ["--e2e", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--no-phase-times", "--full"],
            "config4_vqa_fp32": ["--vqa", "--precision", "fp32", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full"],
            "config5_vcr_fp16": ["--vcr", "--precision", "f16", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full"]}
    res = {}
    for name, flags in runs.items():
        cmd = [sys.executable, here] + flags
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = next((l for l in reversed(r.stdout.splitlines()) if l.startswith("{")), None)
            if r.returncode != 0 or line is None:
                res[name] = {"error": (r.stderr or r.stdout)[-300:], "cmd": "python bench.py " + " ".join(flags)}
                continue
            d = json.loads(line)
            res[name] = {"cmd": "python bench.py " + " ".join(flags), "metric": d.get("metric"), "value": d.get("value"), "unit": d.get("unit"),
                         "ms_per_step": d.get("ms_per_step"), "dtype": d.get("dtype"), "workload": (d.get("config") or {}).get("workload"),
                         "gemm_tflops": (d.get("roofline") or {}).get("achieved"), "gemm_frac_of_peak": (d.get("roofline") or {}).get("frac"),
                         "roofline_peak": (d.get("roofline") or {}).get("peak")}
        except Exception as e:      # (time-out, unparsable output)
            res[name] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200]), "cmd": "python bench.py " + " ".join(flags)}
    return res


def sustained_clock_mhz(ops, lib, dev):
    """Effective shader clock UNDER the large-tile GEMM, measured inside the kernel: every workgroup of one launch stamps the shader-clock
    counter (s_memtime) and the constant 100 MHz real-time counter (s_memrealtime) at entry and exit (gemm_p8.hip, p8_ablate = 4);
    clock = d(cycles) / d(real time), median over the workgroups, after 200 back-to-back launches of the same shape (FFN2 forward,
    25856 x 768 x 3072) have brought the device to its sustained power state.  sysfs / rocm-smi report the DPM level (2.4 GHz), not
    this: at its 1.4 kW cap the MI355X runs these kernels at ~1.9-2.0 GHz (profiles/r04_clock_probe.txt)."""
    try:
        M, N, K = 25856, 768, 3072
        g = torch.Generator().manual_seed(0)
        A = (torch.rand((M, K), generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
        B = ((torch.rand((N, K), generator=g) * 2 - 1) * 0.05).to(torch.bfloat16).to(dev)
        C = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        bias = torch.zeros(N, device=dev)
        table = torch.zeros((256, 32), dtype=torch.bfloat16, device=dev)           # 256 workgroups x 8 x int64
        for _ in range(200):
            ops.gemm_nt(A, B, C, bias=bias)
        lib.gemm_set_option("p8_ablate", 4)
        try:
            ops.gemm_nt(A, B, C, bias=bias, pre=table)
        finally:
            lib.gemm_set_option("p8_ablate", 0)
        torch.cuda.synchronize()
        t = table.view(torch.int64).view(256, 8).cpu()
        t = t[t[:, 3] > 0]
        if t.shape[0] < 8:
            return None
        mhz = (t[:, 2] - t[:, 0]).double() / (t[:, 3] - t[:, 1]).double() * 100.0
        return round(float(mhz.median()), 1)
    except Exception:
        return None


class LadderExhausted(RuntimeError):
    """every rung of run_ladder failed; .failures = [{"rung": name, "reason": text}]"""

    def __init__(self, failures):
        RuntimeError.__init__(self, "; ".join("%s: %s" % (f["rung"], f["reason"]) for f in failures))
        self.failures = failures


def run_ladder(rungs, attempt, agree=None, log=None):
    """First-contact insurance of the data-parallel bench (round 6): try the configurations of the gradient exchange from the fastest to
    the plainest and keep the first that EVERY rank completes.  rungs = [(name, spec)]; attempt(spec) returns a result or raises;
    agree(ok) -> True only when all ranks report ok (an all-reduce MIN over a gloo control group; None: single process).  Returns
    (name, result, failures) where failures lists the rungs given up with the local reason; raises LadderExhausted when none survives.
    A rank whose own attempt succeeded but whose peer failed discards its result and follows the peer down (reason "another rank failed").
    Host logic only -- tests/test_parallel_cpu.py drives it over gloo with injected failures."""
    failures = []
    for name, spec in rungs:
        try:
            res, ok, why = attempt(spec), True, None
        except Exception as e:      # noqa: BLE001 -- whatever a first contact with RCCL / graph capture raises
            res, ok, why = None, False, "%s: %s" % (type(e).__name__, str(e).replace("\n", " ")[:240])
        all_ok = bool(agree(ok)) if agree is not None else ok
        if all_ok:
            return name, res, failures
        failures.append({"rung": name, "reason": why or "another rank failed"})
        if log is not None:
            log("rung '%s' given up (%s)%s" % (name, failures[-1]["reason"], "" if (name, spec) == rungs[-1] else " -- trying the next one"))
        del res
    raise LadderExhausted(failures)


def dp_rungs(dp_mode, graph):
    """The ladder of `bench.py --gpus N`: sharded optimizer inside segmented hipGraphs -> the same exchange launched eagerly ->
    bucketed all-reduce with replicated AdamW, eager, fp32 on the wire (the plainest torch.distributed program there is).
    --dp-mode allreduce starts at the all-reduce rungs; --no-graph drops the graph rungs."""
    rungs = []
    if dp_mode in ("default", "sharded"):
        if graph:
            rungs.append(("sharded + segmented hipGraph", {"dp_mode": "sharded", "graph": True, "wire": None}))
        rungs.append(("sharded, eager", {"dp_mode": "sharded", "graph": False, "wire": None}))
    elif graph:
        rungs.append(("all-reduce + segmented hipGraph", {"dp_mode": "allreduce", "graph": True, "wire": None}))
    rungs.append(("all-reduce, eager, fp32 wire", {"dp_mode": "allreduce", "graph": False, "wire": "fp32"}))
    return rungs


def _fail(reason, code=1):
    """One line with the reason on stderr, non-zero exit code, no clean-up that could block (a hung collective cannot be joined)."""
    print("bench.py: FAILED: " + reason.replace("\n", " "), file=sys.stderr, flush=True)
    os._exit(code)


def _watchdog(seconds):
    """bench.py must never hang a multi-GPU run: after `seconds` of wall clock the process reports why it is stuck and exits 3."""
    import threading
    state = {"phase": "start-up"}

    def run():
        time.sleep(seconds)
        _fail("watchdog: still in phase '%s' after %d s (VLB_BENCH_WATCHDOG_S) -- a collective or a graph segment never completed"
              % (state["phase"], seconds), code=3)
    t = threading.Thread(target=run, daemon=True)
    t.start()
    return state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--global-batch", type=int, default=None, help="default 256 (strong scaling); with --e2e: 8 per GPU (weak scaling)")
    ap.add_argument("--e2e", action="store_true", help="config C3 (cfgs/pretrain/base_e2e_16x16G_fp16.yaml): ResNet-101 trunk + ROIAlign + "
                    "layer4 head on 600x1000 images, 8 images per GPU, in front of the same VL-BERT step")
    ap.add_argument("--image-size", type=int, nargs=2, default=(600, 1000))
    ap.add_argument("--aux-batch", type=int, default=None, help="text-only samples per GPU appended to the caption batch (MODULE "
                    "ResNetVLBERTForPretrainingMultitask).  Default: 8 with --e2e (TRAIN.BATCH_IMAGES [8, 8] of the shipped yaml), else 0")
    ap.add_argument("--large", action="store_true", help="VL-BERT-large shape of BASELINE.json configs 4-5 through the same pretraining step: "
                    "24 layers, hidden 1024, 16 heads, FFN 4096, 128 text + 100 regions (S = 229); default global batch 64")
    ap.add_argument("--vqa", action="store_true", help="BASELINE config 4's workload through the module mirror (vl-bert_amd/vqa): VL-BERT-large VQA "
                    "fine-tuning, 128 text + 100 precomputed regions, AdamW, accumulation 4; config 4's named precision is `--precision fp32`")
    ap.add_argument("--vcr", action="store_true", help="BASELINE config 5 through the module mirror (vl-bert_amd/vcr): VL-BERT-large VCR Q->A, 4 answer "
                    "choices, sequences of 256 positions, ResNet-101 image path with object masks, SGD momentum 0.9, gradient accumulation 4 "
                    "(cfgs/vcr/large_q2a_4x16G_fp16.yaml: 4 samples per GPU per micro-batch); one GPU; a step = one OPTIMIZER step")
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--precision", default=None, choices=["bf16", "f16", "fp32"], help="bf16 (default; BASELINE.json's headline precision) | "
                    "f16 = the fp16 build of the library: IEEE fp16 activations / working weights / gradients + a static loss scale (the "
                    "reference's Apex fp16 mode, TRAIN.FP16: true; same MFMA rate, 3 more mantissa bits per operand) | fp32 = every encoder "
                    "tensor in fp32 (vl-bert_amd/encoder_f32.py: fp32 products on the bf16 matrix cores by operand splitting), the fp16 build "
                    "around it -- the reference's TRAIN.FP16: false configurations (BASELINE config 4: --vqa --precision fp32)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline figure, after it: forward / forward+backward times, "
                    "the roofline of the GEMM launches (one extra instrumented step), the in-kernel clock probe, the per-rank exposed "
                    "communication, the CPU baseline and, on the headline configuration, BASELINE configs 3-5 under \"other_configs\".  "
                    "Without it the run only sets up, warms up, times --steps steps and prints the line (those fields are null)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one handed its "
                    "caller as float32 DIR/<name>.npy: the losses and a fixed seeded sample of the updated weights")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true", help="--full on the headline configuration also reports BASELINE configs 3 "
                    "(--e2e), 4 (--vqa --precision fp32) and 5 (--vcr --precision f16), each from a child bench.py process, under "
                    "\"other_configs\"; this switch (or any of --no-cpu-baseline / --e2e / --large / --vqa / --vcr / --precision / "
                    "--global-batch / --gpus N) skips them")
    ap.add_argument("--cpu-baseline-full", action="store_true", help="time the CPU port at SURVEY 8d's size (batch 32, 3 warm-up + 5 timed "
                    "iterations, median; ~1 min of host time) -- the DEFAULT of --full on the headline configuration (1 GPU, no mode flag)")
    ap.add_argument("--cpu-baseline-quick", action="store_true", help="the quick bounded leg (batch 8, <= 25 s) also on the headline "
                    "configuration")
    ap.add_argument("--dp-mode", default="default", choices=["default", "sharded", "allreduce"], help="data-parallel exchange "
                    "(vl-bert_amd/parallel.py): sharded optimizer (reduce-scatter + weight all-gather; default) or all-reduce")
    ap.add_argument("--head-start", type=int, default=60, help="unrelated 0.55-TFLOP torch.mm launches queued ahead of the instrumented step (roofline)")
    ap.add_argument("--no-clock-probe", action="store_true", help="skip the in-kernel sustained-clock measurement (201 extra launches of the FFN2 "
                    "shape after the timed region): profiling runs, so that the kernel tables hold the step's launches only")
    ap.add_argument("--no-phase-times", action="store_true", help="skip the separate forward / forward+backward timing loops (profiling runs)")
    ap.add_argument("--graph", action="store_true", help="replay the step as one hipGraph (single GPU).  Off by default: the step is "
                    "GPU-bound, not launch-bound -- measured on MI355X the eager stream launches are 3-5 %% FASTER than the graph replay "
                    "(26.97 vs 27.84 ms at batch 256, 6.72 vs 7.11 ms at batch 32)")
    ap.add_argument("--no-graph", action="store_true", help="never replay graphs.  With more than one rank the default IS graph replay in "
                    "segments cut at the collectives (engine.make_step_graph): the eager launch loop (~5 ms of host time per step) would "
                    "bound the 32-sample-per-GPU step")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.precision:      # read by vl-bert_amd/_lib.py / common/visual_linguistic_bert.py at import / construction (the imports below are lazy)
        os.environ["VLB_PRECISION"] = "f16" if args.precision == "fp32" else args.precision
        os.environ["VLB_ENCODER_FP32"] = "1" if args.precision == "fp32" else "0"
    prec = os.environ.get("VLB_PRECISION", "bf16").lower()
    args.fp32 = os.environ.get("VLB_ENCODER_FP32", "0") == "1"
    dtype_name = "fp16 (fp32 accumulation, fp32 master weights, static loss scale)" if prec in ("f16", "fp16", "half", "float16") else "bf16"
    if args.fp32:
        dtype_name = "fp32 (encoder: fp32 tensors, fp32 products by bf16 operand splitting with fp32 accumulation; embedding / head kernels fp16)"
    args.dtype_name = dtype_name

    if "RANK" not in os.environ and args.gpus > 1:
        # plain `python bench.py --gpus N`: re-launch ourselves as N ranks (one per GPU) under torch.distributed.run, exactly the
        # command line the driver would use; rank 0 of that job prints the JSON line, its exit code becomes ours
        import socket
        import subprocess
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "8")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd, env=env))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with --nproc-per-node %d (or without torch.distributed.run: bench.py "
                         "re-launches itself)" % (args.gpus, world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (MI355X); the product path has no CPU fallback")
    ndev = torch.cuda.device_count()
    shared = world > ndev        # more ranks than GPUs (CI on a 1-GPU box): ranks share devices; RCCL refuses that, gloo carries the exchange
    local_rank = local_rank % ndev
    torch.cuda.set_device(local_rank)
    dist = None
    backend = os.environ.get("VLB_BENCH_BACKEND", "gloo" if shared else "nccl")
    # VLB_DP_FORCE_EXCHANGE=1 (parallel.force_exchange): the whole multi-rank path of this file -- communicator, gradient buckets, sharded
    # optimizer, graph segments cut at the collectives, the exposed-communication measurement -- in a world of ONE, every collective the
    # identity: how a 1-GPU box executes what `--gpus 8` will run (tests/test_dp_gpu.py).  The line it prints is a functional record,
    # not a throughput claim (config.forced_exchange = true).
    forced = os.environ.get("VLB_DP_FORCE_EXCHANGE", "0") == "1" and world == 1
    multi = world > 1 or forced
    if forced and "MASTER_PORT" not in os.environ:
        import socket
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        os.environ["MASTER_PORT"] = str(s.getsockname()[1])
        s.close()
    if multi:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        # a collective that cannot complete (a rank that died, a communicator that never formed) must end the run with a reason, not
        # hang it: bounded time-out on every collective (RCCL's watchdog aborts the process group) + the wall-clock watchdog below
        tmo = datetime.timedelta(seconds=int(os.environ.get("VLB_BENCH_COLLECTIVE_TIMEOUT_S", "180")))
        try:
            if backend == "nccl":
                os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank), timeout=tmo)
            else:
                dist.init_process_group(backend, rank=rank, world_size=world, timeout=tmo)
            probe = torch.ones(1, device="cuda")
            dist.all_reduce(probe)           # first contact with the communicator: fail here, with the reason, rather than mid-step
            torch.cuda.synchronize()
            if int(probe.item()) != world:
                raise RuntimeError("probe all-reduce returned %s for %d ranks" % (probe.item(), world))
        except Exception as e:
            _fail("rank %d: %s communicator over %d ranks could not be formed: %s: %s" % (rank, backend, world, type(e).__name__, str(e)[:300]))
        # control plane of the fall-back ladder: a host-side gloo group, so that ranks can agree on "that rung failed somewhere" even when
        # the RCCL communicator is what failed
        try:
            ctl = dist.new_group(backend="gloo", timeout=datetime.timedelta(seconds=600))
        except Exception as e:
            _fail("rank %d: gloo control group could not be formed: %s: %s" % (rank, type(e).__name__, str(e)[:300]))

    args.world, args.rank, args.dist = world, rank, dist
    wd = _watchdog(int(os.environ.get("VLB_BENCH_WATCHDOG_S", "1500"))) if multi else {"phase": ""}
    if args.vqa or args.vcr:
        (bench_vqa if args.vqa else bench_vcr)(args)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    engine = importlib.import_module("vl-bert_amd.engine")
    syn = importlib.import_module("vl-bert_amd.synthetic")
    lib = importlib.import_module("vl-bert_amd._lib")
    ops = importlib.import_module("vl-bert_amd.ops")
    arch, cus = lib.device_info(local_rank)

    T, R = (128, 100) if args.large else (64, 36)
    if args.global_batch is None:
        args.global_batch = 8 * world if args.e2e else (64 if args.large else 256)
    per_gpu = args.global_batch // world
    aux = args.aux_batch if args.aux_batch is not None else (8 if args.e2e else 0)
    if args.large:
        args.layers = 24
        cfg = engine.ModelConfig(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, e2e=args.e2e,
                                 multitask=aux > 0)
    else:
        cfg = engine.ModelConfig(num_hidden_layers=args.layers, e2e=args.e2e, multitask=aux > 0)
    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    inject = [x.strip() for x in os.environ.get("VLB_BENCH_INJECT_FAIL", "").split(";") if x.strip()]      # (tests: ';'-separated rung names that must fail)

    def attempt(spec):
        """Engine + warm-up + the timed region under one configuration of the gradient exchange (spec = a dp_rungs() entry; world 1: the
        one configuration the command line asks for).  Raises when anything in it fails; the caller decides what to try next."""
        if spec.get("wire"):
            os.environ["VLB_DP_WIRE"] = spec["wire"]
        eng = engine.PretrainEngine(cfg, per_gpu, T, R, device="cuda:%d" % local_rank, train=True, lr=1e-4, weight_decay=1e-4,
                                    max_grad_norm=10.0, seed=1234 + rank, image_size=tuple(args.image_size) if args.e2e else None,
                                    B_aux=aux, dp_mode=spec["dp_mode"])
        eng.init_random(seed=rank, visual_ln_init=1.0 if args.e2e else 0.0)
        eng.broadcast_parameters(src=0)      # rank 0's parameters everywhere (the DDP start-up broadcast, pretrain/function/train.py:331-334)
        batch = syn.make_batch(per_gpu, T, R, seed=100 + rank)
        kw = {}
        if aux:           # the text-only corpus batch of the multitask wrapper (general_corpus.py): SEQ_LEN 64, no regions
            aux_text, aux_lab = syn.make_aux_text(aux, T, seed=300 + rank)
            kw.update(aux_text=aux_text.cuda(non_blocking=True), aux_mlm_labels=aux_lab.cuda(non_blocking=True))
        if args.e2e:      # images as the dataset hands them over (mean-subtracted pixels), boxes inside the image
            gi = torch.Generator().manual_seed(200 + rank)
            Hi, Wi = args.image_size
            image = torch.randn(per_gpu, 3, Hi, Wi, generator=gi) * 50.0
            bx = batch[0]
            bx[:, :, 0].clamp_(0, Wi - 170)
            bx[:, :, 1].clamp_(0, Hi - 170)
            bx[:, :, 2] = torch.minimum(bx[:, :, 2], torch.full_like(bx[:, :, 2], Wi - 1.0))
            bx[:, :, 3] = torch.minimum(bx[:, :, 3], torch.full_like(bx[:, :, 3], Hi - 1.0))
            bx[:, 0, :4] = torch.tensor([0.0, 0.0, Wi - 1.0, Hi - 1.0])
            batch[1][:, 0], batch[1][:, 1] = Wi, Hi
            kw["image"] = image.cuda(non_blocking=True)
            kw["mask_raw_pixels"] = True      # the dataset's MASK_RAW_PIXELS step (conceptual_captions.py:201-206), on the device copy
        eng.set_batch(*[t.cuda(non_blocking=True) for t in batch], **kw)
        eng.sync_weights()
        torch.cuda.synchronize()

        use_graph = bool(spec["graph"])
        step = eng.train_step
        graph_info = None
        if use_graph:
            eng.train_step()                            # lazy one-time setup + steady-state flags outside capture
            torch.cuda.synchronize()
            try:
                step = eng.make_step_graph()            # one graph (1 rank) / segments cut at the collectives (data parallel)
                graph_info = "%d graph segment(s) + %d host-side collective calls per step" % (step.n_graphs, step.n_calls)
            except Exception as e:                      # (a capture restriction of the installed runtime: the eager step is the same arithmetic)
                torch.cuda.synchronize()
                if multi:                               # the ladder's next rung is the eager form on a FRESH engine
                    raise RuntimeError("graph capture failed (%s: %s)" % (type(e).__name__, str(e)[:200]))
                print("bench.py: rank %d: graph capture failed (%s: %s) -- running the step eagerly" % (rank, type(e).__name__, str(e)[:200]),
                      file=sys.stderr, flush=True)
                step, use_graph = eng.train_step, False
        wd["phase"] = "warm-up steps (%s)" % spec.get("name", "single process")
        for _ in range(args.warmup):
            step()
        barrier()
        if spec.get("name") in inject:
            raise RuntimeError("injected failure (VLB_BENCH_INJECT_FAIL)")
        wd["phase"] = "timed steps (%s)" % spec.get("name", "single process")
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        elapsed = time.perf_counter() - t0
        return {"eng": eng, "step": step, "elapsed": elapsed, "use_graph": use_graph, "graph_info": graph_info}

    ladder = None
    if multi:
        rungs = [(n, dict(sp, name=n)) for n, sp in dp_rungs(args.dp_mode, not args.no_graph)]

        def agree(ok):
            t = torch.tensor([1 if ok else 0], dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MIN, group=ctl)
            if not int(t):      # leave nothing of the failed configuration behind: queued work, cached blocks
                try:
                    torch.cuda.synchronize()
                except Exception:      # noqa: BLE001
                    pass
                import gc
                gc.collect()
                torch.cuda.empty_cache()
            return bool(int(t))
        try:
            rung, res, given_up = run_ladder(rungs, attempt, agree,
                                             log=lambda m: print("bench.py: rank %d: %s" % (rank, m), file=sys.stderr, flush=True))
        except LadderExhausted as e:
            _fail("rank %d: every configuration of the gradient exchange failed: %s" % (rank, e))
        ladder = {"rung": rung, "given_up": given_up, "rungs": [n for n, _ in rungs]}
    else:
        res = attempt({"dp_mode": args.dp_mode, "graph": args.graph and not args.no_graph, "wire": None})
    eng, step, elapsed, use_graph, graph_info = res["eng"], res["step"], res["elapsed"], res["use_graph"], res["graph_info"]
    wd["phase"] = "post-processing"
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt)
    ms = elapsed / args.steps * 1e3
    total_samples = args.global_batch + aux * world          # caption samples + text-only samples of one step, all ranks
    value = total_samples / (elapsed / args.steps)
    if args.dump_outputs:       # the last timed step's losses, before the drain below runs a forward of its own
        dump = {"losses": eng.losses.clone()}
    if eng.buckets is not None and eng.buckets.sharded:     # drain the weight gathers of the last timed step before anything else runs
        eng.forward(True)
    losses = eng.loss_values()
    if args.dump_outputs:
        if eng.buckets is not None and eng.buckets.sharded:
            eng.buckets.gather_master(eng.P.master)          # (every rank) the owners' slices of the updated fp32 weights
        if rank == 0:
            dump_outputs(args.dump_outputs, dict(dump, weights_sample=sample_flat([eng.P.master])))

    # ---- exposed communication per rank = step time - the same step with every collective call skipped (GradBuckets.null_collectives:
    # identical kernels, graph segments and host calls at the same per-GPU batch; the numbers computed there are meaningless, the
    # parameters are re-broadcast afterwards).  Per-rank wall time between device syncs, no barrier inside.
    comm = None
    if args.full and multi and eng.buckets is not None:
        def rank_loop(n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n * 1e3
        wd["phase"] = "exposed-communication measurement"
        n_c = max(3, min(args.steps, 10))
        barrier()
        with_ms = rank_loop(n_c)
        if eng.buckets.sharded:
            eng.forward(True)
        barrier()
        eng.buckets.null_collectives(True)
        step()
        only_ms = rank_loop(n_c)
        eng.buckets.null_collectives(False)
        barrier()
        both = torch.tensor([with_ms, only_ms], dtype=torch.float64, device="cuda")
        allr = [torch.zeros_like(both) for _ in range(world)]
        dist.all_gather(allr, both)
        # back to consistent replicas (the null steps updated every rank from un-reduced gradients): the owners' master slices in
        # sharded mode (moments stay with their owners), rank 0's state otherwise
        if eng.buckets.sharded:
            eng.buckets.gather_master(eng.P.master)
        else:
            eng.broadcast_parameters(src=0)
        eng.sync_weights()
        torch.cuda.synchronize()
        comm = {"step_ms_per_rank": [round(float(t[0]), 3) for t in allr], "compute_only_ms_per_rank": [round(float(t[1]), 3) for t in allr],
                "exposed_comm_ms_per_rank": [round(float(t[0] - t[1]), 3) for t in allr], "steps": n_c,
                "how": "same step with every collective call skipped (parallel.GradBuckets.null_collectives), per-rank wall time"}
    wd["phase"] = "post-processing"

    # ---- forward-only and forward+backward times (SURVEY.md §8d asks for them next to the step time); outside the timed region
    def timed_loop(fn, n=5):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    fwd_ms = fwd_bwd_ms = None
    if args.full and world == 1 and not forced and not args.no_phase_times:
        fwd_ms = timed_loop(lambda: eng.forward(True))

        def fwd_bwd():
            eng.zero_grad()
            eng.forward(True)
            eng.backward(True)
        fwd_bwd_ms = timed_loop(fwd_bwd)

    roofline = None
    if args.full:
        # ---- roofline of the dominant kernel (the bf16 MFMA GEMM): one extra, instrumented step ---------------
        # HIP events are recorded on the stream the kernels are launched on (torch's current stream).
        rec, host = [], {}
        names = ("gemm_nt", "gemm_nt_splitk", "wgrad_nt", "wgrad_tn")     # wgrad_* / *_splitk include their slab reduce
        orig = {n: getattr(ops, n) for n in names}

        def timed(name):
            fn = orig[name]

            def wrapper(A, B, C, *a, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                h0 = time.perf_counter()
                out = fn(A, B, C, *a, **kw)
                host[name] = host.get(name, 0.0) + time.perf_counter() - h0
                e1.record()
                K = A.shape[0] if name == "wgrad_tn" else A.shape[1]      # TN form reduces over the rows
                nbytes = A.shape[0] * A.shape[1] * 2 + B.shape[0] * B.shape[1] * 2 + C.shape[0] * C.shape[1] * C.element_size()
                # + every side tensor the fused epilogue has to touch once: bias, the GELU' store, residual / aux rows, the LayerNorm
                # statistics and gamma / beta of a re-materialised residual (all "algorithmic": the fusion needs them)
                for key in ("bias", "pre", "aux", "res"):
                    t = kw.get(key)
                    if t is not None:
                        nbytes += t.shape[0] * (t.shape[1] if t.dim() > 1 else 1) * t.element_size()
                if kw.get("res_ln") is not None:
                    nbytes += C.shape[0] * 8 + 2 * C.shape[1] * 4
                rec.append((e0, e1, 2.0 * C.shape[0] * C.shape[1] * K, nbytes, name))
                return out
            return wrapper

        def timed_group(items, *a, **kw):         # the grouped weight gradients of one encoder layer (one launch)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h0 = time.perf_counter()
            out = orig_group(items, *a, **kw)
            host["wgrad_tn_group"] = host.get("wgrad_tn_group", 0.0) + time.perf_counter() - h0
            e1.record()
            fl = sum(2.0 * dy.shape[0] * dy.shape[1] * x.shape[1] for dy, x, _, _ in items)
            nb = sum(dy.numel() * 2 + x.numel() * 2 + C.numel() * 4 + (cs.numel() * 4 if cs is not None else 0) for dy, x, C, cs in items)
            rec.append((e0, e1, fl, nb, "wgrad_tn_group"))
            return out

        for n in names:
            setattr(ops, n, timed(n))
        orig_group = ops.wgrad_tn_group
        ops.wgrad_tn_group = timed_group
        orig_table_run = ops.WgradTable.run

        def timed_table(tab):                     # the deferred 1x1 weight gradients of a ResNet stage (e2e): one table launch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h0 = time.perf_counter()
            orig_table_run(tab)
            host["wgrad_tn_table"] = host.get("wgrad_tn_table", 0.0) + time.perf_counter() - h0
            e1.record()
            rec.append((e0, e1, tab.flops, tab.nbytes, "wgrad_tn_table"))
        ops.WgradTable.run = timed_table
        # the convolution forms of the e2e vision path (implicit-GEMM 3x3 forward / data gradient, TN weight gradients with the BatchNorm
        # scale): round 3's line left them out of `rec`, i.e. the e2e roofline covered the 1x1 convolutions and the encoder only
        conv_names = ("conv3x3_nhwc", "conv3x3_wgrad_tn", "wgrad_tn_rowscale")
        orig_conv = {n: getattr(ops, n) for n in conv_names}

        def timed_conv(name):
            fn = orig_conv[name]

            def wrapper(a, b, c, *rest, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                h0 = time.perf_counter()
                out = fn(a, b, c, *rest, **kw)
                host[name] = host.get(name, 0.0) + time.perf_counter() - h0
                e1.record()
                if name == "conv3x3_nhwc":          # (x [M, C], w [O, 9C], y [M, O])
                    fl, nb = 2.0 * a.shape[0] * b.shape[0] * b.shape[1], a.numel() * 2 + b.numel() * 2 + c.numel() * 2
                elif name == "conv3x3_wgrad_tn":    # (dy [M, O], x [M, C], dW [O, 9C])
                    fl, nb = 2.0 * a.shape[0] * c.shape[0] * c.shape[1], a.numel() * 2 + b.numel() * 2 + c.numel() * 4
                else:                               # (dy [R, Mo], x [R, No], C [Mo, No])
                    fl, nb = 2.0 * a.shape[0] * c.shape[0] * c.shape[1], a.numel() * 2 + b.numel() * 2 + c.numel() * 4
                rec.append((e0, e1, fl, nb, name))
                return out
            return wrapper
        for n in conv_names:
            setattr(ops, n, timed_conv(n))
        side, eng.side = eng.side, None          # kernel efficiency is measured with the GEMMs serialised on one stream
        vside = None
        if eng.vision is not None:
            vside, eng.vision.side = eng.vision.side, None
        # head start: the event pairs bracket single launches, so the device must never wait for the host inside a pair -- queue
        # ~40 ms of unrelated matmul work first (torch.mm = a hipBLASLt kernel, so it shows up under its own name in a kernel trace and
        # not among this library's GEMM launches) and let the eager launch loop run ahead of the device
        hs_a = torch.zeros((8192, 4096), dtype=torch.bfloat16, device=eng.dev)
        hs_b = torch.zeros((4096, 8192), dtype=torch.bfloat16, device=eng.dev)
        hs_c = torch.empty((8192, 8192), dtype=torch.bfloat16, device=eng.dev)
        for _ in range(args.head_start):
            torch.mm(hs_a, hs_b, out=hs_c)
        h_step = time.perf_counter()
        eng.train_step()
        h_step = time.perf_counter() - h_step
        torch.cuda.synchronize()
        eng.side = side
        if eng.vision is not None:
            eng.vision.side = vside
        for n in names:
            setattr(ops, n, orig[n])
        ops.wgrad_tn_group = orig_group
        ops.WgradTable.run = orig_table_run
        for n in conv_names:
            setattr(ops, n, orig_conv[n])
        gemm_ms = sum(r[0].elapsed_time(r[1]) for r in rec)
        gemm_flops = sum(r[2] for r in rec)
        gemm_alg_gb = sum(r[3] for r in rec) / max(len(rec), 1) / 1e9      # operands + epilogue side tensors read once, results written once
        by_op = {}
        for r in rec:
            a = by_op.setdefault(r[4], [0, 0.0, 0.0])
            a[0] += 1; a[1] += r[0].elapsed_time(r[1]); a[2] += r[2]
        by_op = {k: {"launches": v[0], "ms": round(v[1], 3), "tflops": round(v[2] / max(v[1], 1e-9) / 1e9, 1),
                     "host_ms": round(host.get(k, 0.0) * 1e3, 3)} for k, v in by_op.items()}
        by_op["host_launch_ms_whole_step"] = round(h_step * 1e3, 3)
        achieved = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        clock_mhz = sustained_clock_mhz(ops, lib, eng.dev) if (rank == 0 and prec == "bf16" and not args.no_clock_probe) else None
        fwd, fwdbwd = flops_per_sample(cfg, T, R)
        if aux:           # sample-weighted mean: a text-only sample is T tokens + END, no regions, MLM head only
            fa, fba = flops_per_sample(cfg, T, 0)
            wc, wa = per_gpu / (per_gpu + aux), aux / (per_gpu + aux)
        if args.e2e:      # + convolution FLOPs of the vision path (forward of every conv; dgrad + wgrad of the trainable stages)
            vs = eng.vision
            need_dx = vs._dgrad_set()
            vf = 2.0 * vs.N * vs.H1 * vs.W1 * 147 * 64
            vb = 0.0
            for b in vs.blocks:
                k, M, P, C = b["key"], b["M"], b["planes"], b["inplanes"]
                per = {"conv1": 2.0 * M * C * P, "conv2": 2.0 * M * 9 * P * P, "conv3": 2.0 * M * P * 4 * P}
                if b["downsample"]:
                    per["downsample.0"] = 2.0 * M * C * 4 * P
                vf += sum(per.values())
                if b["trainable"]:
                    vb += sum(f * (2 if k + n in need_dx else 1) for n, f in per.items())
            fwd, fwdbwd = fwd + vf / per_gpu, fwdbwd + (vf + vb) / per_gpu
        if aux:
            fwd, fwdbwd = wc * fwd + wa * fa, wc * fwdbwd + wa * fba
        # HBM bytes per GEMM launch come from PMC counters, which need their own rocprofv3 passes (tools/make_profiles.sh);
        # the committed summary of those passes is reported here when it was taken on this workload, else null.
        traffic, traffic_unit = None, None
        pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
        tname = next((n for n in ("r06_gemm_traffic.json", "r05_gemm_traffic.json", "r04_gemm_traffic.json", "r03_gemm_traffic.json", "r02_gemm_traffic.json")
                      if os.path.isfile(os.path.join(pdir, n))), None)
        if world == 1 and args.global_batch == 256 and args.layers == 12 and not args.e2e and not args.large and tname:
            with open(os.path.join(pdir, tname)) as f:
                tj = json.load(f)
            # quoted ONLY when the profile was taken on the GEMM sources this run executes (content hash stamped by tools/profile_report.py);
            # a summary of other kernels is named, not echoed (round-4 review: profile data of other sources must not pass through the line)
            sha = gemm_sources_sha()
            if tj.get("gemm_sources_sha") == sha:
                traffic = round(tj["gemm_hbm_GB_per_launch"], 4)
                traffic_unit = "GB per GEMM launch (avg over %d launches/step; rocprofv3 2xFETCH_SIZE+WRITE_SIZE, separate --pmc passes of this " \
                               "workload on these kernel sources (sha %s): profiles/%s%s; NOT measured inside this bench run)" % (
                                   round(tj["gemm_launches_per_step"]), sha, tname, ", commit " + tj["commit"] if "commit" in tj else "")
            else:
                traffic_unit = "null: profiles/%s was taken on other GEMM sources (sha %s, these are %s) -- re-run tools/make_profiles.sh" % (
                    tname, tj.get("gemm_sources_sha", "unstamped"), sha)
        # FLOPs the step EXECUTES (the MLM head runs on the labelled rows only -- engine mlm_cap -- so less than SURVEY 8d's algorithmic
        # count, which the north star's `step_frac_of_peak` is defined on): the timed GEMM launches + the attention matmuls
        H_, L_ = cfg.hidden_size, cfg.num_hidden_layers
        attn_flops = 3.0 * 4.0 * (T + R + 1) ** 2 * H_ * L_ * (per_gpu + aux)          # fwd + 2x bwd of QK^T and PV
        exec_tflop = (gemm_flops + attn_flops) / 1e12
        roofline = {"bound": "mfma", "kernel": "gemm_nt_p8_kernel + gemm_tn8_kernel (+ the 128x128 gemm_nt / gemm_tn kernels on the small head shapes): "
                                                  "all %d GEMM launches of one step" % len(rec),
                    "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                    # context, not the contract's number: the clock the chip holds under these kernels at its power cap, measured
                    # inside a GEMM launch (sustained_clock_mhz above), and the fraction of the MFMA peak AT that clock
                    "sustained_clock_mhz": clock_mhz, "nominal_clock_mhz": 2400.0,
                    "frac_at_sustained_clock": round(achieved / (PEAK_BF16_TFLOPS * clock_mhz / 2400.0), 4) if clock_mhz else None,
                    "traffic": traffic, "traffic_unit": traffic_unit,
                    "algorithmic_GB_per_launch": round(gemm_alg_gb, 4),
                    "gemm_ms_per_step": round(gemm_ms, 3), "gemm_share_of_step": round(gemm_ms / ms, 3), "by_op": by_op,
                    "step_algorithmic_tflops": round(value * fwdbwd / 1e12, 2),
                    "step_frac_of_peak": round(value * fwdbwd / 1e12 / (world * PEAK_BF16_TFLOPS), 4),
                    "step_executed_tflop_per_gpu": round(exec_tflop, 3),
                    "step_frac_of_peak_executed": round(exec_tflop / (ms * 1e-3) / PEAK_BF16_TFLOPS, 4)}

    if rank == 0:
        out = {
            "metric": "samples/sec VL-BERT-large pretrain step (seq 128+100 regions)" if args.large else ("samples/sec VL-BERT-base e2e pretrain (ResNet-101 on %dx%d images + seq 64+36 regions)" % tuple(args.image_size))
            if args.e2e else "samples/sec VL-BERT-base pretrain (seq 64+36 regions) at 1/2/4/8 MI355X",
            "value": round(value, 2), "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak" if args.e2e else "strong", "vs_baseline": None,
            "dtype": dtype_name, "data": "synthetic (random-init weights, random tokens/boxes/features, resident in HBM)",
            "config": {"workload": "VL-BERT-%s %d-layer pretrain step (fwd+bwd+clip+AdamW), %d text + %d regions, "
                                   "%s, dropout on" % ("large" if args.large else "base", args.layers, T, R, "ResNet-101 trunk + ROIAlign + dilated layer4 head on the device "
                                                       "(stages 1-2 and BatchNorm frozen)" if args.e2e else "precomputed 2048-d region features")
                                   + ("; multitask: %d image-caption + %d text-only samples per GPU in one encoder pass" % (per_gpu, aux) if aux else ""),
                       "global_batch": total_samples, "per_gpu_batch": per_gpu + aux, "per_gpu_caption_samples": per_gpu,
                       "per_gpu_text_only_samples": aux,
                       "module": "ResNetVLBERTForPretrainingMultitask" if aux else "ResNetVLBERTForPretraining",
                       "reference_cfg": ("cfgs/pretrain/base_e2e_16x16G_fp16.yaml" if (args.e2e and aux == 8 and per_gpu == 8 and not args.large)
                                         else None),
                       "seq_len": T + R + 1,
                       "parallelism": "dp%d" % world, "hipgraph": graph_info if use_graph else False, "arch": arch, "cus": cus,
                       "collective_backend": (("RCCL (nccl)" if backend == "nccl" else backend) if multi else None),
                       "forced_exchange": bool(forced),
                       "ranks": world,
                       "dp_exchange": (("sharded optimizer: reduce-scatter -> clip + AdamW on the owned 1/%d -> bf16 weight all-gather under "
                                        "the next forward" % world) if eng.buckets.sharded else "bucketed all-reduce, replicated AdamW")
                       if eng.buckets is not None else None,
                       "grad_wire_dtype": (str(eng.buckets.wire_dtype or torch.float32).replace("torch.", "") if eng.buckets is not None else None),
                       # which configuration of the exchange produced this number (run_ladder: the first one every rank completed) and
                       # the ones given up before it, with this rank's reason
                       "dp_ladder": ladder,
                       # RCCL channels = CUs a collective kernel holds while the persistent one-workgroup-per-CU GEMMs want all 256
                       # (tools/contention_probe.py: +1-7 % on the GEMMs with 8-64 CUs held, independent of how many -- left at RCCL's default)
                       "nccl_max_nchannels": os.environ.get("NCCL_MAX_NCHANNELS"),
                       "ranks_share_devices": bool(shared)},
            "roofline": roofline,
            "comm": comm,
            "fwd_ms": round(fwd_ms, 3) if fwd_ms is not None else None,
            "fwd_bwd_ms": round(fwd_bwd_ms, 3) if fwd_bwd_ms is not None else None,
            "loss": round(losses["loss"], 4),
        }
        if args.full and not args.no_cpu_baseline and world == 1:
            ckw = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096) if args.large \
                else dict(num_hidden_layers=args.layers)
            plain = (args.global_batch == 256 and args.layers == 12 and not args.e2e and not args.large and not args.precision)
            full = args.cpu_baseline_full or (plain and not args.cpu_baseline_quick)      # SURVEY 8d's form on the headline configuration
            out["cpu_baseline"] = cpu_baseline(ckw, T, R, budget_s=12.0 if args.e2e else 25.0, full=full)
            if args.e2e:
                out["cpu_baseline"] = cpu_baseline_e2e(dict(num_hidden_layers=args.layers), T, R, tuple(args.image_size), out["cpu_baseline"])
        if (args.full and not args.no_cpu_baseline and not args.no_other_configs and world == 1 and args.global_batch == 256
                and args.layers == 12 and not args.e2e and not args.large and not args.precision):
            # --full on the headline configuration also reports BASELINE.json's configs 3, 4 and 5, each measured by a child
            # `bench.py` of its own after the headline measurement above is complete: they are context, not part of `value`.
            out["other_configs"] = other_configs()
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
