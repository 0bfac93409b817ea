"""Helpers shared by the `-m gpu` parity tests."""
import importlib
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "gpurun_out", "parity_report.txt")


def pkg(name):
    return importlib.import_module("vl-bert_amd." + name)


def dev():
    return torch.device("cuda:0")


def act_dtype():
    """The library's 16-bit type: torch.bfloat16, or torch.float16 when the suite runs against the fp16 build (VLB_PRECISION=f16)."""
    return pkg("ops").BF16


def bf(t):
    """Round an fp32 CPU tensor to the library's 16-bit type (kept in fp32)."""
    return t.to(act_dtype()).float()


def to_gpu_bf16(t):
    return t.to(act_dtype()).to(dev())


def bar16(rtol):
    """The relative bar of a 16-BIT OUTPUT of the build under test: the caller's value on the bf16 build, 0.2 x it on the fp16 build
    (1e-2 -> 2e-3, the bar fp16 outputs already have in test_gemm_layernorm_residual_fp16_stream).  The unit roundoffs differ by 1/8
    (2^-9 against 2^-12): 0.2 leaves the same kind of headroom.  fp32 outputs keep their bars on both builds."""
    return rtol * 0.2 if act_dtype() == torch.float16 else rtol


def report(name, got, ref, atol, rtol):
    """max |got-ref| <= atol + rtol*max|ref|  (tensor-scale relative tolerance, bf16 friendly)."""
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    scale = ref.abs().max().item() if ref.numel() else 0.0
    bad = not np.isfinite(err) or err > atol + rtol * scale
    line = "%-44s max_err %.3e  ref_max %.3e  tol %.3e  %s" % (name, err, scale, atol + rtol * scale, "FAIL" if bad else "ok")
    print(line)
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass
    assert not bad, line


# ---- numpy re-statement of the device dropout RNG (vl-bert_amd/csrc/vlb_common.h) -------------
def _hash32(x):
    x = x.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def drop_thr(p):
    return 0 if p <= 0 else min(int(p * 65536.0 + 0.5), 65535)


def drop_scale(thr):
    return 65536.0 / (65536.0 - thr) if thr else 1.0


def _pair_hash(pair_idx, key):
    """vlb_pair_hash (vlb_common.h)"""
    m = np.uint64(0xFFFFFFFF)
    return _hash32(((pair_idx.astype(np.uint64) * np.uint64(0x9E3779B1)) + np.uint64(key)) & m)


def keep_mask(seed, tag, idx, thr):
    """idx: numpy integer array of element indices -> bool keep mask."""
    m = np.uint64(0xFFFFFFFF)
    idx = idx.astype(np.uint64)
    key = _hash32(np.array([(seed ^ ((tag * 0x85EBCA6B + 0x632BE5AB) & 0xFFFFFFFF)) & 0xFFFFFFFF], dtype=np.uint64))[0]
    h = _pair_hash(idx >> np.uint64(1), key)
    bits = np.where((idx & np.uint64(1)) == 1, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return bits >= np.uint64(thr)


def rng_advance(seed):
    """vlb_rng_advance (vl-bert_amd/csrc/optim.hip:255): seed <- hash32(seed + 0x9E3779B9) | 1, as uint32."""
    return int(_hash32(np.array([(int(seed) + 0x9E3779B9) & 0xFFFFFFFF], dtype=np.uint64))[0]) | 1


def device_seed(eng):
    """The engine's device-resident dropout seed (an int32 tensor) as the uint32 the kernels read."""
    return int(eng.seed.item()) & 0xFFFFFFFF


# ---- the engine's dropout layout: which (tag, element index) every dropout site draws ---------------------------------------
TAG_EMBED, TAG_DOWNSAMPLE = 1000, 1001          # vl-bert_amd/engine.py:30


class EngineDropoutMasks:
    """`drop_hook` for oracle/vlbert_oracle.py (see its `dropout`): the keep mask x device scale the engine regenerates at each
    dropout site, restated from keep_mask(seed, tag, idx, thr) and placed in the oracle's tensor layout.

    S is the engine's packed length T + R + 1 (the oracle's sequence is only max_length long: the engine-layout index is sliced to
    it); Bt = B + B_aux with the aux samples after the caption samples, as both lay them out.  Sp: the fp32 encoder's padded key
    stride (its softmax writes rows of Sp, vl-bert_amd/csrc/f32_path.hip:430,452), None for the 16-bit attention kernel.

      embedding         (b*S + s)*H + c        tag TAG_EMBED      embed_fwd / embed_bwd (engine.py:651,1036; csrc/embed.hip)
      attention_probs   ((b*nh + h)*S + q)*Sk + k, Sk = S or Sp  tag l*8+0   attention.hip:349 / f32_path.hip:430
      attention_output  m*H + n, m = b*S + s   tag l*8+1          gemm_p8.hip:167 (EPI 3/6), gemm.hip:190, f32_path.hip:230;
      ffn_output        m*H + n                tag l*8+2          backward: layernorm dx_drop (engine.py:949,957, f32_path.hip:363)
      obj_downsample    (b*R + r)*4096 + e     tag TAG_DOWNSAMPLE obj_prep_fwd (embed.hip:99); masked_colsum row_elems 4096,
                                                                  col_off 2048 (engine.py:1064); vision.hip:867 in the e2e path
    """

    def __init__(self, seed, S, R, nh, Sp=None):
        self.seed, self.S, self.R, self.nh, self.Sp = int(seed) & 0xFFFFFFFF, S, R, nh, Sp
        self.sites = []              # (site, layer) in call order: what the oracle asked for

    @staticmethod
    def thr(prob):
        return drop_thr(float(np.float32(prob)))     # vlb_drop_thr reads a float

    @staticmethod
    def scale(thr):
        return float(np.float32(65536.0) / np.float32(65536.0 - thr)) if thr else 1.0     # vlb_drop_scale (fp32 division)

    def index(self, site, shape, layer=None, inds=None):
        """(tag, uint64 element-index array of `shape`) for one site."""
        S, R, nh = self.S, self.R, self.nh
        ar = lambda n: np.arange(n, dtype=np.int64)
        if site == "embedding":
            b, s, H = shape
            return TAG_EMBED, (ar(b)[:, None, None] * S + ar(s)[None, :, None]) * H + ar(H)
        if site == "attention_probs":
            b, h, q, k = shape
            assert h == nh
            Sk = S if self.Sp is None else self.Sp
            row = (ar(b)[:, None, None] * nh + ar(h)[None, :, None]) * S + ar(q)[None, None, :]
            return layer * 8 + 0, row[..., None] * Sk + ar(k)
        if site in ("attention_output", "ffn_output"):
            b, s, H = shape
            m = ar(b)[:, None] * S + ar(s)[None, :]
            return layer * 8 + (1 if site == "attention_output" else 2), m[..., None] * H + ar(H)
        if site == "obj_downsample":
            K, E = shape
            assert E == 4096
            rows = inds[:, 0].numpy().astype(np.int64) * R + inds[:, 1].numpy().astype(np.int64)
            return TAG_DOWNSAMPLE, rows[:, None] * E + ar(E)
        raise ValueError("unknown dropout site %r" % (site,))

    def __call__(self, site, prob, shape, layer=None, inds=None):
        tag, idx = self.index(site, shape, layer, inds)
        thr = self.thr(prob)
        self.sites.append((site, layer))
        keep = keep_mask(self.seed, tag, idx.reshape(-1), thr).reshape(idx.shape)
        return torch.from_numpy(keep.astype(np.float32) * np.float32(self.scale(thr)))
