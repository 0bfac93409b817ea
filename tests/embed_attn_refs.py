"""Input builders and float64 CPU reference statements shared by tests/test_embed_attn_ops_gpu.py (kernel vs reference) and
tests/test_embed_attn_refs_cpu.py (reference vs deliberately wrong reference: every battery must bite).

Every reference here is a closed-form PyTorch / numpy statement of one operation in float64 on 16-bit-rounded inputs, gradients by
autograd.  `mutant=` selects one deliberately WRONG statement; the GPU tests never pass it.
"""
import math

import numpy as np
import torch

from tests.gpu_util import TAG_EMBED, drop_scale, drop_thr, keep_mask

EMBED_SEED = 4242
KIND_PAD, KIND_TEXT, KIND_OBJ, KIND_END = 0, 1, 2, 3

# The embedding battery.  zeroed: text_vis_zeroed of the broadcast text-visual gradient (pretrain form only); ling: which row of the
# 2-row linguistic table the objects select (pretrain form only); types: token-type ids given to text tokens (module form only).
#   H      128 NIT=1 | 320 NIT=2, ragged last 256-column group | 768 NIT=3 | 1024 NIT=4 | 2048 NIT=8
#   B      <= 5: 8 workgroups per sample (broadcast form: only with zeroed=True, else 1) | 520: one workgroup per sample
#   Sx     S = T + R + 1 + Sx: trailing pad rows in every sample
#   P      10 < T = 12: text rows, the shared object row and the end row clamp to P - 1 | 64: positions past the longest stay untouched
#   V      8: hundreds of rows collide on one d_word row | 512: most vocabulary rows stay untouched
# Every case holds a sample with all T tokens and all R objects (sample 0), one with no object (sample 1), object masks with holes
# (samples >= 2: padded boxes between valid ones), token ids < 0 and >= V, and both type ids 0 and 1 in every sample (module form).
EMBED_CASES = {
    # name          mode      H     B   Sx  P   V    p    zeroed ling   types
    "pre-h128":    ("pretrain", 128, 3, 0, 64, 512, 0.0, False, "mix", None),       # one workgroup per sample writes d_text_vis
    "pre-h320":    ("pretrain", 320, 4, 3, 64, 8, 0.1, True, "all0", None),         # table row 1 exactly zero; pad rows; V = 8
    "pre-h768":    ("pretrain", 768, 5, 0, 10, 512, 0.0, True, "all1", None),       # table row 0 exactly zero; position clamp
    "pre-h1024":   ("pretrain", 1024, 2, 2, 64, 512, 0.1, False, "mix", None),
    "pre-h2048":   ("pretrain", 2048, 2, 0, 64, 512, 0.0, True, "mix", None),
    "pre-b520":    ("pretrain", 128, 520, 0, 64, 8, 0.1, False, "mix", None),       # split = 1, plain store of the per-sample sum
    "pre-b520-z":  ("pretrain", 128, 520, 1, 10, 512, 0.0, True, "mix", None),      # split = 1 with zeroed memory; position clamp
    "mod-h128":    ("module", 128, 3, 0, 64, 512, 0.1, False, None, (0, 1)),
    "mod-h320":    ("module", 320, 4, 3, 64, 8, 0.0, False, None, (0, 1, 2)),       # type 2 on text tokens (LDS-atomic branch)
    "mod-h768":    ("module", 768, 5, 0, 10, 512, 0.1, False, None, (0, 1)),        # position clamp
    "mod-h1024":   ("module", 1024, 2, 2, 64, 512, 0.0, False, None, (0, 1)),
    "mod-h2048":   ("module", 2048, 2, 0, 64, 512, 0.1, False, None, (0, 1, 2)),
    "mod-b520":    ("module", 128, 520, 1, 64, 8, 0.0, False, None, (0, 1)),        # split = 1
}
EMBED_T, EMBED_R = 12, 5


def rounder(dtype):
    """fp32 CPU tensor -> the same values rounded to the 16-bit type `dtype`, kept in fp32."""
    return lambda t: t.to(dtype).float()


def seq_layout_ref(text_mask, obj_mask, S):
    """[text || objects || END || pad] per sample: kind [B,S], source index [B,S], text_len [B], nobj [B] (all long)."""
    B, T = text_mask.shape
    R = obj_mask.shape[1]
    kind = torch.zeros(B, S, dtype=torch.long)
    idx = torch.zeros(B, S, dtype=torch.long)
    tl = text_mask.sum(1).long()
    no = obj_mask.sum(1).long()
    for b in range(B):
        ts = torch.nonzero(text_mask[b]).flatten()
        os_ = torch.nonzero(obj_mask[b]).flatten()
        n, m = len(ts), len(os_)
        kind[b, :n], idx[b, :n] = KIND_TEXT, ts
        kind[b, n:n + m], idx[b, n:n + m] = KIND_OBJ, os_
        kind[b, n + m] = KIND_END
    return kind, idx, tl, no


def embed_case(name, dtype):
    """All inputs of one embedding case (CPU; 16-bit tensors as rounded fp32 values)."""
    mode, H, B, Sx, P, V, p, zeroed, ling, types = EMBED_CASES[name]
    T, R = EMBED_T, EMBED_R
    S = T + R + 1 + Sx
    rd = rounder(dtype)
    g = torch.Generator().manual_seed(1000 + sorted(EMBED_CASES).index(name))
    rn = lambda *s, scale=1.0: rd(torch.randn(*s, generator=g) * scale)
    lens = torch.randint(2, T + 1, (B,), generator=g)
    lens[0] = T
    text_mask = torch.arange(T)[None, :] < lens[:, None]
    obj_mask = torch.rand(B, R, generator=g) < 0.6          # holes: padded boxes between valid ones
    obj_mask[0] = True
    obj_mask[1] = False
    text_ids = torch.randint(0, V, (B, T), generator=g)
    text_ids[:, 1] = torch.where(torch.arange(B) % 2 == 0, torch.tensor(-3), torch.tensor(V + 5))     # clamped to 0 / V - 1
    text_ids[0, 2], text_ids[1, 0] = V, -1
    c = dict(name=name, mode=mode, H=H, B=B, T=T, R=R, S=S, P=P, V=V, p=p, zeroed=zeroed, text_mask=text_mask, obj_mask=obj_mask,
             text_ids=text_ids, word=rn(V, H), pos=rn(P, H), type=rn(3, H), end=rn(1, H),
             gamma=1.0 + 0.2 * torch.randn(H, generator=g), beta=0.2 * torch.randn(H, generator=g), obj_vis=rn(B, R, H))
    if mode == "pretrain":
        c["text_type"] = None
        c["text_vis"] = rn(B, H)                                  # one row per sample, broadcast over its tokens
        c["obj_ling"] = rn(2, H)                                  # the 2-row table: independent unit-variance rows, far apart
        sel = torch.randint(0, 2, (B, R), generator=g)
        sel[0, 0], sel[0, 1] = 0, 1
        c["ling_idx"] = {"mix": sel, "all0": torch.zeros_like(sel), "all1": torch.ones_like(sel)}[ling]
    else:
        tt = torch.tensor(types)[torch.randint(0, len(types), (B, T), generator=g)]
        tt[:, 0], tt[:, 1] = 0, 1                                 # both ids in every sample (every sample has >= 2 tokens)
        if 2 in types:
            tt[0, 2] = 2
        c["text_type"] = tt
        c["text_vis"] = rn(B, T, H)
        c["obj_ling"] = rn(B, R, H)
        c["ling_idx"] = None
    c["kind"], c["idx"], c["tl"], c["no"] = seq_layout_ref(text_mask, obj_mask, S)
    dy = torch.randn(B, S, H, generator=g) * (0.25 if B > 64 else 1.0)
    c["dy"] = rd(dy * (c["kind"] != KIND_PAD)[..., None])         # pad rows never reach a loss: their dy is exactly zero
    thr = drop_thr(p)
    c["keep"] = None
    if thr:
        keep = keep_mask(EMBED_SEED, TAG_EMBED, np.arange(B * S * H), thr).reshape(B, S, H)
        c["keep"] = torch.from_numpy(keep.astype(np.float64)) * drop_scale(thr)
    return c


EMBED_MUTANTS = ("type1_to_0", "table_swapped", "pos_not_clamped", "obj_pos_is_s")


def embed_ref(c, mutant=None, eps=1e-12):
    """VisualLinguisticBert.embedding in float64: gather word / position / type rows, add the visual parts, LayerNorm, mask x scale;
    backward of sum(out * dy) by autograd.  Returns (forward dict, gradient dict)."""
    assert mutant is None or mutant in EMBED_MUTANTS
    B, T, R, S, H, V, P = (c[k] for k in "BTRSHVP")
    leaf = lambda t: t.double().clone().requires_grad_(True)
    L = {k: leaf(c[k]) for k in ("word", "pos", "type", "end", "gamma", "beta", "text_vis", "obj_vis", "obj_ling")}
    kind, idx, tl = c["kind"], c["idx"], c["tl"]
    bg = torch.arange(B)[:, None].expand(B, S)
    sg = torch.arange(S)[None, :].expand(B, S)
    is_t, is_o, is_e = kind == KIND_TEXT, kind == KIND_OBJ, kind == KIND_END
    bt, tt = bg[is_t], idx[is_t]
    ids = c["text_ids"][bt, tt].clamp(0, V - 1)                  # the kernel documents the clamp of token ids
    tv = L["text_vis"][bt] if c["mode"] == "pretrain" else L["text_vis"][bt, tt]
    bo, ro = bg[is_o], idx[is_o]
    if c["mode"] == "pretrain":
        sel = c["ling_idx"][bo, ro]
        ling = L["obj_ling"][1 - sel if mutant == "table_swapped" else sel]
    else:
        ling = L["obj_ling"][bo, ro]
    vl = torch.zeros(B, S, H, dtype=torch.float64)
    vl = vl.index_put((bt, sg[is_t]), L["word"][ids] + tv)
    vl = vl.index_put((bo, sg[is_o]), L["obj_vis"][bo, ro] + ling)
    vl = vl.index_put((bg[is_e], sg[is_e]), L["end"][0].expand(int(is_e.sum()), H))
    typ = torch.zeros(B, S, dtype=torch.long)                    # pad rows: zeros + position s + type 0
    if c["text_type"] is not None:
        typ[is_t] = c["text_type"][bt, tt].clamp(0, 2)
    if mutant == "type1_to_0":
        typ[typ == 1] = 0
    typ[is_o | is_e] = 2
    pos = sg.clone()
    if mutant != "obj_pos_is_s":
        pos[is_o] = tl[:, None].expand(B, S)[is_o]              # every object of a sample shares position text_len
    pos[is_e] = (tl + 1)[:, None].expand(B, S)[is_e]
    pos = pos % P if mutant == "pos_not_clamped" else pos.clamp(max=P - 1)
    pre = vl + L["pos"][pos] + L["type"][typ]
    mean = pre.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(pre.var(-1, unbiased=False, keepdim=True) + eps)
    out = (pre - mean) * rstd * L["gamma"] + L["beta"]
    if c["keep"] is not None:
        out = out * c["keep"]
    (out * c["dy"].double()).sum().backward()
    fwd = dict(pre=pre.detach(), out=out.detach(), mean=mean.detach().reshape(B * S), rstd=rstd.detach().reshape(B * S))
    grads = {k: v.grad for k, v in L.items()}
    return fwd, grads


def embed_parts(c, g):
    """Backward results split into the sub-tensors that are reported separately, each against its own scale.  g: dict word / pos /
    type / end / gamma / beta / text_vis / obj_vis / obj_ling -> tensor (device result or reference).  d_pos rows are grouped by
    what lands on them: the shared object row `text_len` of some sample (sum of all its objects: the large rows), the end row
    `text_len + 1` of some sample (where no sample's object row coincides), and rows that only text tokens (and pad rows) reach."""
    P, tl, no = c["P"], c["tl"], c["no"]
    obj_rows = set(int(min(t, P - 1)) for t, n in zip(tl.tolist(), no.tolist()) if n > 0)
    end_rows = set(int(min(t + 1, P - 1)) for t in tl.tolist()) - obj_rows
    text_rows = [r for r in range(min(int(tl.max()), P)) if r not in obj_rows and r not in end_rows]
    f = lambda t: t.detach().double().cpu()
    parts = {"d_word": f(g["word"]), "d_end": f(g["end"]), "d_gamma": f(g["gamma"]), "d_beta": f(g["beta"]),
             "d_text_vis": f(g["text_vis"]), "d_obj_vis": f(g["obj_vis"]),
             "d_type row0": f(g["type"])[0], "d_type row1": f(g["type"])[1], "d_type row2": f(g["type"])[2]}
    pos = f(g["pos"])
    for nm, rows in (("d_pos text rows", text_rows), ("d_pos object rows", sorted(obj_rows)), ("d_pos end rows", sorted(end_rows))):
        if rows:
            parts[nm] = pos[rows]
    if c["mode"] == "pretrain":
        parts["d_ling table row0"], parts["d_ling table row1"] = f(g["obj_ling"])[0], f(g["obj_ling"])[1]
    else:
        parts["d_obj_ling"] = f(g["obj_ling"])
    return parts


def embed_untouched(c):
    """Boolean row masks of gradient rows that no input names: word [V], pos [P], obj [B,R] (padded boxes), text [B,T] (padded tokens)."""
    V, P = c["V"], c["P"]
    word = torch.ones(V, dtype=torch.bool)
    word[c["text_ids"][c["text_mask"]].clamp(0, V - 1)] = False
    pos = torch.ones(P, dtype=torch.bool)
    pos[:min(int(c["tl"].max()), P)] = False                       # text rows (pad rows are skipped: their dy is exactly zero)
    pos[c["tl"][c["no"] > 0].clamp(max=P - 1)] = False             # shared object rows
    pos[(c["tl"] + 1).clamp(max=P - 1)] = False                    # end rows
    return dict(word=word, pos=pos, obj=~c["obj_mask"], text=~c["text_mask"])


FP32_GRAD_TOL = (2e-3, 1e-2)      # the embedding's fp32 gradient outputs (tests/test_ops_gpu.py: test_seq_layout_and_embedding)
ACT16_TOL = (1e-3, 1e-2)          # 16-bit outputs


def bar(ref, tol):
    return tol[0] + tol[1] * (ref.abs().max().item() if ref.numel() else 0.0)


# ------------------------------------------------------------------------------------------------------ MLM compaction
def mlm_case(n, rate, n_split, V, seed=0):
    """labels [n] with ~rate labelled, a few out-of-range ones (-1 = ignore, -7 and >= V are ignored too), src_rows with -1 entries;
    when 0 < n_split < n the positions n_split - 1 and n_split are both labelled (so an off-by-one split changes the counts)."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, V, (n,), generator=g)
    lab = torch.rand(n, generator=g) < rate
    labels[~lab] = -1
    if n > 8 and 0 < rate < 1:
        bad = torch.randperm(n, generator=g)[:max(2, n // 50)]
        labels[bad[0::3]] = V
        labels[bad[1::3]] = V + 1000
        labels[bad[2::3]] = -7
    if 0 < n_split < n and rate > 0:
        labels[n_split - 1], labels[n_split] = 3, V - 1
    src = torch.randperm(n, generator=g).to(torch.int32)
    src[torch.rand(n, generator=g) < 0.1] = -1
    return labels, src


def mlm_compact_ref(labels, src_rows, n_split, V, cap, mutant=None):
    """Stable ascending list of the positions with 0 <= label < V, cut at cap; the counts are those of the kept entries."""
    lab = labels.numpy()
    pos = np.nonzero((lab >= 0) & (lab < V))[0]
    if mutant == "unstable" and len(pos) > 1:
        pos = pos.copy()
        pos[[0, -1]] = pos[[-1, 0]]
    total = len(pos)
    kept = min(total, cap)
    sel_pos = np.full(cap, -1, dtype=np.int32)
    sel_src = np.full(cap, -1, dtype=np.int32)
    labels_c = np.full(cap, -1, dtype=np.int64)
    sel_pos[:kept] = pos[:kept]
    sel_src[:kept] = src_rows.numpy()[pos[:kept]]
    labels_c[:kept] = lab[pos[:kept]]
    n0 = int((pos[:kept] <= n_split).sum() if mutant == "split_off_by_one" else (pos[:kept] < n_split).sum())
    return dict(sel_pos=torch.from_numpy(sel_pos), sel_src=torch.from_numpy(sel_src), labels_c=torch.from_numpy(labels_c),
                count0=torch.tensor([float(n0)]), count1=torch.tensor([float(kept - n0)]),
                overflow=torch.tensor([int(total > cap)], dtype=torch.int32), total=total)


# ------------------------------------------------------------------------------------------------------ attention
def attn_masks(B, S, seed=0):
    """[B,S] 0/1 key masks, sample b by b % 5: 0 full | 1 non-prefix with holes (about half the keys, first key masked when S > 1)
    | 2 one key only (not key 0 when S > 1) | 3 all zero | 4 prefix of length 1.  Also the kind of every sample."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(B, S)
    kinds = []
    for b in range(B):
        k = b % 5
        kinds.append(k)
        if k == 0:
            m[b] = 1
        elif k == 1:
            row = (torch.rand(S, generator=g) < 0.5).float()
            row[0] = 0
            row[S - 1] = 1
            m[b] = row
        elif k == 2:
            m[b, int(torch.randint(1, S, (1,), generator=g)) if S > 1 else 0] = 1
        elif k == 4:
            m[b, 0] = 1
    return m, kinds


def attn_drop_index(B, nh, S, mutant=None):
    """element index of probability (b, h, q, k): ((b*nh + h)*S + q)*S + k"""
    Sk = (S + 31) // 32 * 32 if mutant == "key_stride_32" else S
    row = np.arange(B * nh * S, dtype=np.int64)
    return (row[:, None] * Sk + np.arange(S)[None, :]).reshape(-1)


def attn_ref(qkv, mask, B, S, H, nh, keep=None, dctx=None):
    """BertSelfAttention in float64 (d = H / nh): scores / sqrt(d) + (1 - mask) * -10000, softmax, optional keep x scale, P V.
    Returns ctx [B*S,H], lse [B,nh,S] and, when dctx is given, d(qkv)."""
    d = H // nh
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = [t.view(B, S, nh, d).permute(0, 2, 1, 3) for t in x.view(B, S, 3, H).unbind(2)]
    sc = q @ k.transpose(-1, -2) / math.sqrt(d) + ((1 - mask.double()) * -10000.0)[:, None, None, :]
    p = torch.softmax(sc, -1)
    lse = torch.logsumexp(sc, -1)
    if keep is not None:
        p = p * keep
    ctx = (p @ v).permute(0, 2, 1, 3).reshape(B * S, H)
    grad = None
    if dctx is not None:
        ctx.backward(dctx.double())
        grad = x.grad
    return ctx.detach(), lse.detach(), grad


def attn_groups(mask, kinds, S):
    """Row selectors over [B*S]: live positions of the samples with several live keys; their masked positions; all positions of the
    samples with ONE live key (softmax over one key: d(scores) = 0, so dq and dk are exactly zero in the reference); all positions
    of the all-zero-mask samples (whose gradients are of normal size: every score gets the same -10000)."""
    B = mask.shape[0]
    sel = lambda ks: torch.tensor([k in ks for k in kinds])[:, None].expand(B, S)
    many, one, allzero = sel((0, 1)), sel((2, 4)), sel((3,))
    return {"live": ((mask > 0) & many).reshape(-1), "masked": ((mask == 0) & many).reshape(-1),
            "one-key samples": one.reshape(-1), "all-zero sample": allzero.reshape(-1)}

def attn_rounded_f32(qkv, mask, B, S, H, nh, dtype, keep=None, dctx=None):
    """fp32 CPU restatement of the attention kernels' arithmetic that rounds where they round: P x keep and dS go to the 16-bit type
    before their products, the saved ctx is 16-bit and D = rowsum(dO * O) is taken from that ROUNDED ctx, everything else fp32.
    Not a reference: its distance to attn_ref on the same inputs is the error the number formats alone produce, which sets the bar
    of a destination whose reference value is a cancellation (one live key: dS = P (dP - D) = 0 exactly)."""
    rd = rounder(dtype)
    d = H // nh
    q, k, v = [t.view(B, S, nh, d).permute(0, 2, 1, 3).float() for t in qkv.view(B, S, 3, H).unbind(2)]
    do = dctx.view(B, S, nh, d).permute(0, 2, 1, 3).float()
    kp = torch.ones(B, nh, S, S) if keep is None else keep.float()
    sc = q @ k.transpose(-1, -2) * 0.125 + ((1 - mask) * -10000.0)[:, None, None, :]
    p = torch.softmax(sc, -1)
    pd = rd(p * kp)
    o = rd(pd @ v)
    dD = (do * o).sum(-1, keepdim=True)
    ds = rd(p * ((do @ v.transpose(-1, -2)) * kp - dD))
    dq, dk, dv = rd(ds @ k * 0.125), rd(ds.transpose(-1, -2) @ q * 0.125), rd(pd.transpose(-1, -2) @ do)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, H)
    return flat(o), torch.cat((flat(dq), flat(dk), flat(dv)), 1)
