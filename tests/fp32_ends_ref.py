"""Input builders and float64 CPU reference statements for the fp32 front / back end kernels (vl-bert_amd/csrc/f32_ends.hip) and the
fp32 classifier head (vl-bert_amd/common/heads.py: Head32), shared by tests/test_fp32_ends_gpu.py.

The embedding case has the key set of tests/embed_attn_refs.embed_case (module form), so embed_ref / embed_untouched of that file state
the reference; its values are plain fp32 (nothing is rounded to a 16-bit type)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.embed_attn_refs import EMBED_SEED, KIND_PAD, seq_layout_ref
from tests.gpu_util import TAG_EMBED, drop_scale, drop_thr, keep_mask

EMBED32_B, EMBED32_T, EMBED32_R = 3, 7, 5


def embed_case32(H, S, p, seed=0):
    """B = 3, T = 7, R = 5, ragged: sample 0 has every token and all five objects, sample 1 is `[CLS] x [SEP]` with a single object,
    sample 2 has five tokens and three objects with a hole between them.  One token id below 0 and one >= V (clamped); token types
    cover {0, 1, 2}.  S = 13 is the packed length T + R + 1, S = 16 the engine-padded one (trailing pad rows in every sample)."""
    B, T, R, V, P = EMBED32_B, EMBED32_T, EMBED32_R, 50, (8 if H == 64 else 32)      # P = 8: positions clamp to P - 1
    assert S >= T + R + 1
    g = torch.Generator().manual_seed(7000 + seed)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).float()
    text_mask = torch.arange(T)[None, :] < torch.tensor([T, 3, 5])[:, None]
    obj_mask = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 0, 0], [1, 0, 1, 1, 0]], dtype=torch.bool)
    text_ids = torch.randint(0, V - 10, (B, T), generator=g)          # ids V-10 .. V-2 stay untouched
    text_ids[0, 2], text_ids[2, 1] = -4, V + 7                        # clamped to 0 / V - 1
    tt = torch.randint(0, 2, (B, T), generator=g)
    tt[:, 0], tt[:, 1], tt[0, 3] = 0, 1, 2
    c = dict(name="f32-h%d-s%d-p%g" % (H, S, p), mode="module", H=H, B=B, T=T, R=R, S=S, P=P, V=V, p=p, zeroed=False, text_mask=text_mask,
             obj_mask=obj_mask, text_ids=text_ids, word=rn(V, H), pos=rn(P, H), type=rn(3, H), end=rn(1, H),
             gamma=(1.0 + 0.2 * torch.randn(H, generator=g)).float(), beta=(0.2 * torch.randn(H, generator=g)).float(),
             obj_vis=rn(B, R, H), text_type=tt, text_vis=rn(B, T, H), obj_ling=rn(B, R, H), ling_idx=None)
    c["kind"], c["idx"], c["tl"], c["no"] = seq_layout_ref(text_mask, obj_mask, S)
    c["dy"] = (torch.randn(B, S, H, generator=g) * (c["kind"] != KIND_PAD)[..., None]).float()     # pad rows reach no loss
    thr = drop_thr(p)
    c["keep"] = None
    if thr:
        keep = keep_mask(EMBED_SEED, TAG_EMBED, np.arange(B * S * H), thr).reshape(B, S, H)
        c["keep"] = torch.from_numpy(keep.astype(np.float64)) * drop_scale(thr)
    return c


def keep_scale(seed, tag, n, p):
    """float64 [n]: keep bit x the device's scale for element indices 0 .. n - 1 (all ones for p = 0)."""
    thr = drop_thr(p)
    if not thr:
        return torch.ones(n, dtype=torch.float64)
    return torch.from_numpy(keep_mask(seed, tag, np.arange(n), thr).astype(np.float64)) * drop_scale(thr)


def obj_prep_ref(boxes, im_info, seed, tag, p):
    """common/utils/bbox.py:33-65 + common/fast_rcnn.py:165-175 in float64: [B*R, 4096] = dropout(coordinate embedding || feature);
    rows of padded boxes (x1 <= -1.5) zero.  Element index of the mask: row * 4096 + column."""
    B, R, _ = boxes.shape
    bx = boxes.double()
    w, h = im_info[:, 0].double()[:, None], im_info[:, 1].double()[:, None]
    pos = torch.stack(((bx[..., 0] + bx[..., 2]) / 2 / w * 100, (bx[..., 1] + bx[..., 3]) / 2 / h * 100,
                       (bx[..., 2] - bx[..., 0]) / w * 100, (bx[..., 3] - bx[..., 1]) / h * 100), -1)          # [B, R, 4]
    dim = 1000.0 ** (torch.arange(256, dtype=torch.float64) / 256.0)
    ang = pos[..., None] / dim                                                                                     # [B, R, 4, 256]
    coord = torch.cat((ang.sin(), ang.cos()), -1).reshape(B, R, 2048)
    out = torch.cat((coord, bx[..., 4:]), -1).reshape(B * R, 4096)
    out = out * keep_scale(seed, tag, B * R * 4096, p).reshape(B * R, 4096)
    return out * (bx[..., 0] > -1.5).reshape(B * R, 1)


def bce_ref(logits, label, pos_weight=1.0, gscale=1.0):
    """-> (loss, gscale * d loss / d logits) in float64: (1 / rows) sum w (max(x, 0) - x y + log(1 + exp(-|x|))), w = pos_weight where
    y > 0.5 (what F.binary_cross_entropy_with_logits(x, y, weight=w) * A gives)."""
    x = logits.double().clone().requires_grad_(True)
    y = label.double()
    w = torch.where(y > 0.5, torch.tensor(pos_weight, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    loss = F.binary_cross_entropy_with_logits(x, y, weight=w) * x.shape[1]
    (gscale * loss).backward()
    return loss.detach(), x.grad


def head_ref(classifier, P, x, label, p, seed, tags, g=1.0):
    """final_mlp of vqa/modules/resnet_vlbert_for_vqa.py:54-74 + the BCE of :226 in float64, dropout under the device's masks (element
    index = row * width + column of the contiguous activation).  P: parameters by the mirror's names.  -> (logits, loss, d x,
    {name: gradient}) of g * loss."""
    L = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
    xd = x.double().clone().requires_grad_(True)
    n = x.shape[0]
    drop = lambda t, tag: t * keep_scale(seed, tag, t.numel(), p).reshape(t.shape)
    if classifier == "2fc":
        h = torch.relu(F.linear(drop(xd, tags[0]), L["1.weight"], L["1.bias"]))
        logits = F.linear(drop(h, tags[1]), L["4.weight"], L["4.bias"])
    elif classifier == "1fc":
        logits = F.linear(drop(xd, tags[0]), L["1.weight"], L["1.bias"])
    else:
        u = F.linear(xd, L["0.dense.weight"], L["0.dense.bias"])
        h = u * 0.5 * (1.0 + torch.erf(u / 2.0 ** 0.5))
        mean = h.mean(-1, keepdim=True)
        h = (h - mean) / torch.sqrt(h.var(-1, unbiased=False, keepdim=True) + 1e-12) * L["0.LayerNorm.weight"] + L["0.LayerNorm.bias"]
        logits = F.linear(drop(h, tags[1]), L["2.weight"], L["2.bias"])
    loss = F.binary_cross_entropy_with_logits(logits, label.double()) * label.shape[1]
    (g * loss).backward()
    assert logits.shape[0] == n
    return logits.detach(), loss.detach(), xd.grad, {k: v.grad for k, v in L.items()}
