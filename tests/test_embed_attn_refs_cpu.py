"""The float64 references of tests/test_embed_attn_ops_gpu.py bite: each deliberately wrong statement of an operation, compared
reference against reference on the CPU on the very inputs the GPU tests use, misses the bar of the sub-tensor it concerns by at
least 10x.  So a kernel with that defect cannot pass the GPU battery, and the chosen inputs make every term matter (both type ids
present, table rows far apart, the position clamp actually reached)."""
import numpy as np
import pytest
import torch

from tests import embed_attn_refs as R
from tests.gpu_util import drop_scale, drop_thr, keep_mask

DT = torch.bfloat16      # the default build's 16-bit type (the input values only differ in rounding on the fp16 build)


def miss(ref, bad, tol):
    """how many bars the wrong statement is away from the reference on this sub-tensor"""
    return (bad.double() - ref.double()).abs().max().item() / R.bar(ref, tol)


@pytest.mark.parametrize("case,mutant,parts", [
    ("mod-h128", "type1_to_0", ["d_type row1", "d_type row0"]),
    ("mod-h2048", "type1_to_0", ["d_type row1", "d_type row0"]),
    ("pre-h128", "table_swapped", ["d_ling table row0", "d_ling table row1"]),
    ("pre-h320", "table_swapped", ["d_ling table row0", "d_ling table row1"]),       # all objects select row 0
    ("pre-b520", "table_swapped", ["d_ling table row0", "d_ling table row1"]),
    ("pre-h768", "pos_not_clamped", ["d_pos object rows"]),
    ("mod-h768", "pos_not_clamped", ["d_pos object rows"]),
    ("pre-b520-z", "pos_not_clamped", ["d_pos object rows"]),
    ("pre-h128", "obj_pos_is_s", ["d_pos object rows"]),
    ("mod-b520", "obj_pos_is_s", ["d_pos object rows"]),
])
def test_wrong_embedding_statements_miss_the_bar(case, mutant, parts):
    c = R.embed_case(case, DT)
    fwd, g = R.embed_ref(c)
    fwd_bad, g_bad = R.embed_ref(c, mutant=mutant)
    m = miss(fwd["pre"], fwd_bad["pre"], R.ACT16_TOL)
    print("%s / %s: forward pre misses by %.0f bars" % (case, mutant, m))
    assert m >= 10
    p, p_bad = R.embed_parts(c, g), R.embed_parts(c, g_bad)
    for nm in parts:
        m = miss(p[nm], p_bad[nm], R.FP32_GRAD_TOL)
        print("%s / %s: %s misses by %.0f bars" % (case, mutant, nm, m))
        assert m >= 10, nm


@pytest.mark.parametrize("case", sorted(R.EMBED_CASES))
def test_embedding_inputs_make_every_term_matter(case):
    c = R.embed_case(case, DT)
    B, T, Rr, S, P, V = (c[k] for k in ("B", "T", "R", "S", "P", "V"))
    tl, no = c["tl"], c["no"]
    assert int(no[1]) == 0 and int(tl[0]) == T and int(no[0]) == Rr             # a sample without objects, a completely full one
    assert S >= T + Rr + 1 and (c["kind"][0] == R.KIND_PAD).sum() == S - T - Rr - 1
    ids = c["text_ids"][c["text_mask"]]
    assert (ids < 0).any() and (ids >= V).any()                                  # both clamps of the token id
    assert (~c["obj_mask"][1:]).any()                                            # padded boxes (untouched gradient rows)
    if c["text_type"] is not None:
        for b in range(B):
            present = set(c["text_type"][b][c["text_mask"][b]].tolist())
            assert {0, 1} <= present, b
        assert (2 in R.EMBED_CASES[case][9]) == bool((c["text_type"][c["text_mask"]] == 2).any())
    else:
        assert (c["obj_ling"][0] - c["obj_ling"][1]).abs().max() > 1.0           # table rows far apart
        sel = c["ling_idx"][c["obj_mask"]]
        assert {"mix": {0, 1}, "all0": {0}, "all1": {1}}[R.EMBED_CASES[case][8]] == set(sel.tolist())
    if P < T + Rr + 1:                                                           # the clamp is reached by object and end rows
        assert ((tl >= P) & (no > 0)).any() and (tl + 1 >= P).any()
    else:
        assert c["P"] > int((tl + 1).max()) + 1                                  # position rows past the longest sample exist
    un = R.embed_untouched(c)
    assert un["obj"].any() and (V < 64 or B > 64 or un["word"].sum() > V // 2) and (P < T + Rr + 1 or un["pos"].any())
    # every separately reported backward part is O(0.1 - 10^2): the absolute term of the bar (2e-3) is not what lets it pass
    _, g = R.embed_ref(c)
    ling = R.EMBED_CASES[case][8]
    for nm, t in R.embed_parts(c, g).items():
        mx = t.abs().max().item()
        exact_zero = ((nm == "d_ling table row1" and ling == "all0") or (nm == "d_ling table row0" and ling == "all1") or
                      (nm == "d_type row1" and c["text_type"] is None))
        if exact_zero:
            assert mx == 0.0, nm
        else:
            assert 0.1 <= mx <= 500, (nm, mx)


@pytest.mark.parametrize("n,n_split", [(640, 300), (25600, 12345), (65537, 40000)])
def test_wrong_compaction_statements_differ(n, n_split):
    V = 30522
    labels, src = R.mlm_case(n, 0.15, n_split, V, seed=n)
    ref = R.mlm_compact_ref(labels, src, n_split, V, cap=n)
    assert labels[n_split] >= 0 and labels[n_split - 1] >= 0 and ((labels >= V).any() and (labels < -1).any())
    per = (n + 1023) // 1024
    assert per == 1 or n_split % per != 0                                        # the split lies strictly inside a thread's run
    bad = R.mlm_compact_ref(labels, src, n_split, V, cap=n, mutant="unstable")
    assert not torch.equal(bad["sel_pos"], ref["sel_pos"]) and not torch.equal(bad["labels_c"], ref["labels_c"])
    bad = R.mlm_compact_ref(labels, src, n_split, V, cap=n, mutant="split_off_by_one")
    assert not torch.equal(bad["count0"], ref["count0"]) and not torch.equal(bad["count1"], ref["count1"])


@pytest.mark.parametrize("S", [17, 33, 97, 130])
def test_wrong_attention_mask_statement_misses_the_bar(S):
    B, nh = 5, 2
    H = nh * 64
    rd = R.rounder(DT)
    g = torch.Generator().manual_seed(S)
    qkv, dctx = rd(torch.randn(B * S, 3 * H, generator=g)), rd(torch.randn(B * S, H, generator=g))
    mask, kinds = R.attn_masks(B, S, seed=S)
    ctx, lse, grad = R.attn_ref(qkv, mask, B, S, H, nh, dctx=dctx)
    assert torch.isfinite(ctx).all() and torch.isfinite(grad).all()              # the all-zero mask row is a plain softmax
    prefix = mask.clone()                                                        # the holed mask as a prefix mask of the same length
    n = int(mask[1].sum())
    prefix[1] = (torch.arange(S) < n).float()
    assert 0 < n < S and not torch.equal(prefix[1], mask[1])
    ctx_b, lse_b, grad_b = R.attn_ref(qkv, prefix, B, S, H, nh, dctx=dctx)
    rows = slice(S, 2 * S)
    assert miss(ctx[rows], ctx_b[rows], (2e-3, 1e-2)) >= 10
    assert miss(lse[1], lse_b[1], (2e-3, 1e-3)) >= 10
    for j in range(3):
        assert miss(grad[rows, j * H:(j + 1) * H], grad_b[rows, j * H:(j + 1) * H], (2e-3, 2e-2)) >= 10, j


@pytest.mark.parametrize("S", [33, 130])
def test_wrong_attention_dropout_index_misses_the_bar(S):
    B, nh, p = 5, 2, 0.1
    H = nh * 64
    rd = R.rounder(DT)
    g = torch.Generator().manual_seed(S)
    qkv, dctx = rd(torch.randn(B * S, 3 * H, generator=g)), rd(torch.randn(B * S, H, generator=g))
    mask, kinds = R.attn_masks(B, S, seed=S)
    thr = drop_thr(p)
    out = []
    for mutant in (None, "key_stride_32"):
        keep = keep_mask(777, 3, R.attn_drop_index(B, nh, S, mutant), thr).reshape(B, nh, S, S)
        keep = torch.from_numpy(keep.astype(np.float64)) * drop_scale(thr)
        out.append(R.attn_ref(qkv, mask, B, S, H, nh, keep=keep, dctx=dctx))
    (ctx, _, grad), (ctx_b, _, grad_b) = out
    assert miss(ctx, ctx_b, (2e-3, 1e-2)) >= 10
    for j in range(3):
        assert miss(grad[:, j * H:(j + 1) * H], grad_b[:, j * H:(j + 1) * H], (2e-3, 2e-2)) >= 10, j
