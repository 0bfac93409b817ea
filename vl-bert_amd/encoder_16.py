"""16-bit encoder of the engine (engine.PretrainEngine.encoder unless encoder_fp32): the layer loop of the forward and of the explicit
backward on the fused HIP kernels, with every buffer only that loop touches -- activations, backward scratch, the transposed weight
copies of its dgrad GEMMs and the weight-gradient operand sets.

Replaces external/pytorch_pretrained_bert/modeling.py:268-397 (BertSelfAttention / BertSelfOutput / BertIntermediate / BertOutput, 12 or
24 times) and its autograd backward.  The engine supplies the shared services: flat parameters (w16 / w32 / g32), `lay`, the dropout
seed, the side stream for weight gradients (_on_side / _before_write / _join_side), the deferred LayerNorm finalize (_ln_bwd) and the
gradient buckets, which are read at call time (a step-graph capture swaps them).
"""
import os
from types import SimpleNamespace

import torch

from . import ops
from .engine import F32, _ru


class Encoder16:
    def __init__(self, eng):
        self.eng = eng
        cfg, d = eng.cfg, eng.dev
        H, I, L, nh = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads
        M, S, Bt = eng.M, eng.S, eng.Bt

        def zb(*s):
            return torch.zeros(s, dtype=ops.BF16, device=d)

        def zf(*s):
            return torch.zeros(s, dtype=F32, device=d)

        # bf16 transposed weights for dgrad GEMMs (dX = dY . (W^T)^T); refreshed after every optimizer step
        self.wT = {}
        for l in range(L):
            p = "vlbert.encoder.layer.%d." % l
            self.wT[p + "qkv"] = zb(H, 3 * H)
            self.wT[p + "attention.output.dense.weight"] = zb(H, H)
            self.wT[p + "intermediate.dense.weight"] = zb(H, I)
            self.wT[p + "output.dense.weight"] = zb(I, H)
        self.layer = [self._layer_record(l) for l in range(L)]
        # Operands of the per-layer weight gradients are allocated with their row count rounded up to 128 (the pad rows stay zero:
        # every kernel writes M rows) and used through [:M] views; the grouped large-tile wgrad (gemm_tn8.hip, K tiles of 128 rows)
        # gets the padded tensors, so it also serves the per-GPU batches of a strong-scaling run (M = 3232 at 32 samples).
        self.Mp128 = _ru(M, 128)
        self._row_padded = {}

        def zbm(cols):
            full = zb(self.Mp128, cols)
            view = full[:M]
            self._row_padded[view.data_ptr()] = full
            return view
        self.X = [zbm(H) for _ in range(L + 1)]
        self.QKV = [zb(M, 3 * H) for _ in range(L)]
        self.CTX = [zbm(H) for _ in range(L)]
        self.LSE = [zf(Bt, nh, S) for _ in range(L)]
        # Residual stream precision (DESIGN.md "precision"): the pre-LayerNorm sums Z1 / Z2 are kept in fp16 (3 more mantissa bits
        # than bf16, same bytes; |Z| = O(1..10)) and the residual a sublayer adds is the previous LayerNorm's output re-materialised
        # in fp32 from (Z, mean, rstd, gamma, beta) inside the GEMM epilogue, so nothing on the residual path is ever rounded to
        # bf16 -- only the GEMM operands are.  At 12 layers this takes the logits' error against the fp32 reference from 1.3e-2 to
        # ~6e-3 (relative Frobenius; 5e-3 of it is the bf16 rounding of the weights).  VLB_RESIDUAL_STREAM=bf16: the old behaviour.
        self.hp_res = os.environ.get("VLB_RESIDUAL_STREAM", "f16ln") != "bf16"
        zdt = torch.float16 if self.hp_res else ops.BF16
        zz = lambda *s: torch.zeros(s, dtype=zdt, device=d)
        self.Z1, self.ST1, self.Y1 = [zz(M, H) for _ in range(L)], [zf(M, 2) for _ in range(L)], [zbm(H) for _ in range(L)]
        self.U, self.G = [zb(M, I) for _ in range(L)], [zbm(I) for _ in range(L)]
        self.Z2, self.ST2 = [zz(M, H) for _ in range(L)], [zf(M, 2) for _ in range(L)]
        # backward scratch
        self.dXa, self.dXb = zb(M, H), zb(M, H)
        # The four weight gradients of a layer go out as ONE grouped launch at the end of the layer's backward (side stream), so their
        # gradient operands (LN2 / LN1 outputs through dropout, dU, dQKV) stay alive until then and are double-buffered by layer
        # parity: the next layer writes the other set while the group still reads this one.
        self.dZ = zb(M, H)
        # Round 6: the weight gradients of TWO layers go out as one table launch of full-K work items (216 items for 256 CUs like the
        # grouped launch of one layer, but no K slices: no fp32 slabs, no reduce launch) -- the upper layer of a pair keeps its operands
        # until the lower one is done, so there are four sets (layer & 3) instead of two.  VLB_WGRAD_PAIRS=0: one grouped launch per layer.
        self._pairs = os.environ.get("VLB_WGRAD_PAIRS", "1") != "0"
        self._pair_tables = {}
        nset = 4 if self._pairs else 2
        self.dD2, self.dD1 = [zbm(H) for _ in range(nset)], [zbm(H) for _ in range(nset)]
        self.dU2 = [zbm(I) for _ in range(nset)]
        self.dQKV2 = [zbm(3 * H) for _ in range(nset)]
        self.dCTX = zb(M, H)
        # what the neighbours touch: the front end writes x_in, the heads read x_out and leave d X[L] in dx_in
        self.x_in, self.x_out, self.dx_in = self.X[0], self.X[L], self.dXa

    # -- parameters ---------------------------------------------------------------------------------------------------
    def _layer_record(self, l):
        """Views of encoder layer l's parameters in the flat buffers, built once (nothing rebinds P.master / P.grad / P.w16): per Linear
        (qkv = the fused [3H,H] operand, ao, f1, f2) w (16-bit) / b (fp32) / gw / gb / wT, per LayerNorm (ln1, ln2) g / b / gg / gb."""
        e = self.eng
        P, H, p = e.P, e.cfg.hidden_size, "vlbert.encoder.layer.%d." % l
        q = p + "attention.self.query."
        rec = SimpleNamespace(qkv=SimpleNamespace(
            w=P.view(P.w16, q + "weight", (3 * H, H), span=3), b=P.view(P.master, q + "bias", (3 * H,), span=3),
            gw=P.view(P.grad, q + "weight", (3 * H, H), span=3), gb=P.view(P.grad, q + "bias", (3 * H,), span=3), wT=self.wT[p + "qkv"]))
        for k, n in (("ao", "attention.output.dense."), ("f1", "intermediate.dense."), ("f2", "output.dense.")):
            setattr(rec, k, SimpleNamespace(w=e.w16[p + n + "weight"], b=e.w32[p + n + "bias"], gw=e.g32[p + n + "weight"],
                                            gb=e.g32[p + n + "bias"], wT=self.wT[p + n + "weight"]))
        for k, n in (("ln1", "attention.output.LayerNorm."), ("ln2", "output.LayerNorm.")):
            setattr(rec, k, SimpleNamespace(g=e.w32[p + n + "weight"], b=e.w32[p + n + "bias"], gg=e.g32[p + n + "weight"],
                                            gb=e.g32[p + n + "bias"]))
        return rec

    def transposes(self):
        """[(16-bit weight, its W^T copy)] for the engine's one batched transpose."""
        return [(lin.w, lin.wT) for r in self.layer for lin in (r.qkv, r.ao, r.f1, r.f2)]

    def refresh(self):
        pass

    def overwritten(self):
        """Parameters whose gradient is produced (whole tensor) by exactly one weight-gradient product per backward."""
        names = []
        for l in range(len(self.layer)):
            p = "vlbert.encoder.layer.%d." % l
            names += [p + "attention.self.query.weight", p + "attention.self.key.weight", p + "attention.self.value.weight",
                      p + "attention.output.dense.weight", p + "intermediate.dense.weight", p + "output.dense.weight"]
        return names

    # -- forward ------------------------------------------------------------------------------------------------------
    def forward(self, p_h, p_a):
        """X[0] (the embedding output) -> X[L]."""
        e = self.eng
        H, nh, S, Bt = e.cfg.hidden_size, e.cfg.num_attention_heads, e.S, e.Bt
        seed, mask = e.seed, e.lay["attn_mask"]
        stale = e._gather_pending
        for l, r in enumerate(self.layer):
            x = self.X[l]
            if stale:
                e.buckets.wait_params(l)
            ops.gemm_nt(x, r.qkv.w, self.QKV[l], bias=r.qkv.b)
            ops.attention_fwd(self.QKV[l], mask, self.CTX[l], self.LSE[l], Bt, S, H, nh, drop_p=p_a, seed=seed, tag=l * 8 + 0)
            if self.hp_res and l > 0:    # residual = LayerNorm(Z2[l-1]) in fp32 (layer 0: the bf16 embedding output, one rounding)
                ln = self.layer[l - 1].ln2
                res_kw = dict(res=self.Z2[l - 1], res_ln=(self.ST2[l - 1], ln.g, ln.b))
            else:
                res_kw = dict(res=x)
            ops.gemm_nt(self.CTX[l], r.ao.w, self.Z1[l], bias=r.ao.b, drop_p=p_h, seed=seed, tag=l * 8 + 1, **res_kw)
            ops.layernorm_fwd(self.Z1[l], r.ln1.g, r.ln1.b, self.Y1[l], self.ST1[l])
            ops.gemm_nt(self.Y1[l], r.f1.w, self.G[l], bias=r.f1.b, act=ops.ACT_GELU_D, pre=self.U[l])
            if self.hp_res:
                res_kw = dict(res=self.Z1[l], res_ln=(self.ST1[l], r.ln1.g, r.ln1.b))
            else:
                res_kw = dict(res=self.Y1[l])
            ops.gemm_nt(self.G[l], r.f2.w, self.Z2[l], bias=r.f2.b, drop_p=p_h, seed=seed, tag=l * 8 + 2, **res_kw)
            ops.layernorm_fwd(self.Z2[l], r.ln2.g, r.ln2.b, self.X[l + 1], self.ST2[l])

    # -- backward (weight gradients on the engine's side stream) --------------------------------------------------------
    def _padded(self, items):
        """items with their row-padded operands (zero pad rows): K a multiple of 128 for the large-tile kernels."""
        pad = self._row_padded
        return [(pad.get(dy.data_ptr(), dy), pad.get(x.data_ptr(), x), gw, gb) for dy, x, gw, gb in items]

    def _wgrad_group(self, items):
        """items: [(dy, x, gw, gb)] over the same rows -- the four Linear layers of an encoder layer -- as one grouped launch on the
        side stream (ops.wgrad_tn_group)."""
        e = self.eng
        acc = not e._fresh_grads
        items = self._padded(items)
        if len({t.shape[0] for it in items for t in it[:2]}) != 1:
            items = [(dy[:e.M], x[:e.M], gw, gb) for dy, x, gw, gb in items]
        e._on_side(lambda: ops.wgrad_tn_group(items, workspace=e.wg_ws, accumulate=acc), items)

    def _wgrad_pair(self, items):
        """items: [(dy, x, gw, gb)] of TWO encoder layers (8 products over the same rows) as ONE table launch of full-K 256 x 256 work
        items on the side stream (ops.WgradTable: no K slices, no slabs, no reduce).  The descriptor table of a pair is built once per
        (buffers, accumulate) and replayed.  False: not taken (a product outside what the table kernel covers, or a table that would
        have to be built during stream capture) -- the caller falls back to one grouped launch per layer."""
        e = self.eng
        acc = not e._fresh_grads
        items = self._padded(items)
        key = (acc,) + tuple(t.data_ptr() for it in items for t in it)
        tab = self._pair_tables.get(key)
        if tab is None:
            if e.dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                return False
            if len({t.shape[0] for it in items for t in it[:2]}) != 1:
                return False
            tab = ops.WgradTable([(dy, x, gw, gb, None) for dy, x, gw, gb in items], e.dev, accumulate=acc)
            self._pair_tables[key] = tab
        if not tab.ok:
            return False
        e._on_side(lambda: tab.run(), items)
        return True

    def backward(self, dx, p_h, p_a, on_layer_done=None, will_launch=None):
        """dx: d X[L] in dXa -> weight gradients into the engine's flat fp32 gradient (side stream); returns d X[0] (dXa or dXb)."""
        e = self.eng
        H, nh, S, Bt = e.cfg.hidden_size, e.cfg.num_attention_heads, e.S, e.Bt
        seed, mask = e.seed, e.lay["attn_mask"]
        held = None      # (layer, weight-gradient items) of an odd layer waiting for the layer below it (self._pairs)
        for l in reversed(range(len(self.layer))):
            r = self.layer[l]
            dx_next = self.dXb if dx is self.dXa else self.dXa
            par = l & (len(self.dD2) - 1)
            dD2, dD1, dU, dQKV = self.dD2[par], self.dD1[par], self.dU2[par], self.dQKV2[par]
            # LN2: dZ2 (residual branch) and dD2 (into output.dense, through its dropout; a plain copy when dropout is off --
            # dZ is reused inside the layer, the grouped weight gradient at its end needs its own operand)
            e._before_write(self.dZ, dD2)
            e._ln_bwd(dx, self.Z2[l], self.ST2[l], r.ln2.g, r.ln2.gg, r.ln2.gb, dx=self.dZ, dx_drop=dD2, drop_p=p_h, seed=seed,
                      tag=l * 8 + 2)
            e._before_write(dU)
            ops.gemm_nt(dD2, r.f2.wT, dU, act=ops.ACT_MULAUX, aux=self.U[l])
            ops.gemm_nt(dU, r.f1.wT, dx_next, res=self.dZ)                                         # dY1
            # LN1
            e._before_write(self.dZ, dD1)
            e._ln_bwd(dx_next, self.Z1[l], self.ST1[l], r.ln1.g, r.ln1.gg, r.ln1.gb, dx=self.dZ, dx_drop=dD1, drop_p=p_h, seed=seed,
                      tag=l * 8 + 1)
            ops.gemm_nt(dD1, r.ao.wT, self.dCTX)
            e._before_write(dQKV)
            ops.attention_bwd(self.QKV[l], mask, self.CTX[l], self.LSE[l], self.dCTX, dQKV, Bt, S, H, nh, drop_p=p_a,
                              seed=seed, tag=l * 8 + 0)
            ops.gemm_nt(dQKV, r.qkv.wT, dx_next, res=self.dZ)                                      # dX_l (overwrites dY1)
            # the layer's four weight gradients on the side stream, off the critical dgrad chain: with the layer below as ONE table launch
            # (an odd layer waits for its partner), or as one grouped launch per layer
            wg = [(dD2, self.G[l], r.f2.gw, r.f2.gb), (dU, self.Y1[l], r.f1.gw, r.f1.gb), (dD1, self.CTX[l], r.ao.gw, r.ao.gb),
                  (dQKV, self.X[l], r.qkv.gw, r.qkv.gb)]
            dx = dx_next
            if self._pairs and (l & 1):
                held = (l, wg)              # (its hook fires behind the pair's launch)
                continue
            finished = [l]
            if held is not None:
                if not self._wgrad_pair(held[1] + wg):
                    self._wgrad_group(held[1])
                    self._wgrad_group(wg)
                finished = [held[0], l]
                held = None
            else:
                self._wgrad_group(wg)
            for lf in finished:
                if on_layer_done and (will_launch is None or will_launch(lf)):
                    e._join_side()       # the bucket's weight gradients must be complete before its all-reduce reads them
                    on_layer_done(lf)
        return dx

    # -- inspection of the last forward: no per-layer state beyond what the forward leaves behind anyway ---------------
    def attention_probs(self, layers, n, seed):
        e, cfg = self.eng, self.eng.cfg
        return [ops.attention_probs(self.QKV[l], e.lay["attn_mask"], self.LSE[l], e.Bt, e.S, cfg.hidden_size,
                                    cfg.num_attention_heads, n=n, drop_p=e._last_p_a, seed=seed, tag=l * 8 + 0) for l in layers]

    def encoded_layers(self, layers, n):
        e = self.eng
        return [self.X[l + 1].view(e.Bt, e.S, e.cfg.hidden_size)[:, :n].float() for l in layers]
