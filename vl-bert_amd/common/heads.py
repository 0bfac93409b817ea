"""What the fine-tuning heads of the module mirrors share: the config getter, the 16-bit working copy of an fp32 master Linear, and ONE
hand-scheduled MLP head -- a list of stages (dropout under a tag, Linear with a fused bias / ReLU / GELU epilogue, LayerNorm) walked
forward, and walked in reverse for the backward (TN weight gradients with the bias column sums, the NT GEMM against W^T with the ReLU
mask fused / the kept GELU' multiplied in / the LayerNorm backward, the dropout replayed under the same tag, one rng_advance).  The loss
stays outside: a head takes a callable that leaves d(logits) in the logits buffer and the value in `loss`."""
import torch

from .. import ops

F32 = torch.float32


def cfg_get(obj, name, default=None):
    return getattr(obj, name, default) if not isinstance(obj, dict) else obj.get(name, default)


def round_up(x, m):
    return (x + m - 1) // m * m


class Linear16:
    """16-bit working copy of the Linear `lin` (a module with the fp32 master `weight` [O, K] and `bias`): W [O, K] and Wt [K, O padded
    to 64], recast and retransposed by sync() when the master's version moved; the padding is exact zeros.  pad_k: W is [O, K padded to
    64] (it multiplies activations whose row stride is padded), written through an unpadded staging image."""

    def __init__(self, lin, pad_k=False):
        self.lin, self.pad_k, self.version = lin, pad_k, None
        O, K = lin.weight.shape
        dev = lin.weight.device
        self.W = torch.zeros((O, round_up(K, 64) if pad_k else K), dtype=ops.BF16, device=dev)
        self.Wt = torch.zeros((K, round_up(O, 64)), dtype=ops.BF16, device=dev)

    weight = property(lambda self: self.lin.weight)
    bias = property(lambda self: self.lin.bias)

    def sync(self):
        w = self.weight
        if self.version == w._version:
            return
        O, K = w.shape
        src = torch.zeros((O, K), dtype=ops.BF16, device=w.device) if self.pad_k else self.W
        ops.cast_f32_bf16(w.detach().contiguous(), src)
        if self.pad_k:
            self.W.zero_()
            self.W[:, :K].copy_(src)
        if O == 1:                                    # one live column of 64 (index plumbing)
            self.Wt.zero_()
            self.Wt[:, 0].copy_(src[0])
        else:
            ops.transpose(src, self.Wt)               # into the zero-padded [K, Op] image
        self.version = w._version


# -- stages: fwd(x, b, p, seed) -> output buffer; bwd(d, b, p, seed) -> (d(input) buffer, parameter gradients).  `b` holds the stage's
#    scratch buffers (widths padded to 64) plus "x", the stage's input of this pass ---------------------------------------------------
class Drop:
    def __init__(self, tag):
        self.tag = tag

    def params(self):
        return []

    def buffers(self, zb, w):
        return dict(y=zb(w), dy=zb(w)), w

    def fwd(self, x, b, p, seed):
        return ops.dropout_bf16(x, b["y"], p, seed, self.tag) if p > 0 else x

    def bwd(self, d, b, p, seed):
        return (ops.dropout_bf16(d, b["dy"], p, seed, self.tag) if p > 0 else d), []


class Linear:
    """act None | "relu" (undone by ACT_RELU_MASK inside the dgrad GEMM of the NEXT Linear, against this one's output) | "gelu" (GELU'
    kept by the epilogue, multiplied in by mul_bf16).  wgrad(dy, x, gw, gb) replaces the TN weight gradient of a Linear whose operands
    need their own staging."""

    def __init__(self, w16, act=None, wgrad=None):
        self.w16, self.act, self.wgrad = w16, act, wgrad

    def params(self):
        return [self.w16.weight, self.w16.bias]

    def buffers(self, zb, w):
        N = self.w16.Wt.shape[1]
        b = dict(out=zb(N), dx=zb(w))
        if self.act == "gelu":
            b.update(pre=zb(N), dpre=zb(N))
        return b, N

    def fwd(self, x, b, p, seed):
        N = self.w16.weight.shape[0]
        act = {None: ops.ACT_NONE, "relu": ops.ACT_RELU, "gelu": ops.ACT_GELU_D}[self.act]
        ops.gemm_nt(x, self.w16.W, b["out"][:, :N], bias=self.w16.bias.detach(), act=act, pre=b.get("pre"))
        return b["out"]

    def bwd(self, d, b, p, seed):
        N, K = self.w16.weight.shape
        if self.act == "gelu":
            d = ops.mul_bf16(d, b["pre"], b["dpre"])
        gw, gb = (torch.zeros_like(q, dtype=F32) for q in self.params())
        if self.wgrad is not None:
            self.wgrad(d, b["x"], gw, gb)
        else:
            ops.wgrad_tn(d[:, :N], b["x"][:, :K], gw, colsum=gb, workspace=None)
        if b["relu"] is not None:                      # K of this GEMM = the padded output width (zero columns)
            ops.gemm_nt(d, self.w16.Wt, b["dx"][:, :K], act=ops.ACT_RELU_MASK, aux=b["relu"][:, :K])
        else:
            ops.gemm_nt(d, self.w16.Wt, b["dx"][:, :K])
        return b["dx"], [gw, gb]


class LayerNorm:
    def __init__(self, ln):
        self.ln = ln

    def params(self):
        return [self.ln.weight, self.ln.bias]

    def buffers(self, zb, w):
        return dict(out=zb(w), dx=zb(w), stats=zb(2, F32)), w

    def fwd(self, x, b, p, seed):
        return ops.layernorm_fwd(x, self.ln.weight.detach(), self.ln.bias.detach(), b["out"], b["stats"])

    def bwd(self, d, b, p, seed):
        gg, gbeta = (torch.zeros_like(q, dtype=F32) for q in self.params())
        ops.layernorm_bwd(d, b["x"], b["stats"], self.ln.weight.detach(), dx=b["dx"], dgamma=gg, dbeta=gbeta)
        return b["dx"], [gg, gbeta]


class Head:
    """stages: the list above, ending in the Linear that writes the logits.  seed: the int32 device counter the dropout sites share.
    row_cap: scratch rows are allocated in multiples of it (heads whose row count changes with every batch).
    loss_fn(logits, logits_copy, loss, g, fresh): logits 16-bit [rows, outputs padded to 64] -> g * d(loss)/d(logits) in place, the
    value added to loss [1]; fresh (the forward) asks for the logits to be kept in logits_copy, from which the backward restores them
    when the upstream factor is not 1."""

    def __init__(self, stages, seed, row_cap=1):
        self.stages, self.seed, self.row_cap, self._states = stages, seed, row_cap, {}

    def params(self):
        return [q for s in self.stages for q in s.params()]

    def _state(self, n, dev):
        cap = round_up(n, self.row_cap)
        if cap not in self._states:
            zb = lambda w, dtype=ops.BF16: torch.zeros((cap, w), dtype=dtype, device=dev)
            w = next(s for s in self.stages if isinstance(s, Linear)).w16.W.shape[1]          # the input width
            st = dict(x=zb(w), loss=torch.zeros((1,), dtype=F32, device=dev), per=[])
            for s in self.stages:
                b, w = s.buffers(zb, w)
                st["per"].append(b)
            st.update(logits=st["per"][-1]["out"], copy=zb(w))
            self._states[cap] = st
        cut = lambda d: {k: (v[:n] if isinstance(v, torch.Tensor) and v.dim() == 2 else v) for k, v in d.items()}
        st = cut(self._states[cap])
        st["per"] = [cut(b) for b in st["per"]]
        return st

    def forward(self, x, p, loss_fn=None):
        """x [rows, K] fp32 -> the pass: "logits" (16-bit; after a loss they hold its gradient and "copy" the logits), "loss" [1]."""
        st = self._state(x.shape[0], x.device)
        for s in self.stages:
            if isinstance(s, Linear):
                s.w16.sync()
        cur, relu = ops.cast_f32_bf16(x.detach().contiguous(), st["x"]), None
        for s, b in zip(self.stages, st["per"]):
            b["x"], b["relu"] = cur, relu
            cur = s.fwd(cur, b, p, self.seed)
            if isinstance(s, Linear):
                relu = cur if s.act == "relu" else None
        st["loss"].zero_()
        if loss_fn is not None:
            loss_fn(st["logits"], st["copy"], st["loss"], 1.0, True)
        st.update(p=p, loss_fn=loss_fn)
        return st

    def backward(self, st, g=1.0):
        """-> (d(x) fp32, the gradients of params() in its order) of g * loss."""
        p, loss_fn = st["p"], st["loss_fn"]
        if loss_fn is None:
            return torch.zeros(st["x"].shape, dtype=F32, device=st["x"].device), [torch.zeros_like(q, dtype=F32) for q in self.params()]
        if g != 1.0:      # upstream scale (loss weights, gradient accumulation, loss scaling): re-derive d(logits) from the kept logits
            st["logits"].copy_(st["copy"])
            st["loss"].zero_()
            loss_fn(st["logits"], st["copy"], st["loss"], g, False)
        d, grads = st["logits"], []
        for s, b in zip(reversed(self.stages), reversed(st["per"])):
            d, gs = s.bwd(d, b, p, self.seed)
            grads = gs + grads
        dx = torch.empty(d.shape, dtype=F32, device=d.device)
        ops.cast_bf16_f32(d.contiguous(), dx)
        if p > 0:
            ops.rng_advance(self.seed)
        return dx, grads


# -- fp32 stages (`fp32_ends`: the classifier behind an fp32 encoder; csrc/f32_path.hip GEMMs + csrc/f32_ends.hip) ---------------------
#    Same walk as above with every buffer fp32.  Widths are padded to 32 (the fp32 GEMM's reduction granularity), padding exact zeros.
class Weight32:
    """fp32 operands of the Linear `lin` (fp32 master `weight` [O, K], `bias`): Wt [K padded, O padded] for the data gradient,
    retransposed by sync() when the master's version moved.  The forward multiplies by the master weight itself; where O or K is not a
    multiple of 32 (3129 answers) by an exact zero-padded fp32 copy of it (and of the bias), refreshed with Wt -- the GEMM reads whole
    groups of rows and columns."""

    def __init__(self, lin):
        self.lin, self.version = lin, None
        self.O, self.K = lin.weight.shape
        self.Op, self.Kp = round_up(self.O, 32), round_up(self.K, 32)
        dev = lin.weight.device
        self.Wt = torch.zeros((self.Kp, self.Op), dtype=F32, device=dev)
        self.padded = (self.Op, self.Kp) != (self.O, self.K)
        if self.padded:
            self.Wp = torch.zeros((self.Op, self.Kp), dtype=F32, device=dev)
            self.bp = torch.zeros((self.Op,), dtype=F32, device=dev)

    weight = property(lambda self: self.lin.weight)
    bias = property(lambda self: self.lin.bias)
    W = property(lambda self: self.Wp if self.padded else self.lin.weight.detach())
    b = property(lambda self: self.bp if self.padded else self.lin.bias.detach())

    def sync(self):
        w, b = self.lin.weight, self.lin.bias
        version = (w._version, b._version)
        if self.version == version:
            return
        wd = w.detach().contiguous()
        ops.transpose_f32(wd, self.K, self.Wt, self.Op, self.O, self.K, self.Op)
        if self.padded:                                # exact copies (data movement)
            self.Wp[:self.O, :self.K].copy_(wd)
            self.bp[:self.O].copy_(b.detach())
        self.version = version


class Drop32:
    def __init__(self, tag):
        self.tag = tag

    def params(self):
        return []

    def buffers(self, zb, w):
        return dict(y=zb(w), dy=zb(w)), w

    def fwd(self, x, b, p, seed):
        return ops.dropout_f32(x, b["y"], p, seed, self.tag) if p > 0 else x

    def bwd(self, d, b, p, seed):
        return (ops.dropout_f32(d, b["dy"], p, seed, self.tag) if p > 0 else d), []


class Linear32:
    """act None | "relu" (undone by the "keep where aux > 0" epilogue of the NEXT Linear's data-gradient GEMM, against this one's
    output) | "gelu" (GELU' kept by the epilogue, multiplied in by mul_f32)."""

    def __init__(self, w32, act=None):
        self.w32, self.act = w32, act

    def params(self):
        return [self.w32.weight, self.w32.bias]

    def buffers(self, zb, w):
        N = self.w32.Op
        b = dict(out=zb(N), dx=zb(w))
        if self.act == "gelu":
            b.update(pre=zb(N), dpre=zb(N))
        return b, N

    def fwd(self, x, b, p, seed):
        w, n = self.w32, x.shape[0]
        assert x.shape[1] == w.Kp and b["out"].shape[1] == w.Op
        ops.gemm_nt_f32(x, x.stride(0), w.W, w.Kp, b["out"], b["out"].stride(0), n, w.Op, w.Kp, bias=w.b, epi={None: 0, "relu": 2, "gelu": 1}[self.act],
                        pre=b.get("pre"), ldpre=w.Op)
        return b["out"]

    def bwd(self, d, b, p, seed):
        w, n = self.w32, d.shape[0]
        if w.K % 4:
            raise NotImplementedError("fp32 head: a Linear input width that is not a multiple of 4")
        if self.act == "gelu":
            d = ops.mul_f32(d, b["pre"], b["dpre"])
        gw, gb = (torch.zeros_like(q, dtype=F32) for q in self.params())
        # gw [O, K] += d^T . x as the NT product of the two transposed operands (rows zero-padded to 32), gb = column sums of d
        np_ = round_up(n, 32)
        tG, tA = b["tG"][:w.O * np_].view(w.O, np_), b["tA"][:w.K * np_].view(w.K, np_)
        ops.transpose_f32(d, w.Op, tG, np_, n, w.O, np_, colsum=gb)
        ops.transpose_f32(b["x"], w.Kp, tA, np_, n, w.K, np_)
        ops.gemm_nt_f32(tG, np_, tA, np_, gw, w.K, w.O, w.K, np_, atomic=True)
        if b["relu"] is not None:
            ops.gemm_nt_f32(d, w.Op, w.Wt, w.Op, b["dx"], w.Kp, n, w.Kp, w.Op, epi=5, aux=b["relu"], ldaux=w.Kp)
        else:
            ops.gemm_nt_f32(d, w.Op, w.Wt, w.Op, b["dx"], w.Kp, n, w.Kp, w.Op)
        return b["dx"], [gw, gb]


class LayerNorm32:
    def __init__(self, ln):
        self.ln = ln

    def params(self):
        return [self.ln.weight, self.ln.bias]

    def buffers(self, zb, w):
        return dict(out=zb(w), dx=zb(w), stats=zb(2)), w

    def fwd(self, x, b, p, seed):
        H = self.ln.weight.shape[0]
        ops.layernorm_f32_fwd(x[:, :H], self.ln.weight.detach(), self.ln.bias.detach(), b["out"][:, :H], b["stats"])
        return b["out"]

    def bwd(self, d, b, p, seed):
        H = self.ln.weight.shape[0]
        gg, gbeta = (torch.zeros_like(q, dtype=F32) for q in self.params())
        ops.layernorm_f32_bwd(d[:, :H], b["x"][:, :H], b["stats"], self.ln.weight.detach(), dx=b["dx"][:, :H], dgamma=gg, dbeta=gbeta)
        return b["dx"], [gg, gbeta]


class Head32(Head):
    """Head over the fp32 stages: scratch, logits and d(x) stay fp32.  loss_fn sees fp32 logits [rows, outputs padded to 32]."""

    def _state(self, n, dev):
        cap = round_up(n, self.row_cap)
        if cap not in self._states:
            zb = lambda w: torch.zeros((cap, w), dtype=F32, device=dev)
            lins = [s.w32 for s in self.stages if isinstance(s, Linear32)]
            w = lins[0].Kp                                                                   # the input width
            st = dict(x=zb(w), loss=torch.zeros((1,), dtype=F32, device=dev), per=[])
            # transposed operands of the weight gradients, shared by the Linears (the largest of them)
            rp = round_up(cap, 32)
            tG = torch.zeros((max(l.O for l in lins) * rp,), dtype=F32, device=dev)
            tA = torch.zeros((max(l.K for l in lins) * rp,), dtype=F32, device=dev)
            for s in self.stages:
                b, w = s.buffers(zb, w)
                if isinstance(s, Linear32):
                    b.update(tG=tG, tA=tA)
                st["per"].append(b)
            st.update(logits=st["per"][-1]["out"], copy=zb(w))
            self._states[cap] = st
        cut = lambda d: {k: (v[:n] if isinstance(v, torch.Tensor) and v.dim() == 2 else v) for k, v in d.items()}
        st = cut(self._states[cap])
        st["per"] = [cut(b) for b in st["per"]]
        return st

    def forward(self, x, p, loss_fn=None):
        """x [rows, K] fp32 -> the pass: "logits" (fp32; after a loss they hold its gradient and "copy" the logits), "loss" [1]."""
        st = self._state(x.shape[0], x.device)
        for s in self.stages:
            if isinstance(s, Linear32):
                s.w32.sync()
        st["x"][:, :x.shape[1]].copy_(x.detach())                # into the head's own (width-padded) input buffer
        cur, relu = st["x"], None
        for s, b in zip(self.stages, st["per"]):
            b["x"], b["relu"] = cur, relu
            cur = s.fwd(cur, b, p, self.seed)
            if isinstance(s, Linear32):
                relu = cur if s.act == "relu" else None
        st["loss"].zero_()
        if loss_fn is not None:
            loss_fn(st["logits"], st["copy"], st["loss"], 1.0, True)
        st.update(p=p, loss_fn=loss_fn, K=x.shape[1])
        return st

    def backward(self, st, g=1.0):
        p, loss_fn = st["p"], st["loss_fn"]
        if loss_fn is None:
            return torch.zeros((st["x"].shape[0], st["K"]), dtype=F32, device=st["x"].device), \
                [torch.zeros_like(q, dtype=F32) for q in self.params()]
        if g != 1.0:      # upstream scale: re-derive d(logits) from the kept logits
            st["logits"].copy_(st["copy"])
            st["loss"].zero_()
            loss_fn(st["logits"], st["copy"], st["loss"], g, False)
        d, grads = st["logits"], []
        for s, b in zip(reversed(self.stages), reversed(st["per"])):
            d, gs = s.bwd(d, b, p, self.seed)
            grads = gs + grads
        if p > 0:
            ops.rng_advance(self.seed)
        return d[:, :st["K"]].clone(), grads


class HeadFn(torch.autograd.Function):
    """x [rows, K] fp32 -> (the 16-bit logits [rows, padded outputs] as the pass keeps them, loss): one autograd node per head."""

    @staticmethod
    def forward(ctx, x, head, p, loss_fn, *params):
        ctx.head, ctx.st = head, head.forward(x, p, loss_fn)
        logits = ctx.st["copy" if loss_fn is not None else "logits"]
        ctx.mark_non_differentiable(logits)
        return logits, ctx.st["loss"][0].clone()

    @staticmethod
    def backward(ctx, _g_logits, g_loss):
        dx, grads = ctx.head.backward(ctx.st, float(g_loss))
        return (dx, None, None, None) + tuple(grads)


def run_head(head, x, p, loss_fn=None):
    return HeadFn.apply(x, head, p, loss_fn, *head.params())
