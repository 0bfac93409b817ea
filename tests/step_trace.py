"""The library calls of an engine step, recorded on the CPU with the library stubbed: what a refactor of the host side must leave
as it is.  No build and no GPU: `_lib.load` hands out an object whose every attribute records its call and returns 0, and the three
`ops` helpers that refuse CPU tensors (`_p`, `_pf`, `_stream`) hand out plain addresses.

    with recording() as calls:
        eng = E.PretrainEngine(E.ModelConfig(num_hidden_layers=2), 2, 8, 4, device="cpu")
        train_step(eng)
    normalised(calls)      # [(entry point, (arguments...))], every pointer replaced by the index of its first appearance

Pointers are numbered in the order the calls first show them, so two traces are equal exactly when the same entry points run in the
same order on buffers that alias each other in the same way, with the same scalar arguments.  The (source, destination) pairs of an
`ops.TransposeBatch` live in a device table the launch only points to: they are recorded when the table is built, as a call of their
own named "TransposeBatch(pairs)".
"""
import contextlib
import ctypes
import importlib

ENGINE = importlib.import_module("vl-bert_amd.engine")
OPS = importlib.import_module("vl-bert_amd.ops")
LIB = importlib.import_module("vl-bert_amd._lib")


class Ptr(int):
    """An address (ctypes takes it as the integer it is)."""


class _Recorder:
    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        def entry(*args):
            self._calls.append((name, args))
            return 0
        return entry


def _p(t, dtype=None):
    return None if t is None else Ptr(t.data_ptr())


def _pf(t, off=0):
    if t is None:
        return None
    if isinstance(t, tuple):
        t, off = t
    return Ptr(t.data_ptr() + 4 * off)


@contextlib.contextmanager
def recording():
    calls = []
    saved = (LIB.load, OPS._p, OPS._pf, OPS._stream, OPS.TransposeBatch.__init__)
    tb_init = OPS.TransposeBatch.__init__

    def tb_recorded(self, pairs, device):
        pairs = list(pairs)
        calls.append(("TransposeBatch(pairs)", tuple(x for s, d in pairs for x in (Ptr(s.data_ptr()), Ptr(d.data_ptr()), tuple(s.shape)))))
        tb_init(self, pairs, device)
    rec = _Recorder(calls)
    LIB.load, OPS._p, OPS._pf, OPS._stream, OPS.TransposeBatch.__init__ = (lambda: rec), _p, _pf, (lambda: 0), tb_recorded
    try:
        yield calls
    finally:
        LIB.load, OPS._p, OPS._pf, OPS._stream, OPS.TransposeBatch.__init__ = saved


def normalised(calls):
    """[(name, args)] with pointers as ("p", first-seen index); ctypes arrays become tuples.  An integer too large for any size,
    count or tag of these shapes is an address (the descriptor tables pass theirs as `data_ptr()`)."""
    seen = {}

    def ptr(v):
        return ("p", seen.setdefault(int(v), len(seen)))

    def norm(a):
        if isinstance(a, Ptr):
            return ptr(a)
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return tuple(None if v is None else ptr(v) for v in a)
            if a._type_ is ctypes.c_char:
                return ("bytes", len(a))
            return tuple(a)
        if isinstance(a, tuple):
            return tuple(norm(v) for v in a)
        if isinstance(a, int) and not isinstance(a, bool) and a >= 1 << 36:
            return ptr(a)
        return a
    return [(name, tuple(norm(a) for a in args)) for name, args in calls]


def names(calls):
    return [name for name, _ in calls if not name.endswith("(pairs)")]


def train_step(eng):
    eng.zero_grad()
    eng.forward(True)
    eng.backward(True)
    eng.optimizer_step()


def core_step(eng, hidden=False):
    """The module-API engine: forward, then the backward entry point of its mode on zero gradients."""
    eng.zero_grad()
    eng.forward_core(True)
    if eng.seq_out:
        eng.backward_core_sequence(None, train=True)
    elif hidden or not eng.with_heads:
        eng.backward_core_hidden(None, None, train=True)
    else:
        eng.backward_core(None, None, train=True)
    eng.optimizer_step()


def run(cfg_kw=None, B=2, T=8, R=4, step=train_step, **kw):
    """Trace of construction + one step of PretrainEngine(ModelConfig(num_hidden_layers=2, **cfg_kw), B, T, R, device='cpu', **kw)
    -> (engine, raw calls of the step; of the construction, which only asks the library for workspace sizes, the "(pairs)" entries)."""
    with recording() as calls:
        eng = ENGINE.PretrainEngine(ENGINE.ModelConfig(num_hidden_layers=2, **(cfg_kw or {})), B, T, R, device="cpu", **kw)
        calls[:] = [c for c in calls if c[0].endswith("(pairs)")]
        step(eng)
    return eng, calls
