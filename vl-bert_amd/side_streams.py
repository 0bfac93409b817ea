"""Hazard bookkeeping for work pushed onto a second stream (the weight gradients of engine.py and vision.py: they only feed the
optimizer, while the data-gradient chain on the main stream is the critical path).

Two hazards per launch: it reads buffers the main stream produced (it starts behind an event recorded after the producers), and the
main stream must not overwrite those buffers before it is done (an event recorded behind it, waited for by the next writer).  Events
only, no host synchronisation: everything here is capturable in a hipGraph.  The streams belong to the callers, which choose one per
call (None = no side stream: run inline)."""
import torch


class SideStreams:
    def __init__(self):
        self._pending = {}       # data_ptr -> {stream: newest event behind a reader on that stream} (it implies the older ones)

    def run(self, stream, fn, reads=()):
        """fn() on `stream`, behind everything enqueued on the current stream so far; `reads` are the transient buffers it reads."""
        if stream is None:
            fn()
            return
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(stream):
            stream.wait_event(ready)
            fn()
            done = torch.cuda.Event()
            done.record()
        for t in reads:          # whoever overwrites `t` next must wait for this
            self._pending.setdefault(t.data_ptr(), {})[stream] = done

    def before_write(self, *bufs):
        """The current stream is about to overwrite these buffers (None entries skipped): wait for the launches still reading them."""
        for t in bufs:
            evs = self._pending.pop(t.data_ptr(), None) if t is not None else None
            for ev in (evs or {}).values():
                torch.cuda.current_stream().wait_event(ev)

    def join(self, streams):
        """Everything issued on `streams` so far completes before later work of the current stream."""
        for s in streams:
            ev = torch.cuda.Event()
            ev.record(s)
            torch.cuda.current_stream().wait_event(ev)
        self._pending.clear()
