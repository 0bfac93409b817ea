"""Hazard bookkeeping for work pushed onto a second stream (the weight gradients of engine.py and vision.py: they only feed the
optimizer, while the data-gradient chain on the main stream is the critical path).

Two hazards per launch: it reads buffers the main stream produced (it starts behind an event recorded after the producers), and the
main stream must not overwrite those buffers before it is done (an event recorded behind it, waited for by the next writer).  A
launch can also name the tensors it WRITES (gradients it accumulates into): whoever adds into or reads one of them on another stream
waits for exactly the launches that wrote it (before_accumulate), not for the whole side stream.  Events
only, no host synchronisation: everything here is capturable in a hipGraph.  The streams belong to the callers, which choose one per
call (None = no side stream: run inline)."""
import torch


class SideStreams:
    def __init__(self):
        self._pending = {}       # data_ptr -> {stream: newest event behind a reader on that stream} (it implies the older ones)
        self._written = {}       # data_ptr -> [event behind each launch that wrote the tensor since the last join]

    def run(self, stream, fn, reads=(), writes=()):
        """fn() on `stream`, behind everything enqueued on the current stream so far; `reads` are the transient buffers it reads,
        `writes` the tensors it writes or accumulates into (None entries skipped)."""
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
        for t in writes:
            if t is not None:
                self._written.setdefault(t.data_ptr(), []).append(done)

    def writers(self, *bufs):
        """The events behind exactly the launches (since the last join) that named one of these tensors in `writes`, oldest first per
        tensor, each once (None entries skipped)."""
        evs = []
        for t in bufs:
            for ev in self._written.get(t.data_ptr(), ()) if t is not None else ():
                if not any(ev is e for e in evs):
                    evs.append(ev)
        return evs

    def before_accumulate(self, *bufs):
        """The current stream is about to add into (or read) these tensors: wait for the side launches that wrote them."""
        for ev in self.writers(*bufs):
            torch.cuda.current_stream().wait_event(ev)

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
        self._written.clear()
