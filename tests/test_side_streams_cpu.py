"""side_streams.SideStreams write tracking, on the CPU: streams and events are stand-ins that log what was recorded and waited for
(the module only calls torch.cuda.Event / stream / current_stream and Stream.wait_event), so the bookkeeping -- which events a
tensor's writers own, what join forgets -- is checked without a device."""
import contextlib
import importlib

import pytest
import torch


class _Event:
    def __init__(self, log):
        self.log, self.on = log, None

    def record(self, stream=None):
        self.on = stream if stream is not None else _State.current


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_event(self, ev):
        self.log.append((self.name, ev))


class _State:
    current = None


@pytest.fixture
def hz(monkeypatch):
    log = []
    main = _Stream("main", log)
    _State.current = main

    @contextlib.contextmanager
    def use(stream):
        prev, _State.current = _State.current, stream
        try:
            yield
        finally:
            _State.current = prev

    monkeypatch.setattr(torch.cuda, "Event", lambda: _Event(log))
    monkeypatch.setattr(torch.cuda, "stream", use)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: _State.current)
    h = importlib.import_module("vl-bert_amd.side_streams").SideStreams()
    h.log, h.main, h.side = log, main, _Stream("side", log)
    return h


def test_writers_are_exactly_the_launches_that_wrote_the_tensor(hz):
    a, b, c, x = (torch.zeros(4) for _ in range(4))
    ran = []
    hz.run(hz.side, lambda: ran.append(1), reads=[x], writes=[a, None])
    hz.run(hz.side, lambda: ran.append(2), reads=[x], writes=[b])
    hz.run(hz.side, lambda: ran.append(3), reads=[x], writes=[a, b])
    hz.run(hz.side, lambda: ran.append(4), reads=[x])
    assert ran == [1, 2, 3, 4]
    wa, wb = hz.writers(a), hz.writers(b)
    assert len(wa) == 2 and len(wb) == 2 and hz.writers(c) == [] and hz.writers(None) == []
    assert wa[1] is wb[1] and wa[0] is not wb[0]                     # launch 3 wrote both; launches 1 and 2 one each
    assert all(ev.on is hz.side for ev in wa + wb)                   # recorded behind the launch, on its stream
    both = hz.writers(a, b, None)
    assert len(both) == 3 and both[0] is wa[0] and both[1] is wa[1] and both[2] is wb[0]      # each launch once
    # the reader bookkeeping is untouched by the writes: the newest reader of x on the side stream is launch 4's event
    assert list(hz._pending) == [x.data_ptr()] and all(hz._pending[x.data_ptr()][hz.side] is not ev for ev in both)


def test_before_accumulate_waits_on_the_main_stream_for_those_launches_only(hz):
    a, b, x = (torch.zeros(4) for _ in range(3))
    hz.run(hz.side, lambda: None, reads=[x], writes=[a])
    hz.run(hz.side, lambda: None, reads=[x], writes=[b])
    n = len(hz.log)
    hz.before_accumulate(a, None)
    assert hz.log[n:] == [("main", hz.writers(a)[0])]
    n = len(hz.log)
    hz.before_accumulate(torch.zeros(4))
    assert hz.log[n:] == []


def test_join_forgets_writers_and_an_inline_launch_records_none(hz):
    a, x = torch.zeros(4), torch.zeros(4)
    hz.run(hz.side, lambda: None, reads=[x], writes=[a])
    assert len(hz.writers(a)) == 1
    n = len(hz.log)
    hz.join([hz.side])
    assert [s for s, _ in hz.log[n:]] == ["main"] and hz.log[n][1].on is hz.side      # one event behind the side stream
    assert hz.writers(a) == [] and hz._written == {} and hz._pending == {}
    calls = []
    hz.run(None, lambda: calls.append(1), reads=[x], writes=[a])
    assert calls == [1] and hz.writers(a) == [] and hz._written == {}
