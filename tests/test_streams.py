"""The fork / join and prefetch / take helpers of fiode_amd.streams issue exactly the stream calls
the hand-written sites issued, in the same order, and never make a stream wait on itself.  Fake
streams that log their calls stand in for HIP streams: no device is needed."""
import contextlib

import pytest
import torch

from fiode_amd import streams


class FakeStream:
    device = None

    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append((self.name, "wait_stream", other.name))

    def wait_event(self, ev):
        self.log.append((self.name, "wait_event", ev.name))


class FakeEvent:
    name = "ev"

    def __init__(self, log):
        self.log = log

    def record(self, stream):
        self.log.append((self.name, "record", stream.name))


class LoggedTensor(torch.Tensor):
    def record_stream(self, stream):
        self.log.append((self.tag, "record_stream", stream.name))


@pytest.fixture
def fake(monkeypatch):
    """log, the streams 'cur' and 'side', and a tensor factory; streams' three touch points with
    torch.cuda replaced by fakes ('cur' is the current stream outside a stream context)."""
    log = []
    cur, side = FakeStream("cur", log), FakeStream("side", log)
    stack = [cur]

    @contextlib.contextmanager
    def on(stream):
        log.append(("enter", stream.name))
        stack.append(stream)
        try:
            yield
        finally:
            stack.pop()
            log.append(("exit", stream.name))

    def tensor(name):
        t = torch.Tensor._make_subclass(LoggedTensor, torch.zeros(1))
        t.tag, t.log = name, log
        return t

    monkeypatch.setattr(streams, "_current_stream", lambda device=None: stack[-1])
    monkeypatch.setattr(streams, "_on", on)
    monkeypatch.setattr(streams, "_event", lambda: FakeEvent(log))
    return log, cur, side, tensor


def test_fork_then_join_call_sequence(fake):
    """One layer of the linear head's backward: the side stream waits for the current one, the
    weight / bias gradient run on it, its inputs are kept for it; later the current stream waits for
    the side stream and takes the results over."""
    log, cur, side, tensor = fake
    g, x, dW, db = (tensor(n) for n in ("g", "x", "dW", "db"))

    def wgrad():
        log.append(("fn",))
        return dW, db

    branch = streams.fork(side, wgrad, reads=(g, x))
    log.append(("input-gradient chain",))
    (out,) = streams.join(branch)
    assert out[0] is dW and out[1] is db
    assert log == [("side", "wait_stream", "cur"), ("enter", "side"), ("fn",), ("exit", "side"),
                   ("g", "record_stream", "side"), ("x", "record_stream", "side"),
                   ("input-gradient chain",),
                   ("cur", "wait_stream", "side"), ("dW", "record_stream", "cur"), ("db", "record_stream", "cur")]


def test_join_waits_once_per_stream_in_fork_order(fake):
    log, cur, side, tensor = fake
    other = FakeStream("other", log)
    a = streams.fork(side, lambda: tensor("a"))
    b = streams.fork(other, lambda: tensor("b"))
    c = streams.fork(side, lambda: tensor("c"))
    del log[:]
    outs = streams.join(a, b, c)
    assert [t.tag for t in outs] == ["a", "b", "c"]
    assert [e for e in log if e[1] == "wait_stream"] == [("cur", "wait_stream", "side"), ("cur", "wait_stream", "other")]


def test_fork_without_fn_only_orders_the_side_stream(fake):
    log, cur, side, _ = fake
    assert streams.fork(side) == (None, side)
    assert log == [("side", "wait_stream", "cur")]


@pytest.mark.parametrize("which", ["current", "none"])
def test_side_stream_that_is_current_runs_inline_with_no_wait(fake, which):
    log, cur, side, tensor = fake
    target = cur if which == "current" else None
    t = tensor("t")

    def fn():
        log.append(("fn",))
        return t

    branch = streams.fork(target, fn, reads=(tensor("r"),))
    (out,) = streams.join(branch)
    assert out is t and streams.run_on(target, fn) is t
    assert streams.join((None, target)) == (None,)
    assert log == [("fn",), ("fn",)]                    # no wait, no stream switch, no record_stream
    if target is not None:
        pre = streams.prefetch(target, fn)
        assert pre == (t, None) and streams.take(pre) is t
        assert log == [("fn",)] * 3


def test_run_on_is_fork_and_join(fake):
    log, cur, side, tensor = fake
    t = tensor("t")
    assert streams.run_on(side, lambda: t) is t
    assert log == [("side", "wait_stream", "cur"), ("enter", "side"), ("exit", "side"),
                   ("cur", "wait_stream", "side"), ("t", "record_stream", "cur")]


def test_prefetch_then_take_call_sequence(fake):
    """The event pair: the result's event is recorded on the side stream inside its context; take
    makes the current stream wait for the event, not for the stream, and walks dicts and tuples."""
    log, cur, side, tensor = fake
    out = {"Q": tensor("Q"), "b": (tensor("b0"), 3)}
    pre = streams.prefetch(side, lambda: out)
    assert pre[0] is out
    assert log == [("side", "wait_stream", "cur"), ("enter", "side"), ("ev", "record", "side"), ("exit", "side")]
    del log[:]
    assert streams.take(pre) is out
    assert log == [("cur", "wait_event", "ev"), ("Q", "record_stream", "cur"), ("b0", "record_stream", "cur")]


def test_step_streams_scope_restores_owner_and_step_stream():
    a, b = streams.StepStreams(), streams.StepStreams()
    outside = streams.current()
    with a.scope("s1"):
        assert streams.current() is a and a.step == "s1"
        with b.scope("s2"):
            assert streams.current() is b and b.step == "s2"
        assert streams.current() is a
    assert streams.current() is outside and a.step is None and b.step is None
    assert a.all() == list(streams._SHARED.values())     # nothing is made before its first use
