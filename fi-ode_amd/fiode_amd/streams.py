"""The HIP streams of the training step's side branches: where they are made, named and joined.

torch.cuda.Stream() hands out streams from a fixed pool (32 per priority, round robin), so a stream
made "fresh" for one role can be the very stream another role already holds: the placement trials
of GraphTrainStep (4 captures, ~9 new side streams each) wrap the pool and alias, e.g., a map-prefetch
stream with the head's weight-gradient stream.  Inside a hipGraph capture that aliasing can make a
stream that joined the capture wait on an event it recorded itself, and this ROCm runtime then
crashes the host in hipStreamEndCapture (a recursive walk of the captured nodes; SIGSEGV under
torch.cuda.graph's capture_end -- tools/probes/capture_selfwait_probe.py reproduces it with four
lines of torch, DESIGN.md "capture_end SIGSEGV").  Every side stream of the product is therefore a
stream of its own, made with hipStreamCreateWithPriority in torch's own HIP runtime and wrapped as
torch.cuda.ExternalStream; they live for the process (a handful per captured step).

* ``new_stream`` makes one; ``shared(device, name)`` is one per name for the whole process (the
  head's weight-gradient streams, certify_lipschitz's side stream).
* ``StepStreams`` owns the streams of one capture of the step (or of eager training), by role.
* ``fork`` / ``join`` (stream waits) and ``prefetch`` / ``take`` (an event) are the only way the
  product sends work to a side stream.  A side stream that IS the current stream runs the work
  inline with no wait, so no stream waits on an event it recorded itself through them.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading

import torch

_HIP = None
_LOCK = threading.Lock()
# (device index, handle, priority) of every stream made here, in creation order (never destroyed);
# which hardware queue a stream gets is fixed when it is made, so this trace is the step's placement
_MADE: list = []
_SHARED: dict = {}               # (device index, name) -> stream


def _hip():
    global _HIP
    if _HIP is None:
        # the runtime instance torch itself uses (a stream of another libamdhip64 would be foreign to it)
        _HIP = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        _HIP.hipStreamCreateWithPriority.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint, ctypes.c_int]
        _HIP.hipStreamCreateWithPriority.restype = ctypes.c_int
    return _HIP


def _index(device) -> int:
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    if dev.type != "cuda":
        raise ValueError(f"new_stream: a ROCm device, got {dev}")
    return dev.index if dev.index is not None else torch.cuda.current_device()


def new_stream(device, priority: int = 0) -> torch.cuda.Stream:
    """A stream no other role shares (non-blocking, like torch's pool streams; priority as torch's:
    0 normal, -1 high)."""
    idx = _index(device)
    h = ctypes.c_void_p()
    with _LOCK, torch.cuda.device(idx):
        rc = _hip().hipStreamCreateWithPriority(ctypes.byref(h), 1, int(priority))   # 1 = hipStreamNonBlocking
        if rc != 0 or not h.value:
            raise RuntimeError(f"hipStreamCreateWithPriority failed ({rc})")
        _MADE.append((idx, h.value, int(priority)))
    return torch.cuda.ExternalStream(h.value, device=torch.device("cuda", idx))


def shared(device, name: str) -> torch.cuda.Stream:
    """The process-lifetime stream called ``name`` on ``device``, made at its first use."""
    key = (_index(device), name)
    if key not in _SHARED:
        _SHARED[key] = new_stream(device)
    return _SHARED[key]


def distinct(streams) -> bool:
    """True when no two of ``streams`` (None entries ignored) are the same HIP stream."""
    ids = [s.cuda_stream for s in streams if s is not None]
    return len(ids) == len(set(ids))


class StepStreams:
    """The streams of one capture of the training step (or of eager training), by role: ``capture``
    (the stream the step is captured on), ``comm`` (the captured all-reduces), ``maps`` (the four
    map-prefetch streams), ``ode`` (the train_ode solve), ``wtap`` (the dynamics' weight gradients)
    and one per conv layer whose map is computed ahead (``conv``).  Each is made at its first use.
    ``step`` is the stream compute_loss was entered on, set only while it runs (``scope``)."""

    def __init__(self):
        self.capture = self.comm = self.ode = self.wtap = self.maps = self.step = None
        self.conv: dict = {}

    def get(self, role: str, device, priority: int = 0) -> torch.cuda.Stream:
        """The stream of ``role`` ('capture', 'comm', 'ode' or 'wtap')."""
        if getattr(self, role) is None:
            setattr(self, role, new_stream(device, priority))
        return getattr(self, role)

    def map_streams(self, device) -> list:
        if self.maps is None:
            self.maps = [new_stream(device) for _ in range(4)]
        return self.maps

    def conv_stream(self, layer) -> torch.cuda.Stream:
        if layer not in self.conv:
            self.conv[layer] = new_stream(layer.weight.device)
        return self.conv[layer]

    def all(self) -> list:
        """Every stream a step run under this owner can fork work to (the shared ones included)."""
        return ([s for s in (self.capture, self.comm, self.ode, self.wtap) if s is not None] + list(self.maps or [])
                + list(self.conv.values()) + list(_SHARED.values()))

    @contextlib.contextmanager
    def scope(self, step_stream):
        """This owner is ``current()`` and ``step`` = ``step_stream`` inside; both restored on exit,
        so a later eager or non-parallel step never sends work to a stale (e.g. capture) stream."""
        global _CURRENT
        prev, prev_step = _CURRENT, self.step
        _CURRENT, self.step = self, step_stream
        try:
            yield self
        finally:
            _CURRENT, self.step = prev, prev_step


_CURRENT = StepStreams()         # outside any scope: the process's own


def current() -> StepStreams:
    return _CURRENT


# ---- fork / join --------------------------------------------------------------------------------
# (the three touch points with torch.cuda, so the helpers' call order can be tested without a device)
def _current_stream(device=None):
    return torch.cuda.current_stream(device)


def _on(stream):
    return torch.cuda.stream(stream)


def _event():
    return torch.cuda.Event()


def _tensors(x):
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            yield from _tensors(v)
    elif isinstance(x, (tuple, list)):
        for v in x:
            yield from _tensors(v)


def _is_current(side) -> bool:
    """No side stream, or it is the current one: the work runs inline and nothing waits."""
    return side is None or side == _current_stream(side.device)


def fork(side, fn=None, reads=()):
    """Run fn() on ``side`` after everything on the current stream so far; returns a branch for
    ``join``.  ``reads``: tensors fn reads that the current stream allocated (the caching allocator
    keeps them until ``side`` is done with them).  fn None: only order ``side`` after the current
    stream.  ``side`` None or the current stream: fn() runs inline, nothing waits."""
    if _is_current(side):
        return (fn() if fn is not None else None), None
    side.wait_stream(_current_stream(side.device))
    out = None
    if fn is not None:
        with _on(side):
            out = fn()
    for t in reads:
        t.record_stream(side)
    return out, side


def join(*branches):
    """The current stream waits for the branches' streams (each once, in fork order) and takes
    over their results; returns the results, one per branch."""
    waited = []
    for out, side in branches:
        if _is_current(side):
            continue
        cur = _current_stream(side.device)
        if side not in waited:
            cur.wait_stream(side)
            waited.append(side)
        for t in _tensors(out):
            t.record_stream(cur)
    return tuple(out for out, _ in branches)


def run_on(side, fn):
    """fork + join at once: fn() on ``side``, ordered after and before the current stream."""
    return join(fork(side, fn))[0]


def prefetch(stream, fn):
    """Run fn() on ``stream`` (forked from the current stream); returns (result, done event) for
    ``take``.  ``stream`` the current stream: inline, and no event."""
    if _is_current(stream):
        return fn(), None
    stream.wait_stream(_current_stream(stream.device))
    with _on(stream):
        out = fn()
        ev = _event()
        ev.record(stream)
    return out, ev


def take(pre):
    """Join a prefetched result into the current stream."""
    out, ev = pre
    if ev is not None:
        main = _current_stream()
        main.wait_event(ev)
        for t in _tensors(out):
            t.record_stream(main)
    return out
