"""A caller's non-blocking stream, held back by a delay, for the tests of tests/test_caller_stream.py.

held_stream() yields a Held around a fresh torch.cuda.Stream() -- torch creates these non-blocking: they do not synchronise
with the null stream -- made current, whose first piece of work is a spin kernel (torch.cuda._sleep) of DELAY_MS.  The test
then queues the copies of its inputs into their device tensors on that stream (Held.copy), behind the delay, and calls the
library with the stream current.  Until the copies run the tensors hold a decoy, so whatever the library issues on another
stream (the null stream, the handle's private stream, the stream of an earlier build) runs at once, reads the decoy or an
intermediate that is not written yet, and the result cannot equal the reference.

The decoy of a build or a consumer is rolled(x): the wanted rows moved up by one, x[(i + 1) % n].  The same multiset of
points: every per-cell count, row total and pair count is the wanted build's, so a mis-ordered stage gives a wrong list or
wrong forces and never a size that a later stage was not sized for.  The decoy of an update chain is what the tensor holds
anyway: the previous step's positions.

The runtime multiplexes streams onto a few hardware queues, and streams that share one run in order.  held_stream() therefore
probes each stream it makes: a fill on the null stream must complete while the stream spins; a stream behind whose delay the
null stream waits is left to drain and the next one of torch's pool is taken (about one in four is).

Non-vacuity is asserted: Held.copy records an event behind each copy, and Held.assert_held() -- called immediately before the
first library call of a sequence, and behind the last call of a sequence that only enqueues (on a handle warmed so that
nothing allocates) -- demands that the event has not happened.  The second assertion is the header's "only enqueues".

The delay.  torch.cuda._sleep counts ticks of the device's clock, whose rate differs between devices, so the ticks per
millisecond are measured once per session with two events (ticks_per_ms; 2.41 million on the MI355X).  DELAY_MS = 100 ms, of
at most DELAY_CAP_MS = 500 ms.  Measured on an MI355X, host time from the start of the delay, the probe
of the null stream included, to the return of the last call of a warmed sequence, over the 398 sequences of
tests/test_caller_stream.py in four runs: 0.14 to 0.17 ms in the median, 0.67 ms at most (two handles interleaved; five
updates, each behind a copy: 0.25 to 0.54 ms), and 6.1 ms for the first sequence of a fresh process.  100 ms is 16 times the
longest of these; the requirement is 4 times.  Python's garbage collector is off while a stream is held (held_stream).
"""
import contextlib
import gc
import time

import numpy as np

DELAY_MS = 100.0
DELAY_CAP_MS = 500.0
_ticks_per_ms = None
HOST_MS = []  # (label, host milliseconds between the start of the delay and the last enqueue) of this session


def _torch():
    import torch

    return torch


def rolled(x):
    """The decoy of x: x[(i + 1) % n] in row i."""
    out = np.roll(np.asarray(x), -1, axis=0)
    out.setflags(write=False)
    return out


def unrolled_ids(n):
    """new_id[j] = the row of the decoy that holds the wanted row j."""
    return (np.arange(n, dtype=np.int64) - 1) % n


def ticks_per_ms():
    """torch.cuda._sleep ticks per millisecond on the current device, measured once: the spin is lengthened until it lasts
    at least 5 ms, so that the launch overhead does not count."""
    global _ticks_per_ms
    if _ticks_per_ms is None:
        torch = _torch()
        torch.cuda._sleep(1000)
        warm = torch.empty(8, device="cuda")  # (torch's fill and copy kernels load here, not inside the first held sequence)
        warm.fill_(0.0)
        warm.clone().copy_(warm, non_blocking=True)
        torch.cuda.synchronize()
        ticks = 100_000
        for _ in range(16):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(ticks)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0:
                break
            ticks *= 4
        assert ms >= 5.0, (ticks, ms)
        _ticks_per_ms = ticks / ms
        print(f"held: {_ticks_per_ms:.0f} _sleep ticks per ms")
    return _ticks_per_ms


class Held:
    def __init__(self, stream, delay_ms, began):
        self.stream, self.delay_ms, self.t0 = stream, delay_ms, began  # (began: the host's clock when the delay was queued)
        self.event = None
        self._keep = []

    def copy(self, dst, src):
        """dst.copy_(src) on the held stream, behind the delay; both are device tensors (a copy from pageable host memory
        would make the host wait for the delay).  src is kept alive until the stream has drained."""
        torch = _torch()
        assert dst.is_cuda and src.is_cuda and torch.cuda.current_stream() == self.stream
        dst.copy_(src, non_blocking=True)
        self._keep.append((dst, src))
        self.event = torch.cuda.Event()
        self.event.record(self.stream)

    def assert_held(self, label=None):
        """The last input copy has not run yet.  With a label: the end of a sequence that only enqueues; the host time it
        took is kept in HOST_MS and printed."""
        assert self.event is not None, "no input was queued behind the delay"
        done = self.event.query()
        ms = (time.perf_counter() - self.t0) * 1e3
        if label is not None:
            HOST_MS.append((label, ms))
            print(f"held {label}: host {ms:.2f} ms of {self.delay_ms:.0f} ms")
        assert not done, (f"the inputs were copied before the library was called ({ms:.1f} ms after the delay of "
                          f"{self.delay_ms:.0f} ms began)" if label is None else
                          f"{label}: the stream drained while the host enqueued ({ms:.1f} ms of {self.delay_ms:.0f} ms): some call waited")

    def drain(self):
        self.stream.synchronize()
        self._keep.clear()


@contextlib.contextmanager
def held_stream(delay_ms=None, settle=True):
    """A new non-blocking stream, current within the block, that begins with a delay of delay_ms (DELAY_MS).  settle:
    everything queued before (on any stream) is waited for first -- False for a second held stream opened while the first is
    still held.  The stream is drained when the block ends.  A stream whose delay the null stream would have to wait behind
    is not taken (see below): every held stream has the teeth that test_harness_sees_an_off_stream_read shows for one."""
    torch = _torch()
    delay_ms = DELAY_MS if delay_ms is None else float(delay_ms)
    assert 0 < delay_ms <= DELAY_CAP_MS
    ticks = int(delay_ms * ticks_per_ms())
    if settle:
        torch.cuda.synchronize()
    default = torch.cuda.default_stream()
    probe = torch.empty(1, device="cuda")
    # no garbage collection while a stream is held: a handle that the collector finds then is destroyed then, and freeing
    # its device memory waits for the device -- the host would stand still for the rest of the delay in the middle of a
    # sequence that is asserted to only enqueue
    collecting = gc.isenabled()
    gc.disable()
    for _ in range(8):
        s = torch.cuda.Stream()
        began = time.perf_counter()
        with torch.cuda.stream(s):
            torch.cuda._sleep(ticks)
        # the runtime multiplexes streams onto a few hardware queues: a stream behind whose delay the null stream has to
        # wait would hide what this harness is there to show, so it is left to drain and the next one is taken
        t0 = time.perf_counter()
        with torch.cuda.stream(default):
            probe.fill_(0.0)
            default.synchronize()
        if (time.perf_counter() - t0) * 1e3 < 0.25 * delay_ms:
            break
        print("held: the null stream waits behind this stream's delay; taking the next stream")
        s.synchronize()
    else:
        if collecting:
            gc.enable()
        raise AssertionError("no side stream lets the null stream run while it is held")
    with torch.cuda.stream(s):
        h = Held(s, delay_ms, began)
        try:
            yield h
        finally:
            h.drain()
            if collecting:
                gc.enable()


def device(a, dtype=None):
    """A host array as a device tensor, staged on the default stream and complete on return."""
    torch = _torch()
    a = np.ascontiguousarray(np.asarray(a) if dtype is None else np.asarray(a).astype(dtype))
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t
