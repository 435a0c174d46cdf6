"""A stream that is busy for a known time, so that a test sees WHEN a call's device work runs and not only what it computes.

stall(stream, ms) queues a finite busy-wait on `stream` (torch.cuda._sleep where the installed torch has it, else a chain of matmuls on
tensors allocated here once) and records an event behind it; still_running() is `not event.query()`.  Work the call under test queues on
`stream` runs behind the stall; work it queues anywhere else does not, and that difference is what the tests look at:

  (P) producer   the input is overwritten on `stream` behind the stall -- a call that reads it early codes the decoy that lay there
  (W) no early   a clone of the sentinel-filled output is queued on `stream` in front of the call -- a call that writes the output from
      write      another stream, ahead of the caller's queue, leaves pixels in the clone
  (C) consumer   a clone of the output is queued on `stream` right behind the call and only `stream` is waited for -- a call that has
                 not ordered `stream` behind its own streams leaves the sentinel in the clone

STALL_MS is a condition, not a measurement: it only has to outlast the host part of the call under test, and every test that relies on
it asserts still_running() at the point it relies on it, so a stall that is too short fails loudly and never passes vacuously.

Allocation rule.  Allocate every tensor of a test up front on the default stream, do ONE torch.cuda.synchronize(), then stall -- ready()
is that synchronise.  Keep references to every tensor until the test ends: the caching allocator hands a freed block to the next request
of the stream that allocated it, and a block recycled in the middle of a test would be written by two streams the test does not order.
snapshot() is the one allocation made later; its block comes from the pool of the stream that fills it, and that stream is waited for
before the clone is read.

Synchronisation rule.  After ready() a test waits only with stream.synchronize() or event.synchronize() and never calls
torch.cuda.synchronize(): the point is what the caller's stream alone guarantees."""
import numpy as np

STALL_MS = 200
SENTINEL = 0xA5

_cycles_per_ms = None
_matmul = None  # (a, b, iterations per millisecond)


def _timed(torch, stream, work):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        t0.record(stream)
        work()
        t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


def calibrate():
    """Once per process (a module fixture calls it): how many _sleep cycles, or matmuls, make a millisecond."""
    global _cycles_per_ms, _matmul
    import torch
    if _cycles_per_ms is not None or _matmul is not None:
        return
    s = torch.cuda.Stream()
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1000)  # load the kernel outside the measurement
        torch.cuda.synchronize()
        cycles = 20_000_000
        ms = _timed(torch, s, lambda: torch.cuda._sleep(cycles))
        assert ms > 0.5, "torch.cuda._sleep(%d) took %.3f ms: cannot calibrate a stall" % (cycles, ms)
        _cycles_per_ms = cycles / ms
    else:
        a = torch.rand((1024, 1024), device="cuda")
        b = torch.empty_like(a)
        torch.mm(a, a, out=b)
        torch.cuda.synchronize()
        ms = _timed(torch, s, lambda: [torch.mm(a, a, out=b) for _ in range(200)])
        _matmul = (a, b, 200 / ms)
    torch.cuda.synchronize()


class Stall:
    def __init__(self, event):
        self.event = event

    def still_running(self):
        return not self.event.query()


def stall(stream, ms=STALL_MS):
    """Keeps `stream` busy for about `ms` milliseconds; -> Stall (still_running())."""
    import torch
    calibrate()
    with torch.cuda.stream(stream):
        if _cycles_per_ms is not None:
            left = int(_cycles_per_ms * ms)
            while left > 0:  # (the kernel's argument is a 64-bit count, but stay far from any 2^31 in the clock arithmetic)
                torch.cuda._sleep(min(left, 1_000_000_000))
                left -= 1_000_000_000
        else:
            a, b, per_ms = _matmul
            for _ in range(max(1, int(per_ms * ms))):
                torch.mm(a, a, out=b)
        e = torch.cuda.Event()
        e.record(stream)
    return Stall(e)


def ready():
    """The one device-wide synchronise of a test: every allocation and upload made so far is done."""
    import torch
    torch.cuda.synchronize()


def sentinel_like(t):
    """`t` (a tensor, or a list of tensors) filled with 0xA5 bytes, in place; -> t"""
    import torch
    for x in (t if isinstance(t, (list, tuple)) else [t]):
        x.view(torch.uint8).fill_(SENTINEL) if x.is_contiguous() else x.fill_(_pattern(x.dtype))
    return t


def _pattern(dtype):
    import torch
    return {torch.uint8: 0xA5, torch.int16: -23131, torch.uint16: 0xA5A5}[dtype]


def snapshot(stream, t):
    """A clone of `t` (a tensor, or a list of tensors) made by a copy queued on `stream`."""
    import torch
    with torch.cuda.stream(stream):
        if isinstance(t, (list, tuple)):
            return [x.clone() for x in t]
        return t.clone()


def host(t):
    """numpy bytes-or-samples of a snapshot whose stream has been waited for (uint16 tensors come back as uint16)"""
    import torch
    if t.dtype == torch.uint16:
        return t.cpu().view(torch.int16).numpy().view(np.uint16)
    return t.cpu().numpy()


def all_sentinel(t):
    """every byte of a waited-for snapshot (a tensor, or a list of tensors) is still 0xA5"""
    import torch
    return all(bool((x.contiguous().view(torch.uint8).cpu() == SENTINEL).all()) for x in (t if isinstance(t, (list, tuple)) else [t]))
