"""The harness of tests/test_stream_order_gpu.py: an entry is called with ``stream=side`` while its input is still
on its way on ``side``, and must give the bytes it gives from that input on the default stream.

TEST INFRASTRUCTURE ONLY: the product never imports this module.

The method is deterministic.  The input buffer first holds a *stale* input and the device is synchronised.  Then,
on ``side``: a ``torch.cuda._sleep`` of a calibrated length, the write of the *real* input into the same buffer, an
event ``ready``.  The host returns to the default stream at once and calls the entry with ``stream=side``, then
waits for ``side`` alone.  Whatever part of the entry runs on another stream -- a torch copy, a memset, an inner
launch -- runs during the sleep, reads the stale input and changes the result's bytes.

Why a stale input is always VALID data of the right shape (another snapshot's field, another class array, another
label array, another finite image, other last points), never NaN-filled indices, an index out of range or
uninitialised memory: a read from the wrong stream must show as wrong bytes and nothing else.  No kernel here is
ever handed data it could take out of bounds, whichever of the two inputs it sees, or a mixture of both.

The sleep is plumbing, not a tolerance: per case it is the larger of ``MIN_DELAY_MS`` and ``DELAY_FACTOR`` times
the host wall time of the entry's warm call on the default stream (call plus device synchronisation), which bounds
the time a launch from the wrong stream needs to get onto the device.  A case that would need more than
``MAX_DELAY_MS`` fails; it never sleeps longer.
"""
import time

import numpy as np

MIN_DELAY_MS = 20.0
DELAY_FACTOR = 20.0
MAX_DELAY_MS = 500.0
FORMS = ("stream", "handle")  # the two forms engine._stream_handle accepts besides None


def to_bytes(x):
    """The bytes of a result: tensors, arrays, numbers, None, and tuples / lists / dicts (by sorted key) of them.
    Call it with the producing stream synchronised."""
    import torch
    if x is None:
        return b"<none>"
    if isinstance(x, torch.Tensor):
        a = x.detach().cpu().numpy()
        return str((a.dtype, a.shape)).encode() + np.ascontiguousarray(a).tobytes()
    if isinstance(x, np.ndarray):
        return str((x.dtype, x.shape)).encode() + np.ascontiguousarray(x).tobytes()
    if isinstance(x, dict):
        return b"".join(str(k).encode() + to_bytes(x[k]) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return b"".join(to_bytes(v) for v in x)
    if isinstance(x, (int, float, str)):
        return repr(x).encode()
    raise TypeError(f"to_bytes: {type(x).__name__}")


def first_difference(a: bytes, b: bytes) -> str:
    if len(a) != len(b):
        return f"{len(a)} bytes against {len(b)}"
    x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    d = np.flatnonzero(x != y)
    return f"{len(d)} of {len(a)} bytes differ, the first at offset {int(d[0])}" if len(d) else "no byte differs"


def copy_into(buf, src):
    """A writer: ``src`` (a CUDA tensor prepared and synchronised beforehand) into ``buf`` on torch's current
    stream."""
    def write():
        buf.copy_(src)
    return write


def rebuild(field, raw, timestep):
    """A writer: ``DeviceField.rebuild_from_device`` of the raw HBM snapshot ``raw`` on torch's current stream."""
    def write():
        import torch
        field.rebuild_from_device(raw, timestep=timestep, stream=torch.cuda.current_stream().cuda_stream)
    return write


def both(*writers):
    def write():
        for w in writers:
            w()
    return write


def under(stream, fn):
    """``fn()`` with ``stream`` (either form, or None: no change) as torch's current stream: how an entry without a
    ``stream=`` argument is put on a stream."""
    import torch
    from mops_amd import engine
    if stream is None:
        return fn()
    with torch.cuda.stream(engine._torch_stream(stream)):
        return fn()


class Harness:
    """One side stream, the sleep's calibration, the positive control and the delays used so far."""

    def __init__(self):
        import torch
        self.torch = torch
        self.side = torch.cuda.Stream()
        self.delays = []  # (case, ms)
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = 20_000_000
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.0, "the sleep kernel took no time"
        self.cycles_per_ms = cycles / ms
        self.control = self._positive_control()

    def form(self, which):
        return self.side if which == "stream" else int(self.side.cuda_stream)

    def _late(self, delay_ms, write):
        """sleep, ``write()``, event -- all on the side stream; torch's current stream is as before on return."""
        torch = self.torch
        before = torch.cuda.current_stream()
        with torch.cuda.stream(self.side):
            torch.cuda._sleep(int(delay_ms * self.cycles_per_ms))
            write()
            ready = torch.cuda.Event()
            ready.record()
        assert torch.cuda.current_stream() == before == torch.cuda.default_stream()
        return ready

    def _positive_control(self):
        """Torch only: what a read from the wrong stream and a read from the right one see of a late write.  If
        this fails, no case of the module can detect anything on this device."""
        torch = self.torch
        stale = torch.arange(4096, dtype=torch.float64, device="cuda")
        real = stale + 0.5
        buf = stale.clone()
        torch.cuda.synchronize()
        ready = self._late(MIN_DELAY_MS, copy_into(buf, real))
        wrong = buf.clone()                         # the default stream, at once
        pending = not ready.query()
        with torch.cuda.stream(self.side):
            right = buf.clone()
        torch.cuda.synchronize()
        assert pending, "positive control: the late write had landed before the reads were enqueued"
        assert to_bytes(wrong) == to_bytes(stale), "positive control: a default-stream read saw the late write"
        assert to_bytes(right) == to_bytes(real), "positive control: a side-stream read missed the late write"
        return dict(delay_ms=MIN_DELAY_MS, cycles_per_ms=self.cycles_per_ms)

    def truth(self, write, entry, before=None):
        """(bytes, warm wall seconds, result) of ``entry(None)`` from the input ``write()`` leaves, everything on
        the default stream with the device synchronised around each step."""
        torch = self.torch
        out = None
        for _ in range(2):  # cold, then warm
            write()
            if before is not None:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = entry(None)
            torch.cuda.synchronize()
            warm = time.perf_counter() - t0
        return to_bytes(out), warm, out

    def case(self, what, form, stale, real, entry, before=None, no_host_sync=False):
        """Run one case; returns (the late result, the default-stream result of the real input).

        ``stale`` / ``real``: writers of the two inputs on torch's current stream.  ``entry(stream)``: the call under
        test, returning its result; ``stream`` is None for the truths.  ``before``: state to restore on the default
        stream ahead of every call (never part of the timed call).  ``no_host_sync``: the entry is documented as
        not synchronising the host, so ``ready`` must still be pending when it returns."""
        torch = self.torch
        torch.cuda.synchronize()
        # the real input first and the stale one second: whatever state the calls leave behind is the stale run's
        want, warm, ref = self.truth(real, entry, before)
        other, _, _ = self.truth(stale, entry, before)
        assert want != other, f"{what}: the real and the stale input give the same bytes; the case proves nothing"
        delay = max(MIN_DELAY_MS, DELAY_FACTOR * warm * 1e3)
        assert delay <= MAX_DELAY_MS, (f"{what}: the warm call took {warm * 1e3:.1f} ms, which asks for a sleep of "
                                       f"{delay:.0f} ms > {MAX_DELAY_MS:.0f} ms")
        self.delays.append((f"{what}[{form}]", delay))
        print(f"{what}[{form}]: warm call {warm * 1e3:.2f} ms, delay {delay:.1f} ms")
        stale()
        if before is not None:
            before()
        torch.cuda.synchronize()
        ready = self._late(delay, real)
        queued = not ready.query()      # the late write itself did not wait for the sleep
        got = entry(self.form(form))
        pending = not ready.query()
        self.side.synchronize()         # and nothing else
        assert queued, f"{what}: the late write was not pending once enqueued (delay {delay:.1f} ms too short?)"
        if no_host_sync:
            assert pending, (f"{what}: the input had arrived when the call returned: the call synchronised the host, "
                             f"or the delay of {delay:.1f} ms was too short")
        mine = to_bytes(got)
        torch.cuda.synchronize()
        assert mine != other, f"{what}: stream={form} gave the bytes of the stale input"
        assert mine == want, f"{what}: stream={form} gave other bytes than the default stream: " + \
            first_difference(mine, want)
        return got, ref
