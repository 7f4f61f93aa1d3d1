"""Hold a stream back on purpose: hold(stream, microseconds) enqueues a filler kernel of about
that length, on a torch stream or on a raw hipStream_t (wrapped with torch.cuda.ExternalStream);
hold_background(conv, microseconds) does so on a convolver's step-group background stream, fetched
from the handle every time (a setup call may have destroyed it) and skipped while there is none.

The filler is torch.cuda._sleep (a spin on the device clock), its cycles per microsecond measured
once per session between a pair of timing events, at two lengths so that the launch's own cost
drops out. Where _sleep cannot be used the filler is an in-place elementwise multiply on a tensor
whose size comes from the same two-point measurement. A plain module: the ordering tests import it."""
import torch

_FILL_ELEMS = 1 << 22  # the fallback filler's largest tensor (16 MiB)
_cal = None            # ("sleep", cycles per us) or ("mul", elements per us, buffer)


def _time_us(fn):
    fn()  # the first launch loads the kernel
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _slope(fn, n0, n1):
    """units of n per microsecond from the times at two lengths (the best of three each)"""
    t0 = min(_time_us(lambda: fn(n0)) for _ in range(3))
    t1 = min(_time_us(lambda: fn(n1)) for _ in range(3))
    if not t1 > t0 + 20.0:
        raise RuntimeError(f"filler does not scale: {n0} -> {t0:.1f} us, {n1} -> {t1:.1f} us")
    return (n1 - n0) / (t1 - t0)


def calibrate():
    global _cal
    if _cal is None:
        try:
            _cal = ("sleep", _slope(lambda n: torch.cuda._sleep(int(n)), 200_000, 2_000_000))
        except Exception:  # no usable _sleep on this device: a fixed elementwise op instead
            buf = torch.ones(_FILL_ELEMS, dtype=torch.float32, device="cuda")
            _cal = ("mul", _slope(lambda n: buf[:int(n)].mul_(1.0), _FILL_ELEMS // 8, _FILL_ELEMS), buf)
    return _cal


def as_stream(stream):
    return stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream))


def hold(stream, microseconds):
    """enqueue about `microseconds` of filler on `stream` (a torch stream or a raw stream pointer)"""
    cal = calibrate()
    n = max(1, int(cal[1] * microseconds))
    with torch.cuda.stream(as_stream(stream)):
        if cal[0] == "sleep":
            torch.cuda._sleep(n)
        else:
            left = n
            while left > 0:  # longer than the buffer: several launches
                cal[2][:min(left, _FILL_ELEMS)].mul_(1.0)
                left -= _FILL_ELEMS


def hold_background(conv, microseconds):
    """the same on the convolver's background stream; False (no hold) while it has none"""
    ptr = conv.background_stream()
    if not ptr:
        return False
    hold(ptr, microseconds)
    return True
