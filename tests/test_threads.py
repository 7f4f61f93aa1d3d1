"""The harness of test_threads_gpu.py bites, and what of the thread contract (include/neo_hip.h,
"Threads and streams") can be held without a GPU: run_threads hands a worker's exception to the
caller and the bit comparison names the worker whose result is another worker's; the Python FFT
facade passes every thread's own arrays to the plan untouched; neo_hip_last_error is per thread.
This is how a reader knows what the GPU tests detect without anyone racing a broken library on a
device."""
import ctypes
import threading
import time

import numpy as np
import pytest

from test_threads_gpu import N_THREADS, check_results, run_threads, same_bits


# ------------------------------------------------------------------ run_threads and the comparison
def test_run_threads_returns_in_order_and_runs_at_once():
    """every worker is inside its body before any leaves: the threads really overlap"""
    inside = threading.Barrier(N_THREADS)

    def worker(i):
        inside.wait(10.0)  # passes only with all eight threads running together
        return i * i

    assert run_threads(worker, N_THREADS) == [i * i for i in range(N_THREADS)]
    assert run_threads([lambda: "a", lambda: "b"]) == ["a", "b"]


def test_a_raising_worker_makes_the_call_raise():
    def worker(i):
        if i == 5:
            raise ValueError("worker five saw another thread's transform")
        return i

    with pytest.raises(ValueError, match="worker five"):
        run_threads(worker, N_THREADS)
    # a failed comparison inside a worker arrives as it is
    with pytest.raises(AssertionError, match="thread 1, call 0"):
        run_threads(lambda i: same_bits(np.full((1, 4), i, np.float32), np.zeros((1, 4), np.float32),
                                        f"thread {i}, call 0"), 2)


def test_a_stuck_worker_fails_the_call_instead_of_hanging_it():
    release = threading.Event()
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="still running after 0.2 s: worker-1"):
        run_threads([lambda: 0, lambda: release.wait(30.0)], timeout=0.2)
    assert time.monotonic() - t0 < 5.0
    release.set()  # the daemon thread ends


def test_a_wrong_array_is_named_by_worker_index():
    """worker 3 returns worker 2's result (what a shared staging buffer would hand it)"""
    rng = np.random.default_rng(3)
    want = [(rng.random((2, 16)) - 0.5).astype(np.float32) for _ in range(N_THREADS)]
    got = run_threads(lambda i: want[2 if i == 3 else i].copy(), N_THREADS)
    with pytest.raises(AssertionError, match=r"fft: worker 3, round 0: \d+ of 32 words differ, first at channel 0, column 0"):
        check_results(got, want, "fft")
    check_results([w.copy() for w in want], want, "fft")
    # rounds of one worker, and dtypes other than float32 [C][n]: one low bit of one complex element
    z = (rng.random((2, 8)) + 1j * rng.random((2, 8))).astype(np.complex64)
    bad = z.copy()
    bad.view(np.int32)[1, 7] ^= 1
    with pytest.raises(AssertionError, match=r"plan: worker 0, round 1: 1 of 16 elements differ, first at flat index 11"):
        check_results([[z.copy(), bad]], [z], "plan")
    with pytest.raises(AssertionError):  # equal values, another dtype: not the same bits
        same_bits(np.zeros(4, np.int64), np.zeros(4, np.int32), "dtype")
    nan = np.array([np.nan], np.float64)
    same_bits(nan, nan.copy(), "NaNs compare as bit patterns")


# ------------------------------------------------------------------ the Python plan cache under threads
def test_plan_cache_under_threads(monkeypatch):
    """Eight threads call neo.fft.fft on the same shape with different data; the plan is a stub
    whose execute_host marks "inside", sleeps 1 ms and writes out[:] = a * 2.

    The cache keeps handing ONE plan to every thread (get_plan is unchanged: same key, same
    object), so calls on it do overlap here; excluding them from the plan's staging buffers is the C
    library's job (the mutex of neo_hip_fft_plan, fft.hip) and is tested on the GPU
    (test_threads_gpu.py::test_fft_facade_from_threads, test_one_plan_many_threads_c_abi). What the
    facade owes that design is asserted here: it passes each thread's own input array and a
    fresh output array of its own to the plan, and returns that very array, so nothing but the
    plan is shared between two calls. The fix did not touch the Python layer: every assertion
    here also holds on the parent commit's Python."""
    import neo
    from neo.fft import _plan

    class StubPlan:
        made = []

        def __init__(self, kind, order, batch=1, device=0):
            self.key = (kind, order, batch, device)
            self.lock = threading.Lock()
            self.inside = 0
            self.overlapped = False
            self.calls = []  # (thread, id of a, id of out)
            StubPlan.made.append(self)

        def execute_host(self, a, out, direction):
            with self.lock:
                self.inside += 1
                self.overlapped |= self.inside > 1
                self.calls.append((threading.get_ident(), a.ctypes.data, out.ctypes.data))
            time.sleep(0.001)
            out[:] = a * 2
            with self.lock:
                self.inside -= 1

        def close(self):
            pass

    monkeypatch.setattr(_plan, "FFTPlan", StubPlan)
    monkeypatch.setattr(_plan, "_cache", {})
    rng = np.random.default_rng(5)
    xs = [(rng.random((4, 64)) + 1j * rng.random((4, 64))).astype(np.complex64) for _ in range(N_THREADS)]
    before = [x.copy() for x in xs]

    def worker(i):
        outs = [neo.fft.fft(xs[i]) for _ in range(20)]
        return threading.get_ident(), outs

    results = run_threads(worker, N_THREADS)
    for i, (_, outs) in enumerate(results):
        for r, y in enumerate(outs):
            same_bits(y, before[i] * 2, f"thread {i}, call {r}")  # its own data doubled
        same_bits(xs[i], before[i], f"thread {i}: input changed")
    assert len(StubPlan.made) == 1, "one shape, one plan: the cache shares it between the threads"
    plan = StubPlan.made[0]
    assert plan.key == (neo._native.C2C, 6, 4, 0)
    assert plan.overlapped, "the calls on the shared plan overlap in Python: exclusion is the C library's"
    assert len(plan.calls) == 20 * N_THREADS
    mine = {ident: i for i, (ident, _) in enumerate(results)}
    outs_seen = set()
    for ident, a_ptr, out_ptr in plan.calls:
        i = mine[ident]
        assert a_ptr == xs[i].ctypes.data, f"thread {i}: the plan did not get the caller's own input array"
        assert all(out_ptr != x.ctypes.data for x in xs), "the output aliases an input"
        outs_seen.add(out_ptr)
    returned = {y.ctypes.data for _, outs in results for y in outs}
    assert returned == outs_seen and len(returned) == 20 * N_THREADS, "every call returns the array the plan wrote"


# ------------------------------------------------------------------ neo_hip_last_error
def test_last_error_is_per_thread():
    """Two threads, 200 rounds each of a refused call followed by neo_hip_last_error(): thread A
    (an FFT plan of order 28) must read "max_order", thread B (a convolver of block 100) "power of
    two", never the other's message. No device is touched: both are refused on the host."""
    import neo

    lib = neo._native.load()
    EINVAL = neo._native.NEO_HIP_EINVAL

    def fft_order(_):
        h = ctypes.c_void_p()
        return lib.neo_hip_fft_plan_create(28, 1, 0, 0, ctypes.byref(h))

    def upols_block(_):
        h = ctypes.c_void_p()
        return lib.neo_hip_upols_create(1, 100, 3, 0, ctypes.byref(h))

    def worker(call, mine, other):
        for r in range(200):
            assert call(r) == EINVAL
            msg = lib.neo_hip_last_error()
            assert mine in msg and other not in msg, (r, msg)
        return lib.neo_hip_last_error()

    a, b = run_threads([lambda: worker(fft_order, b"max_order", b"power of two"),
                        lambda: worker(upols_block, b"power of two", b"max_order")])
    assert b"unsupported order '28'" in a and b"got 100" in b
    # and a thread that made no failing call has no message of theirs
    assert run_threads([lambda: lib.neo_hip_last_error()]) == [b""]
