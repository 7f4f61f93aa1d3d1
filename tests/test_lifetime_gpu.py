"""Setup and destroy calls with the caller's stream still busy.

Freeing device memory is a list operation of the pool (csrc/dmem.hip): nothing waits for the
device, and a freed range goes straight to the next allocation. What stands between a queued
kernel and recycled memory is the join discipline: every asynchronous entry point remembers its
stream in the handle's stream_set (csrc/common.hpp), and every call that frees, reallocates or
rewrites a buffer from the host first joins those streams. Every other GPU test synchronizes
before such a call, so none of them needs the discipline; these do.

Each case (tests/lifetime_cases.py) runs one script twice on fresh objects:

  serial  torch.cuda.synchronize() after every call; checked against the oracle (float32: 1e-5 of
          the peak) or the float64 numpy statement (upols_f64_truth.TOL)
  held    a side stream is held back by HOLD_US of filler (tests/stream_holds.py), the object's
          work is queued on it through the wrappers' stream arguments, and an event recorded
          after the last queued call must still be pending (else the case FAILS: the hold was too
          short). Then the call under test, with host (numpy) arguments and torch's current stream
          the default stream, so that no synchronization of the Python layer stands in for the
          library's join. Calls marked J (close, filter, set_impulse, reset, a host update_filter,
          the matrix and float64 mode setters, an FFT plan's or overlap stage's close, the note
          that overflows a stream_set) must leave that event complete. Then a second object of
          the same kind and shape is brought up (first fit hands it the ranges just freed), loads
          the other filter and runs two blocks on the default stream; the first object, where it
          lives on, steps more blocks on the side stream.

Every output of the held run (the queued work, the blocks after the call, the second object's
blocks) equals the serial run's bit for bit: equal calls give equal bits in this library. The
reuse step must not grow neo.memory_info()["reserved"]. (With chunks of 256 MiB that is all the
counters can show: that no new chunk was mapped, not which ranges were handed out.)

The hold: ten times the largest host time of a serial run from the first queued call to the
return of the call under test, at least 20 ms. Measured on an MI355X, in ms, in the order the
cases run (the first case of a kind also loads its kernels):

  dense-a-upols-close 8.4, dense-a-upols-filter 0.5, dense-a-upols-set_impulse 0.5,
  dense-a-upols-reset 0.4, dense-a-upols-update_filter 0.5, dense-a-upola-close 0.4,
  dense-a-upola-filter 0.4, dense-a-upola-set_impulse 0.4, dense-a-upola-reset 0.4,
  dense-a-upola-update_filter 0.4, dense-b-upols-close 11.0, dense-b-upols-filter 4.1,
  dense-b-upols-set_impulse 3.6, dense-b-upols-reset 4.8, dense-b-upols-update_filter 3.1,
  dense-b-upola-close 3.3, dense-b-upola-filter 3.6, dense-b-upola-set_impulse 4.9,
  dense-b-upola-reset 3.5, dense-b-upola-update_filter 3.1, dense-c-upols-close 5.1,
  dense-c-upols-filter 0.5, dense-c-upols-set_impulse 0.7, dense-c-upols-reset 0.6,
  dense-c-upols-update_filter 0.5, dense-c-upola-close 0.5, dense-c-upola-filter 0.6,
  dense-c-upola-set_impulse 0.7, dense-c-upola-reset 0.5, dense-c-upola-update_filter 0.5,
  dense-b-upols-set_ahead 3.3, dense-b-upola-set_ahead 3.1, dense-c-upols-set_batch 0.1,
  dense-c-upola-set_batch 0.2, dense-c-upols-set_offline 0.1, dense-c-upola-set_offline 0.2,
  sparse-upols-close 0.2, sparse-upols-filter 0.2, sparse-upols-update_reset 0.9,
  sparse-upola-close 0.1, sparse-upola-filter 0.2, sparse-upola-update_reset 0.2,
  f64-upols-close 2.1, f64-upols-filter 0.1, f64-upols-reset 0.1, f64-upols-set_batch 0.1,
  f64-upola-close 0.1, f64-upola-filter 0.1, f64-upola-reset 0.1, f64-upola-set_batch 0.1,
  matrix-upols-P9-close 0.2, matrix-upols-P9-filter 0.2, matrix-upols-P9-update_filter 0.2,
  matrix-upols-P9-set_batch 0.2, matrix-upols-P130-set_offline 0.2,
  matrix-upols-P130-set_levels 0.2, matrix-upola-P9-close 0.2, matrix-upola-P9-filter 0.2,
  matrix-upola-P9-update_filter 0.2, matrix-upola-P9-set_batch 0.2,
  matrix-upola-P130-set_offline 0.2, matrix-upola-P130-set_levels 0.2, overlap-save 3.4,
  overlap-add 0.2, fft-0-13-2 0.1, fft-16-13-2 0.1, fft-1-14-1 0.1, stream-set-overflow 0.3

The largest is 11.0 ms (140 single-block calls with a synchronize each), so every case holds
its stream for HOLD_US = 110 ms (the cases with two held calls twice); a run of the whole
module takes about 10 s. The serial runs came out within 5.4e-7 of the peak (float32) of the
oracle. A J call can also pass because the handle's own stream and the held one share a hardware
queue (the library's join of its own stream then waits for the hold): with the join of the matrix
convolver's host update missing, the upols case failed its J assertion and the upola case passed.

Checked by hand against three builds with one line removed each, the held dense, sparse and overflow
cases (43) or the FFT cases (3) once: without note_stream in launch_step and process_samples 18
cases failed (all on J, 13 of them on the bits of the queued blocks too); without used.join() in
setup_join 16 (13 on both, 2 on J alone, 1 on the bits alone); without the join in free_plan all
three FFT cases, on J alone (the second plan's tables hold the same values). The cases that passed
are those whose handle drew the shared stream that queues behind the held one.
"""
import numpy as np
import pytest

import lifetime_cases as L
from conftest import peak_err

pytestmark = pytest.mark.gpu

HOLD_US = 110_000.0  # ten times the largest serial host time above

IDS = [c[0] for c in L.CASES]
_serial = {}


def serial(neo, torch, oracle, i):
    if i not in _serial:
        name, run, case = L.CASES[i]
        _serial[i] = run(neo, torch, oracle, case, "serial", 0.0)
        print(f"lifetime {name} serial: host {1e3 * _serial[i][3]:.2f} ms from the first queued call to the return of "
              "the call under test")
    return _serial[i]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize % 8 == 0 else np.uint32)


@pytest.mark.parametrize("i", range(len(L.CASES)), ids=IDS)
def test_serial_matches_truth(neo_gpu, oracle, i):
    torch = pytest.importorskip("torch")
    outs, truths, problems, _ = serial(neo_gpu, torch, oracle, i)
    assert not problems, problems
    assert set(truths) == set(outs) - {"spectra"}
    for k, (ref, tol) in truths.items():
        err = peak_err(outs[k], ref)
        print(f"lifetime {IDS[i]} serial {k}: peak error {err:.2e}")
        assert err <= tol, (IDS[i], k, err)


@pytest.mark.parametrize("i", range(len(L.CASES)), ids=IDS)
def test_held_equals_serial(neo_gpu, oracle, i):
    torch = pytest.importorskip("torch")
    want = serial(neo_gpu, torch, oracle, i)[0]
    name, run, case = L.CASES[i]
    try:
        outs, _, problems, _ = run(neo_gpu, torch, oracle, case, "held", HOLD_US)
    finally:
        torch.cuda.synchronize()
    problems = list(problems)
    assert set(outs) == set(want)
    for k in want:
        a, b = _bits(outs[k]), _bits(want[k])
        if not np.array_equal(a, b):
            problems.append(f"bits: {k}: {int((a != b).sum())} of {a.size} words differ from the serial run "
                            f"(peak error {peak_err(outs[k], want[k]):.3g})")
    print(f"lifetime {name} held: hold {HOLD_US:.0f} us, {len(problems)} problems")
    if problems:
        pytest.fail(f"{name}: " + "; ".join(problems))
