"""Offline windows of the double-precision UPOLS / UPOLA convolvers on the device
(neo.UpolsConvolver64.set_offline, csrc/upols_f64_offline.hip) against the float64 numpy truth of
tests/upols_f64_truth.py at its TOL, 1e-12 of the peak (tests/test_upols_f64_offline.py shows on the
CPU that the window rule is that algorithm within 1e-13): the value shapes of
tests/upols_f64_offline_replay.py; windows, batched passes and plain steps mixed on one handle; the
setup calls and the stale-spectra flag; bits across equal calls; the I/O contract of neo_hip.h by the
arena method; refusals; a NaN block; dense_convolve; the info calls and the pool bytes."""
import numpy as np
import pytest

import upols_f64_offline_replay as R
import upols_f64_truth as T
from test_upols_f64_gpu import IN_FILL, OUT_FILL, PAD_IN, PAD_OUT, check_regions, same_bits

pytestmark = pytest.mark.gpu

OFF = {"blocks_per_pass": 0, "segments": 0, "spectra_bytes": 0, "extra_bytes": 0}


@pytest.fixture(scope="module")
def torch(neo_gpu):
    import torch as t

    return t


def run(torch, neo, C, B, P, method, H, x, calls=None, batch=False):
    """A fresh handle, the filter H, x [C][n] through it on the device. calls: [(blocks, offline)]
    (None: one call with offline windows on); batch: set_batch for the whole run. The output and
    offline_info() as it stood last."""
    conv = neo.UpolsConvolver64(C, B, P, method=method)
    conv.filter(H)
    conv.set_batch(batch)
    t = torch.from_numpy(np.array(x)).cuda()
    n = x.shape[1]
    o = 0
    for k, offline in calls or [(n // B, True)]:
        conv.set_offline(offline)
        conv.process_device(t.data_ptr() + 8 * o, n, t.data_ptr() + 8 * o, n, n=k * B)
        o += k * B
    assert o == n
    torch.cuda.synchronize()
    info = conv.offline_info()
    conv.close()
    return t.cpu().numpy(), info


# ------------------------------------------------------------------ values against truth
@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb", R.VALUE_SHAPES)
def test_values_against_truth(torch, neo_gpu, C, B, P, nb, method):
    """Whole windows in one call. P < 128: one segment, a ring shorter than a window, the zero rows,
    the commit of min(128, P) rows; 128 / 129: the segment boundary and a last segment of one
    partition; 257: three segments; B = 16, 128, 512, 4096: every class of the block transforms."""
    ir, H, x = T.problem(C, B, P, nb)
    y, info = run(torch, neo_gpu, C, B, P, method, H, x)
    plan = neo_gpu.upols64_offline_plan(C, B, P, method)
    assert info == {k: plan[k] for k in OFF} and info["blocks_per_pass"] == 128 and info["segments"] == R.segments(P)
    err = T.peak_err(y, T.truth(C, B, P, method, nb))
    print(f"{C} x {B} x {P}, {nb} blocks {method}: {err:.3g}")
    assert err <= T.TOL, err


# ------------------------------------------------------------------ the three gears on one handle
@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("P", [3, 129, 200])
def test_window_batched_pass_and_steps_in_one_call(torch, neo_gpu, method, P):
    """5 plain steps (so w = 5 mod P and the ring wraps inside a pair), then one call of 128 + 16 + 3 blocks
    with batching on: a window, a batched pass, three steps; then 256 blocks: two windows."""
    C, B = 3, 16
    calls = [(5, True), (128 + 16 + 3, True), (256, True)]
    nb = sum(k for k, _ in calls)
    ir, H, x = T.problem(C, B, P, nb)
    y, _ = run(torch, neo_gpu, C, B, P, method, H, x, calls, batch=16)
    err = T.peak_err(y, T.truth(C, B, P, method, nb))
    print(f"P {P} {method}: steps, window + pass + steps, windows vs truth {err:.3g}")
    assert err <= T.TOL, err


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_turning_the_mode_off_and_on_between_calls(torch, neo_gpu, method):
    """128 blocks as a window, 130 with the mode off (plain steps), 128 as a window again: against
    truth at TOL, and within 2 TOL of a handle that ran every block as a plain step."""
    C, B, P = 3, 16, 129
    calls = [(128, True), (130, False), (128, True)]
    nb = sum(k for k, _ in calls)
    ir, H, x = T.problem(C, B, P, nb)
    y, info = run(torch, neo_gpu, C, B, P, method, H, x, calls)
    assert info["blocks_per_pass"] == 128
    plain, off = run(torch, neo_gpu, C, B, P, method, H, x, [(nb, False)])
    assert off == OFF
    want = T.truth(C, B, P, method, nb)
    err, diff = T.peak_err(y, want), T.peak_err(y, plain)
    print(f"{method}: toggled vs truth {err:.3g}, vs plain steps {diff:.3g}")
    assert err <= T.TOL and T.peak_err(plain, want) <= T.TOL and diff <= 2 * T.TOL


# ------------------------------------------------------------------ setup calls
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_reset_set_filter_and_set_impulse(torch, neo_gpu, method):
    """One handle, 133 blocks (a window and five steps) after: nothing, reset, set_filter with another
    filter and a window pass with it, set_filter back, set_impulse. Every run with the first filter
    equals a fresh handle's bit for bit, and so does the run with the other one: the segment spectra
    follow the filter."""
    C, B, P, nb = 3, 16, 129, 133
    ir, _, x = T.problem(C, B, P, nb)
    H = neo_gpu.uniform_partition(np.array(ir), B, dtype=np.float64)
    H2 = np.ascontiguousarray(H[:, ::-1]) * 0.5
    want, _ = run(torch, neo_gpu, C, B, P, method, H, x)
    want2, _ = run(torch, neo_gpu, C, B, P, method, H2, x)
    assert T.peak_err(want, T.truth(C, B, P, method, nb)) <= T.TOL
    assert T.peak_err(want2, want) > 1e-3
    conv = neo_gpu.UpolsConvolver64(C, B, P, method=method)
    conv.filter(H)
    conv.set_offline(True)
    on = conv.offline_info()
    outs = []
    for setup in (lambda: None, conv.reset, lambda: conv.filter(H2), lambda: conv.filter(H),
                  lambda: conv.set_impulse(np.array(ir), normalize=False)):
        setup()
        assert conv.offline_info() == on  # the setup calls leave the mode as it is
        t = torch.from_numpy(np.array(x)).cuda()
        conv.process(t)
        outs.append(t.cpu().numpy())
    conv.close()
    for i, y in enumerate(outs):
        same_bits(y, want2 if i == 2 else want, f"run {i} on one handle")


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_equal_calls_give_equal_bits(torch, neo_gpu, method):
    C, B, P, nb = 3, 16, 129, 256
    ir, H, x = T.problem(C, B, P, nb)
    a, _ = run(torch, neo_gpu, C, B, P, method, H, x)
    assert T.peak_err(a, T.truth(C, B, P, method, nb)) <= T.TOL
    b, _ = run(torch, neo_gpu, C, B, P, method, H, x)
    same_bits(b, a, "two fresh handles, the same calls")
    c, _ = run(torch, neo_gpu, C, B, P, method, H, x, [(128, True), (128, True)])
    same_bits(c, a, "two calls of 128 blocks against one call of 256 blocks")
    conv = neo_gpu.UpolsConvolver64(C, B, P, method=method)
    conv.filter(H)
    conv.set_offline(True)
    h = np.array(x)
    assert conv.process(h) is h
    conv.close()
    same_bits(h, a, "host buffers against device buffers")


# ------------------------------------------------------------------ where it reads and writes
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_io_contract_in_padded_arenas(torch, neo_gpu, method, host):
    """The arenas of tests/test_upols_f64_gpu.py over a call of 128 + 3 blocks, a window and a
    remainder: separate buffers of unequal even strides, and in place; nothing written outside the
    payload, the input left as it was, the payloads equal to the contiguous run bit for bit."""
    C, B, P, nb = 3, 16, 129, 131
    ir, H, x = T.problem(C, B, P, nb)
    n = x.shape[1]
    A, _ = run(torch, neo_gpu, C, B, P, method, H, x)
    assert T.peak_err(A, T.truth(C, B, P, method, nb)) <= T.TOL

    def arena(ld, fill, data=None):
        a = np.full((C + 2, ld), fill, dtype=np.int64)
        if data is not None:
            a.view(np.float64)[1:C + 1, :n] = data
        buf = a if host else torch.from_numpy(a).cuda()
        base = a.ctypes.data if host else buf.data_ptr()
        return buf, base + 8 * ld

    def read(buf):
        return buf.copy() if host else buf.cpu().numpy()

    def go(ip, li, op, lo):
        conv = neo_gpu.UpolsConvolver64(C, B, P, method=method)
        conv.filter(H)
        conv.set_offline(True)
        conv.process_device(ip, li, op, lo, n=n, is_device=not host)
        torch.cuda.synchronize()
        conv.close()

    ia, ip = arena(n + PAD_IN, IN_FILL, x)
    oa, op = arena(n + PAD_OUT, OUT_FILL)
    before = read(ia)
    go(ip, n + PAD_IN, op, n + PAD_OUT)
    same_bits(check_regions(read(oa), C, n, OUT_FILL, before, read(ia)), A, "separate padded buffers")
    pa, pp = arena(n + PAD_OUT, IN_FILL, x)
    go(pp, n + PAD_OUT, pp, n + PAD_OUT)
    same_bits(check_regions(read(pa), C, n, IN_FILL), A, "in place, padded")


def test_refusals_do_not_advance_state(torch, neo_gpu):
    """With the mode on, a ragged sample count, an odd stride, a misaligned base and a bad enable are
    refused; the next valid call gives what a handle that never saw them gives."""
    C, B, P = 3, 16, 129
    first, nb = 129, 129 + 130
    ir, H, x = T.problem(C, B, P, nb)
    n = x.shape[1]
    half = first * B
    want, _ = run(torch, neo_gpu, C, B, P, "upols", H, x, [(first, True), (nb - first, True)])
    conv = neo_gpu.UpolsConvolver64(C, B, P)
    conv.filter(H)
    conv.set_offline(True)
    on = conv.offline_info()
    t = torch.from_numpy(np.array(x)).cuda()
    p = t.data_ptr()
    conv.process_device(p, n, p, n, n=half)
    for li, lo, k, ptr in ((n, n, 128 * B - 8, p), (n, n, 128 * B + 2, p), (n + 1, n, 128 * B, p), (n, n + 3, 128 * B, p),
                           (n, n, 128 * B, p + 8)):
        with pytest.raises(neo_gpu._native.NeoHipError) as e:
            conv.process_device(ptr + 8 * half, li, ptr + 8 * half, lo, n=k)
        assert e.value.code == neo_gpu._native.NEO_HIP_EINVAL
    for bad in (2, -1):
        with pytest.raises(neo_gpu._native.NeoHipError) as e:
            conv.set_offline(bad)
        assert e.value.code == neo_gpu._native.NEO_HIP_EINVAL
    assert conv.offline_info() == on
    conv.process_device(p + 8 * half, n, p + 8 * half, n, n=n - half)
    torch.cuda.synchronize()
    conv.close()
    same_bits(t.cpu().numpy(), want, "after the refused calls")


# ------------------------------------------------------------------ Inf / NaN
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_a_nan_block_stays_in_its_channel_and_its_windows(torch, neo_gpu, method):
    """Three channels, P = 129 (two segments), five windows; a NaN in block 130 of channel 1. Channels 0
    and 2 equal a clean run bit for bit; channel 1 does in the window before the NaN's; the NaN's
    window is non-finite; channel 1 is finite again from the first window that starts at a block t_W
    with t_W - 256 > 130, that is 512 (overlap-add: from 513, the block after carries the tail)."""
    C, B, P, nb, bad = 3, 16, 129, 640, 130
    ir, H, x = T.problem(C, B, P, nb)
    clean, _ = run(torch, neo_gpu, C, B, P, method, H, x)
    assert T.peak_err(clean, T.truth(C, B, P, method, nb)) <= T.TOL
    xn = np.array(x)
    xn[1, bad * B + 5] = np.nan
    y, _ = run(torch, neo_gpu, C, B, P, method, H, xn)
    same_bits(y[[0, 2]], clean[[0, 2]], "the other channels")
    same_bits(y[1:2, :128 * B], clean[1:2, :128 * B], "channel 1 before the NaN's window")
    assert not np.isfinite(y[1, 128 * B:256 * B]).any(), "every block of the NaN's window"
    nseg = R.segments(P)
    again = next(tw for tw in range(0, nb, 128) if tw - 128 * nseg > bad)
    assert again == 512
    lo = (again + (method == "upola")) * B
    assert np.isfinite(y[1, lo:]).all()
    assert T.peak_err(y[1:2, lo:], clean[1:2, lo:]) <= 2 * T.TOL


# ------------------------------------------------------------------ the rest
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_dense_convolve_f64_offline_with_a_ragged_tail(neo_gpu, method):
    rng = np.random.default_rng(13)
    C, B = 2, 16
    N, L = B * (128 + 16 + 5) + 9, B * 130 + 7  # a window, a batched pass and steps; two segments
    x, ir = rng.standard_normal((C, N)), rng.standard_normal((C, L))
    want = T.whole(x, T.normalize(ir))
    for batch in (False, True):
        y = neo_gpu.dense_convolve(x, ir, B, method=method, dtype=np.float64, offline=True, batch=batch)
        assert y.dtype == np.float64 and y.shape == (C, N)
        err = T.peak_err(y, want)
        print(f"dense_convolve offline=True batch={batch} {method}: {err:.3g}")
        assert err <= T.TOL


def test_offline_info_and_the_pool_bytes(neo_gpu):
    """offline_info before, while and after the mode; memory_info shows the pool bytes taken while it is
    on and given back by set_offline(False) and by close()."""
    for C, B, P, method in ((3, 128, 200, "upols"), (3, 128, 200, "upola"), (2, 16, 1, "upols")):
        start = neo_gpu.memory_info()["in_use"]
        conv = neo_gpu.UpolsConvolver64(C, B, P, method=method)
        state, base = conv.info(), neo_gpu.memory_info()["in_use"]
        assert conv.offline_info() == OFF
        plan = neo_gpu.upols64_offline_plan(C, B, P, method)
        want = {k: plan[k] for k in OFF}
        for _ in range(2):
            conv.set_offline(True)
            assert conv.offline_info() == want and conv.info() == state
            conv.set_offline(True)  # on already: nothing more is taken
            held = neo_gpu.memory_info()["in_use"] - base
            assert plan["spectra_bytes"] + plan["extra_bytes"] <= held <= plan["spectra_bytes"] + plan["extra_bytes"] + 4 * 4096
            conv.set_offline(False)
            assert conv.offline_info() == OFF and neo_gpu.memory_info()["in_use"] == base
        conv.set_offline(True)
        conv.close()
        assert neo_gpu.memory_info()["in_use"] == start
