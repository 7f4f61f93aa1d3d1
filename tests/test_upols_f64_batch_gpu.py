"""Batched passes of the double-precision UPOLS / UPOLA convolvers on the device
(neo.UpolsConvolver64.set_batch, csrc/upols_f64_batch.hip) against the float64 numpy truth of
tests/upols_f64_truth.py at its TOL, 1e-12 of the peak (tests/test_upols_f64_batch.py shows on the
CPU that the pass's index rule is that algorithm within 1e-13); their bits across equal calls; passes
and plain steps interleaved on one handle; the I/O contract of neo_hip.h by the arena method; refusals
and the setup calls."""
import numpy as np
import pytest

import upols_f64_batch_replay as R
import upols_f64_truth as T
from test_upols_f64_gpu import IN_FILL, OUT_FILL, PAD_IN, PAD_OUT, check_regions, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch(neo_gpu):
    import torch as t

    return t


def run(torch, neo, C, B, P, method, H, x, batch, split=0, calls=None):
    """A fresh handle, the filter H, x [C][n] through it on the device. calls: [(blocks, batched)]
    (None: one call with set_batch(batch)); the output, the batch info as it stood last."""
    conv = neo.UpolsConvolver64(C, B, P, method=method, split_workgroups=split)
    conv.filter(H)
    t = torch.from_numpy(np.array(x)).cuda()
    n = x.shape[1]
    o = 0
    for k, batched in calls or [(n // B, bool(batch))]:
        conv.set_batch(batch if batched else False)
        conv.process_device(t.data_ptr() + 8 * o, n, t.data_ptr() + 8 * o, n, n=k * B)
        o += k * B
    assert o == n
    torch.cuda.synchronize()
    info = conv.batch_info()
    conv.close()
    return t.cpu().numpy(), info


# ------------------------------------------------------------------ values against truth
@pytest.mark.parametrize("Tb", [8, 16])
@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P", T.VALUE_SHAPES)
def test_values_against_truth(torch, neo_gpu, C, B, P, method, Tb):
    """2T + 3 blocks in one call: two passes and a remainder of three plain steps. P in {1, 3, 9}: the
    ring wraps inside a pass; P = 70: four splits asked for (18, 18, 18, 16), so splits start at
    p0 > 0 and the last one is short."""
    nb = 2 * Tb + 3
    ir, H, x = T.problem(C, B, P, nb)
    split = T.forced_split(C) if P == 70 else 0
    y, info = run(torch, neo_gpu, C, B, P, method, H, x, Tb, split)
    S, rows = R.batch_rule(C, B, P, Tb, split)
    assert info["blocks_per_pass"] == Tb and info["splits"] == S and (P != 70 or (S, rows) == (4, 18))
    for statement in ("blockwise", "whole"):
        err = T.peak_err(y, T.truth(C, B, P, method, nb, statement=statement))
        print(f"{C} x {B} x {P} {method} T {Tb} (S {S}, rows {rows}) vs {statement}: {err:.3g}")
        assert err <= T.TOL, (statement, err)


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_values_block_4096(torch, neo_gpu, method):
    C, B, P = T.BIG_SHAPE
    Tb = neo_gpu.upols64_batch_plan(C, B, P, method)["blocks_per_pass"]
    nb = Tb + 2
    ir, H, x = T.problem(C, B, P, nb)
    y, _ = run(torch, neo_gpu, C, B, P, method, H, x, True)
    for statement in ("blockwise", "whole"):
        err = T.peak_err(y, T.truth(C, B, P, method, nb, statement=statement))
        print(f"{C} x {B} x {P} {method} T {Tb} vs {statement}: {err:.3g}")
        assert err <= T.TOL, (statement, err)


# ------------------------------------------------------------------ passes and steps on one handle
@pytest.mark.parametrize("Tb", [8, 16])
@pytest.mark.parametrize("P", [3, 70])
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_passes_and_steps_interleave(torch, neo_gpu, method, P, Tb):
    """(3 plain, T + 5 batched, 2 plain, 2T batched) blocks on one handle, set_batch toggled between
    the calls: against truth at TOL, and against a handle that ran every block as a plain step
    within 2 TOL (each is within TOL of the truth)."""
    C, B = 3, 128
    calls = R.sequence(Tb)
    nb = sum(k for k, _ in calls)
    ir, H, x = T.problem(C, B, P, nb)
    split = T.forced_split(C) if P == 70 else 0
    y, info = run(torch, neo_gpu, C, B, P, method, H, x, Tb, split, calls)
    assert info["blocks_per_pass"] == Tb
    plain, off = run(torch, neo_gpu, C, B, P, method, H, x, False, split)
    assert off == {"blocks_per_pass": 1, "splits": 1, "extra_bytes": 0}
    err, diff = T.peak_err(y, T.truth(C, B, P, method, nb)), T.peak_err(y, plain)
    print(f"P {P} {method} T {Tb}: interleaved vs truth {err:.3g}, vs plain steps {diff:.3g}")
    assert err <= T.TOL and T.peak_err(plain, T.truth(C, B, P, method, nb)) <= T.TOL
    assert diff <= 2 * T.TOL


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_equal_calls_give_equal_bits(torch, neo_gpu, method):
    C, B, P, Tb = 3, 128, 70, 16
    nb = 2 * Tb
    ir, H, x = T.problem(C, B, P, nb)
    a, _ = run(torch, neo_gpu, C, B, P, method, H, x, Tb)
    assert T.peak_err(a, T.truth(C, B, P, method, nb)) <= T.TOL
    b, _ = run(torch, neo_gpu, C, B, P, method, H, x, Tb)
    same_bits(b, a, "two fresh handles, the same calls")
    c, _ = run(torch, neo_gpu, C, B, P, method, H, x, Tb, calls=[(Tb, True), (Tb, True)])
    same_bits(c, a, "two calls of T blocks against one call of 2T blocks")
    conv = neo_gpu.UpolsConvolver64(C, B, P, method=method)
    conv.filter(H)
    conv.set_batch(Tb)
    h = np.array(x)
    assert conv.process(h) is h
    conv.close()
    same_bits(h, a, "host buffers against device buffers")


# ------------------------------------------------------------------ where it reads and writes
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_io_contract_in_padded_arenas(torch, neo_gpu, method, host):
    """The arenas of tests/test_upols_f64_gpu.py over a call of T + 3 blocks, a pass and a remainder:
    separate buffers of unequal even strides, and in place; nothing written outside the payload, the
    input left as it was, the payloads equal to the contiguous run bit for bit."""
    C, B, P, Tb = 3, 128, 9, 8
    nb = Tb + 3
    ir, H, x = T.problem(C, B, P, nb)
    n = x.shape[1]
    A, _ = run(torch, neo_gpu, C, B, P, method, H, x, Tb)
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
        conv.set_batch(Tb)
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
    """With batching on, a ragged sample count, an odd stride and a misaligned base are refused; the
    next valid call gives what a handle that never saw them gives."""
    C, B, P, Tb = 3, 128, 9, 8
    nb = 2 * Tb + 3
    ir, H, x = T.problem(C, B, P, nb)
    n = x.shape[1]
    half = (Tb + 1) * B
    want, _ = run(torch, neo_gpu, C, B, P, "upols", H, x, Tb, calls=[(Tb + 1, True), (Tb + 2, True)])
    conv = neo_gpu.UpolsConvolver64(C, B, P)
    conv.filter(H)
    conv.set_batch(Tb)
    t = torch.from_numpy(np.array(x)).cuda()
    p = t.data_ptr()
    conv.process_device(p, n, p, n, n=half)
    for li, lo, k, ptr in ((n, n, Tb * B - 16, p), (n, n, Tb * B + 2, p), (n + 1, n, Tb * B, p), (n, n + 3, Tb * B, p),
                           (n, n, Tb * B, p + 8)):
        with pytest.raises(neo_gpu._native.NeoHipError) as e:
            conv.process_device(ptr + 8 * half, li, ptr + 8 * half, lo, n=k)
        assert e.value.code == neo_gpu._native.NEO_HIP_EINVAL
    with pytest.raises(neo_gpu._native.NeoHipError):
        conv.set_batch(5)
    assert conv.batch_info()["blocks_per_pass"] == Tb
    conv.process_device(p + 8 * half, n, p + 8 * half, n, n=n - half)
    torch.cuda.synchronize()
    conv.close()
    same_bits(t.cpu().numpy(), want, "after the refused calls")


# ------------------------------------------------------------------ setup calls
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_set_filter_set_impulse_and_reset_clear_state(torch, neo_gpu, method):
    C, B, P, Tb = 3, 16, 9, 8
    nb = Tb + 2
    ir, _, x = T.problem(C, B, P, nb)
    H = neo_gpu.uniform_partition(np.array(ir), B, dtype=np.float64)
    want, _ = run(torch, neo_gpu, C, B, P, method, H, x, Tb)
    assert T.peak_err(want, T.truth(C, B, P, method, nb)) <= T.TOL
    conv = neo_gpu.UpolsConvolver64(C, B, P, method=method)
    conv.filter(H)
    conv.set_batch(Tb)
    outs = []
    for clear in (lambda: None, conv.reset, lambda: conv.filter(H), lambda: conv.set_impulse(np.array(ir), normalize=False)):
        clear()
        assert conv.batch_info()["blocks_per_pass"] == Tb  # the setup calls leave batching as it is
        t = torch.from_numpy(np.array(x)).cuda()
        conv.process(t)
        outs.append(t.cpu().numpy())
    conv.close()
    for i, y in enumerate(outs):
        same_bits(y, want, f"run {i} on one handle")


def test_batch_info_is_the_plan(neo_gpu):
    for C, B, P, method, split, blocks in ((3, 128, 70, "upols", 0, True), (3, 128, 70, "upola", 12, 8), (1, 512, 188, "upola", 0, 16),
                                           (2, 16, 1, "upols", 0, True)):
        conv = neo_gpu.UpolsConvolver64(C, B, P, method=method, split_workgroups=split)
        state = conv.info()
        assert conv.batch_info() == {"blocks_per_pass": 1, "splits": 1, "extra_bytes": 0}
        conv.set_batch(blocks)
        plan = neo_gpu.upols64_batch_plan(C, B, P, method, split, int(blocks))
        assert conv.batch_info() == {k: plan[k] for k in ("blocks_per_pass", "splits", "extra_bytes")}
        assert plan["blocks_per_pass"] in (8, 16) and conv.info() == state
        conv.set_batch(False)
        assert conv.batch_info() == {"blocks_per_pass": 1, "splits": 1, "extra_bytes": 0}
        conv.close()


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_dense_convolve_f64_batched_with_a_ragged_tail(neo_gpu, method):
    rng = np.random.default_rng(12)
    C, B = 2, 64
    N, L = B * (2 * 16 + 5) + 29, B * 4 + 7  # N > 2 T B for either T
    x, ir = rng.standard_normal((C, N)), rng.standard_normal((C, L))
    y = neo_gpu.dense_convolve(x, ir, B, method=method, dtype=np.float64, batch=True)
    assert y.dtype == np.float64 and y.shape == (C, N)
    err = T.peak_err(y, T.whole(x, T.normalize(ir)))
    print(f"dense_convolve batch=True {method}: {err:.3g}")
    assert err <= T.TOL
    assert T.peak_err(y, neo_gpu.dense_convolve(x, ir, B, method=method, dtype=np.float64)) <= 2 * T.TOL
