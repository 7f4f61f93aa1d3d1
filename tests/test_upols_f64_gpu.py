"""The double-precision UPOLS / UPOLA convolvers on the device (neo.UpolsConvolver64, the float64
paths of uniform_partition / normalize_impulse / dense_convolve and the single-channel classes)
against float64 numpy truth at the project's f64 bar, 1e-12 of the peak (tests/upols_f64_truth.py;
tests/test_upols_f64.py shows that truth's two statements agree within 1e-13), their bits across
equal calls, and the I/O contract of neo_hip.h by the arena method of DESIGN.md section 3 in float64."""
import numpy as np
import pytest

import upols_f64_truth as T

pytestmark = pytest.mark.gpu

IN_FILL = 0x7FF8BEEF0BADF00D   # a quiet NaN with a payload: a padding or guard word that reaches a sum poisons it
OUT_FILL = 0x7FF9CAFE0D15EA5E  # another one, so a copy of input padding into output padding shows too
PAD_IN, PAD_OUT = 36, 4        # ld_in = n + 36, ld_out = n + 4: even, and they differ


@pytest.fixture(scope="module")
def torch(neo_gpu):
    import torch as t

    return t


def run_device(torch, neo, C, B, P, method, H, x, split=0, per_call=None):
    """A fresh handle, the filter H, x [C][n] through it on the device in calls of per_call blocks
    (None: one call); the output and the handle's info."""
    conv = neo.UpolsConvolver64(C, B, P, method=method, split_workgroups=split)
    conv.filter(H)
    t = torch.from_numpy(np.array(x)).cuda()
    if per_call is None:
        conv.process(t)
    else:
        n = x.shape[1]
        step = per_call * B
        for o in range(0, n, step):
            k = min(step, n - o)
            conv.process_device(t.data_ptr() + 8 * o, n, t.data_ptr() + 8 * o, n, n=k)
    torch.cuda.synchronize()
    info = conv.info()
    conv.close()
    return t.cpu().numpy(), info


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    bad = np.ascontiguousarray(got).view(np.int64) != np.ascontiguousarray(want).view(np.int64)
    if bad.any():
        c, j = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at channel {c}, column {j}: "
                             f"{got[c, j]!r} != {want[c, j]!r}")


# ------------------------------------------------------------------ values against truth
@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P", T.VALUE_SHAPES)
def test_values_against_truth(torch, neo_gpu, C, B, P, method):
    """P + 5 blocks (the ring of P rows wraps), automatic splits and four splits asked for (P = 9:
    rows 3; P = 70: rows 18, 18, 18, 16), against both statements of the truth at 1e-12."""
    ir, H, x = T.problem(C, B, P)
    for split in (0, T.forced_split(C)):
        y, info = run_device(torch, neo_gpu, C, B, P, method, H, x, split)
        S, rows = T.float_rule(C, P, split)
        assert (info["splits"], info["rows"]) == (S, rows)
        assert info["state_bytes"] == 32 * C * P * B + 8 * C * B + 16 * C * S * B
        for statement in ("blockwise", "whole"):
            err = T.peak_err(y, T.truth(C, B, P, method, statement=statement))
            print(f"{C} x {B} x {P} {method} split {split} (S {S}, rows {rows}) vs {statement}: {err:.3g}")
            assert err <= T.TOL, (split, statement, err)


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_values_block_4096(torch, neo_gpu, method):
    C, B, P = T.BIG_SHAPE
    ir, H, x = T.problem(C, B, P, T.BIG_BLOCKS)
    y, _ = run_device(torch, neo_gpu, C, B, P, method, H, x)
    for statement in ("blockwise", "whole"):
        err = T.peak_err(y, T.truth(C, B, P, method, T.BIG_BLOCKS, statement=statement))
        print(f"{C} x {B} x {P} {method} vs {statement}: {err:.3g}")
        assert err <= T.TOL, (statement, err)


@pytest.mark.parametrize("B", [128, 256, 512, 1024])
@pytest.mark.parametrize("kind", ["upols_convolver", "upola_convolver", "split_upols_convolver", "split_upola_convolver"])
def test_identity_filter_returns_the_input(neo_gpu, kind, B):
    """The reference's convolver test (uniform_partitioned_convolver_test.cpp): an identity filter of
    3 partitions, 20 blocks, output equal to input within 1e-12 absolute."""
    filt = np.zeros((3, B + 1), dtype=np.complex128)
    filt[0] = 1.0
    conv = getattr(neo_gpu, kind)(dtype=np.float64)
    conv.filter(filt)
    rng = np.random.default_rng(77 + B)
    for _ in range(20):
        x = rng.uniform(-1.0, 1.0, B)
        y = x.copy()
        assert conv(y) is y
        assert np.abs(y - x).max() <= 1e-12


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_equal_calls_give_equal_bits(torch, neo_gpu, method):
    C, B, P = 3, 128, 70
    ir, H, x = T.problem(C, B, P)
    a, _ = run_device(torch, neo_gpu, C, B, P, method, H, x)
    b, _ = run_device(torch, neo_gpu, C, B, P, method, H, x)
    same_bits(b, a, "two fresh handles, the same calls")
    c, _ = run_device(torch, neo_gpu, C, B, P, method, H, x, per_call=1)
    same_bits(c, a, "k calls of one block against one call of k blocks")
    d, _ = run_device(torch, neo_gpu, C, B, P, method, H, x, per_call=7)
    same_bits(d, a, "calls of 7 blocks")
    conv = neo_gpu.UpolsConvolver64(C, B, P, method=method)
    conv.filter(H)
    h = np.array(x)
    assert conv.process(h) is h
    conv.close()
    same_bits(h, a, "host buffers against device buffers")


# ------------------------------------------------------------------ where it reads and writes
def check_regions(out_after, C, n, out_fill, in_before=None, in_after=None):
    """Host copies of the arenas as int64 [C + 2][ld] (bit patterns, so NaNs compare): (a) the input
    arena equals its copy from before the call bit for bit, (b) every word of the output arena
    outside columns [0, n) of rows 1..C still holds the sentinel; returns (c) the output payload
    [C][n] as float64. (tests/test_io_contract_gpu.py's check_regions takes 32-bit words only.)"""
    for a in (out_after, in_before, in_after):
        assert a is None or (a.dtype == np.int64 and a.ndim == 2 and a.shape[0] == C + 2 and a.shape[1] >= n)
    if in_before is not None:
        bad = in_after != in_before
        assert not bad.any(), f"the call changed its input at (row, column) {tuple(int(v) for v in np.argwhere(bad)[0])}"
    bad = out_after != np.int64(out_fill)
    bad[1:C + 1, :n] = False
    assert not bad.any(), f"the call wrote outside its output at (row, column) {tuple(int(v) for v in np.argwhere(bad)[0])}"
    return np.ascontiguousarray(out_after[1:C + 1, :n]).view(np.float64)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_io_contract_in_padded_arenas(torch, neo_gpu, method, host):
    """Arenas of C + 2 rows of ld words holding a NaN-payload sentinel, the channels in rows 1..C.
    B: from an input arena of stride n + 36 into an output arena of stride n + 4; B': in place
    inside one arena of stride n + 4. The input arena stays as it was, every word outside the
    payload still holds the sentinel, and the payloads equal the contiguous run bit for bit."""
    C, B, P = 3, 128, 9
    ir, H, x = T.problem(C, B, P)
    n = x.shape[1]
    A, _ = run_device(torch, neo_gpu, C, B, P, method, H, x)
    assert T.peak_err(A, T.truth(C, B, P, method)) <= T.TOL

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
        conv.process_device(ip, li, op, lo, n=n, is_device=not host)
        torch.cuda.synchronize()
        conv.close()

    ia, ip = arena(n + PAD_IN, IN_FILL, x)
    oa, op = arena(n + PAD_OUT, OUT_FILL)
    before = read(ia)
    go(ip, n + PAD_IN, op, n + PAD_OUT)
    same_bits(check_regions(read(oa), C, n, OUT_FILL, before, read(ia)), A, "B (separate padded buffers)")
    pa, pp = arena(n + PAD_OUT, IN_FILL, x)
    go(pp, n + PAD_OUT, pp, n + PAD_OUT)
    same_bits(check_regions(read(pa), C, n, IN_FILL), A, "B' (in place, padded)")


def test_refusals_do_not_advance_state(torch, neo_gpu):
    """Odd or too-small strides, a misaligned base and n that is no multiple of B are refused; the
    next valid call gives the untouched sequence's output."""
    C, B, P = 3, 128, 9
    ir, H, x = T.problem(C, B, P)
    n = x.shape[1]
    want, _ = run_device(torch, neo_gpu, C, B, P, "upols", H, x)
    conv = neo_gpu.UpolsConvolver64(C, B, P)
    conv.filter(H)
    t = torch.from_numpy(np.array(x)).cuda()
    p = t.data_ptr()
    half = (n // B // 2) * B
    conv.process_device(p, n, p, n, n=half)
    for li, lo, k, ptr in ((n + 1, n, B, p), (n, n + 3, B, p), (B - 2, n, B, p), (n, B - 2, B, p), (n, n, B - 16, p),
                           (n, n, B + 2, p), (n, n, -B, p), (n, n, B, p + 8)):
        with pytest.raises(neo_gpu._native.NeoHipError) as e:
            conv.process_device(ptr + 8 * half, li, ptr + 8 * half, lo, n=k)
        assert e.value.code == neo_gpu._native.NEO_HIP_EINVAL
    h = np.zeros((C, B + 1))
    with pytest.raises(neo_gpu._native.NeoHipError):  # host buffers: the same contract
        conv.process_device(h.ctypes.data, B + 1, h.ctypes.data, B + 1, n=B, is_device=False)
    conv.process_device(p + 8 * half, n, p + 8 * half, n, n=n - half)
    torch.cuda.synchronize()
    conv.close()
    same_bits(t.cpu().numpy(), want, "after the refused calls")


# ------------------------------------------------------------------ setup calls
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_set_filter_and_reset_clear_state(torch, neo_gpu, method):
    C, B, P = 3, 16, 9
    ir, H, x = T.problem(C, B, P)
    want, _ = run_device(torch, neo_gpu, C, B, P, method, H, x)
    conv = neo_gpu.UpolsConvolver64(C, B, P, method=method)
    conv.filter(H)
    outs = []
    for clear in (lambda: None, conv.reset, lambda: conv.filter(H), lambda: conv.filter(torch.from_numpy(np.array(H)).cuda())):
        clear()
        t = torch.from_numpy(np.array(x)).cuda()
        conv.process(t)
        outs.append(t.cpu().numpy())
    conv.close()
    for i, y in enumerate(outs):
        same_bits(y, want, f"run {i} on one handle")


def test_set_impulse_equals_the_three_calls(torch, neo_gpu):
    """set_impulse = normalize_impulse + uniform_partition + filter, bit for bit; host and device input."""
    C, B, P = 3, 128, 9
    ir, _, x = T.problem(C, B, P)
    n_ir = neo_gpu.normalize_impulse(np.array(ir), dtype=np.float64)
    H = neo_gpu.uniform_partition(n_ir, B, dtype=np.float64)
    assert H.dtype == np.complex128 and H.shape == (C, P, B + 1)
    want, _ = run_device(torch, neo_gpu, C, B, P, "upols", H, x)
    assert T.peak_err(want, T.whole(x, T.normalize(ir))) <= T.TOL
    for src in (np.array(ir), torch.from_numpy(np.array(ir)).cuda()):
        conv = neo_gpu.UpolsConvolver64(C, B, P)
        conv.set_impulse(src, normalize=True)
        t = torch.from_numpy(np.array(x)).cuda()
        conv.process(t)
        conv.close()
        same_bits(t.cpu().numpy(), want, "set_impulse against normalize + partition + filter")
    assert np.array_equal(src.cpu().numpy(), ir)  # the caller's impulse stays as it was
    conv = neo_gpu.UpolsConvolver64(C, B, P + 1)
    with pytest.raises(neo_gpu._native.NeoHipError):
        conv.set_impulse(np.array(ir))
    conv.close()


@pytest.mark.parametrize("B,L,C", [(16, 13, 1), (16, 16 * 5, 3), (128, 128 * 9 - 3, 3), (512, 512 * 2 + 1, 2), (4096, 4096 * 2 - 5, 1)])
def test_uniform_partition_f64(torch, neo_gpu, B, L, C):
    ir = np.random.default_rng(B + L).standard_normal((C, L))
    want = T.partition(ir, B)
    got = neo_gpu.uniform_partition(ir, B, dtype=np.float64)
    assert got.dtype == np.complex128 and got.shape == want.shape
    assert T.peak_err(got, want) <= T.TOL
    assert not got[:, :, 0].imag.any() and not got[:, :, B].imag.any()
    dev = neo_gpu.uniform_partition(torch.from_numpy(ir).cuda(), B, dtype=np.float64)
    assert dev.dtype == torch.complex128 and np.array_equal(dev.cpu().numpy(), got)
    one = neo_gpu.uniform_partition(ir[0], B, dtype=np.float64)
    assert np.array_equal(one[0], got[0])
    assert neo_gpu.uniform_partition(ir.astype(np.float32), B).dtype == np.complex64  # the default is float32


def test_normalize_impulse_f64(torch, neo_gpu):
    rng = np.random.default_rng(5)
    one = rng.standard_normal(4099)
    got = neo_gpu.normalize_impulse(one.copy(), dtype=np.float64)
    assert got.dtype == np.float64 and T.peak_err(got, one / np.sqrt((one * one).sum())) <= T.TOL
    two = rng.standard_normal((3, 1031)) * np.array([[1.0], [3.0], [0.25]])
    want = T.normalize(two)
    assert abs((want[1] ** 2).sum() - 1.0) < 1e-12  # min over channels: the loudest channel ends at unit energy
    got = neo_gpu.normalize_impulse(two.copy(), dtype=np.float64)
    assert T.peak_err(got, want) <= T.TOL
    dev = torch.from_numpy(two.copy()).cuda()
    assert neo_gpu.normalize_impulse(dev, dtype=np.float64) is dev
    assert np.array_equal(dev.cpu().numpy(), got)  # a fixed summation order: equal bits
    zero = np.zeros((2, 64))
    assert not neo_gpu.normalize_impulse(zero, dtype=np.float64).any()
    with pytest.raises(TypeError):
        neo_gpu.normalize_impulse(two.astype(np.float32), dtype=np.float64)


# ------------------------------------------------------------------ against the float32 handle, dense_convolve
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_float32_handle_is_within_its_bar_of_the_double_one(torch, neo_gpu, method):
    C, B, P = 3, 128, 70
    ir, H, x = T.problem(C, B, P)
    y64, _ = run_device(torch, neo_gpu, C, B, P, method, H, x)
    conv = neo_gpu.UpolsConvolver(C, B, P, method=method)
    conv.filter(H.astype(np.complex64))
    y32 = x.astype(np.float32)
    conv.process(y32)
    conv.close()
    err = T.peak_err(y32.astype(np.float64), y64)
    print(f"float32 handle vs double handle: {err:.3g}")
    assert err <= 1e-5


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_dense_convolve_f64_with_a_ragged_tail(neo_gpu, method):
    rng = np.random.default_rng(11)
    C, B, N, L = 2, 64, 64 * 11 + 29, 64 * 4 + 7
    x, ir = rng.standard_normal((C, N)), rng.standard_normal((C, L))
    y = neo_gpu.dense_convolve(x, ir, B, method=method, dtype=np.float64)
    assert y.dtype == np.float64 and y.shape == (C, N)
    assert T.peak_err(y, T.whole(x, T.normalize(ir))) <= T.TOL
    y32 = neo_gpu.dense_convolve(x.astype(np.float32), ir.astype(np.float32), B, method=method)
    assert y32.dtype == np.float32 and T.peak_err(y32.astype(np.float64), y) <= 1e-5
