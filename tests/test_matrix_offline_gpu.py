"""Offline windows of the matrix convolver on the device (neo_hip_matrix_set_offline,
MatrixConvolver.set_offline, k_matrix_off_fwd / k_matrix_off_mac). Reference and bar are those of
tests/test_matrix_gpu.py: per output the float64 sum, in ascending input order, of
oracle.dense_convolve over its routes; conftest.peak_err <= 1e-5 (the project's bar; the dense
offline windows are held to it in tests/test_offline_gpu.py and the GPU paths measure 3-5e-7
against the oracle, so the reference alone leaves room)."""
import numpy as np
import pytest

from conftest import peak_err
from test_io_contract_gpu import IN_FILL, OUT_FILL, _arena, assert_same_bits, check_regions
from test_matrix_gpu import ROUTE_LISTS, ROUTE_SHAPE, problem, reference

pytestmark = pytest.mark.gpu
TOL = 1e-5

# (I, O, B, P, blocks per call, calls): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (1, 1, 16, 3, 300, 1),    # one segment, nearly all padding; the only unit is the bin-0 unit; 256 blocks, then 44 by other passes
    (2, 2, 32, 130, 420, 2),  # two segments, the second with two partitions; passes of 256 and 128 and a rest; call 2 wraps the ring of 513 rows
    (3, 5, 128, 260, 384, 1),  # I != O; three segments; exactly 256 + 128
    (2, 3, 512, 129, 256, 1),  # 32 units per row; one two-window pass
    (1, 2, 4096, 3, 128, 1),  # 256 units; one one-window pass
]


def make(neo, I, O, B, P, parts, routes, method, offline=True, wpp=0, batch=False):
    conv = neo.MatrixConvolver(I, O, B, P, method=method)
    conv.filter(parts, routes)
    if batch:
        conv.set_batch(True)
    if offline:
        conv.set_offline(True, wpp)
    return conv


def run(neo, I, O, B, P, parts, routes, x, method, offline=True, wpp=0, batch=False, calls=1):
    conv = make(neo, I, O, B, P, parts, routes, method, offline, wpp, batch)
    n = x.shape[1] // calls
    y = np.concatenate([conv.process(x[:, k * n:(k + 1) * n]) for k in range(calls)], axis=1)
    info = conv.offline_info()
    info["desc"] = conv.info()
    conv.close()
    return y, info


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("I,O,B,P,nb,calls", SHAPES)
def test_shapes_windows_per_pass_and_the_rest(neo_gpu, oracle, I, O, B, P, nb, calls, method):
    neo = neo_gpu
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb * calls)
    ref = reference(oracle, I, O, B, P, nb * calls, method)
    for wpp in (0, 1, 2):
        plan = neo.matrix_offline_plan(I, O, B, P, windows=wpp)
        for batch in (True, False):
            y, info = run(neo, I, O, B, P, parts, rt, x, method, True, wpp, batch, calls)
            err = peak_err(y, ref)
            print(f"{(I, O, B, P, nb, calls)} {method} windows_per_pass {wpp} batch {batch}: err {err:.3g}")
            assert info["blocks_per_pass"] == plan["blocks_per_pass"] == (128 if wpp == 1 else 256)
            assert info["segments"] == plan["segments"] == -(-P // 128)
            assert info["ring_rows"] == plan["min_ring_rows"] == 128 * (plan["segments"] + 2) + 1
            assert info["spectra_bytes"] == plan["hf_bytes"] == I * O * plan["segments"] * 256 * B * 8
            assert info["desc"]["fdl_bytes"] == I * info["ring_rows"] * B * 8
            assert info["desc"]["offline_bytes"] >= plan["hf_bytes"] + I * (plan["segments"] + 1) * 256 * B * 8
            assert err <= TOL, (wpp, batch, err)


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("name", list(ROUTE_LISTS))
def test_route_lists(neo_gpu, oracle, name, method):
    neo = neo_gpu
    I, O, B, _, _ = ROUTE_SHAPE
    P, nb = 130, 300
    routes = ROUTE_LISTS[name]
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb, routes)
    ref = reference(oracle, I, O, B, P, nb, method, routes)
    perm = [int(k) for k in np.random.default_rng(3).permutation(len(routes))]
    y, _ = run(neo, I, O, B, P, parts, routes, x, method)
    err = peak_err(y, ref)
    print(f"{name} {method}: err {err:.3g}")
    assert err <= TOL, err
    if name == "no_output_1":
        assert not y[1].any(), "an output without a route must be exactly zero"
    ys, _ = run(neo, I, O, B, P, parts[perm], [routes[k] for k in perm], x, method)
    assert_same_bits(ys, y, f"{name} shuffled")
    y2, _ = run(neo, I, O, B, P, parts, routes, x, method)
    assert_same_bits(y2, y, f"{name}: two fresh handles")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_all_kinds_of_pass_mix(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 130, 446
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    single, _ = run(neo, I, O, B, P, parts, rt, x, method, False)
    # on and off again before any block: the bits of a handle that was never touched
    conv = make(neo, I, O, B, P, parts, rt, method, True)
    conv.set_offline(False)
    assert conv.offline_info() == {"blocks_per_pass": 0, "segments": 2, "ring_rows": 513, "spectra_bytes": 0}
    assert_same_bits(conv.process(x), single, "set_offline(True) then set_offline(False)")
    conv.close()
    # calls of 5, 300, 1 and 140 blocks, offline and batching toggled between them: one stream
    conv = make(neo, I, O, B, P, parts, rt, method, False)
    assert conv.offline_info()["ring_rows"] == P
    out, t = [], 0
    for n, off, wpp, batch in [(5, False, 0, False), (300, True, 0, True), (1, False, 0, False), (140, True, 1, False)]:
        conv.set_batch(batch)
        conv.set_offline(off, wpp)
        out.append(conv.process(x[:, t * B:(t + n) * B]))
        t += n
    assert t == nb
    conv.close()
    mixed = np.concatenate(out, axis=1)
    err = peak_err(mixed, ref)
    print(f"{method}: mixed calls {err:.3g}")
    assert err <= TOL
    assert_same_bits(mixed[:, :5 * B], single[:, :5 * B], "the single steps before the first offline pass")
    # refused settings leave the state untouched
    conv = make(neo, I, O, B, P, parts, rt, method, True, 1)
    before = conv.offline_info()
    for bad in ((2, 0), (-1, 0), (1, -1), (1, 3), (0, 3)):
        with pytest.raises(neo._native.NeoHipError):
            neo._native.check(neo._native.load().neo_hip_matrix_set_offline(conv._h, *bad))
    assert conv.offline_info() == before and before["blocks_per_pass"] == 128
    assert peak_err(conv.process(x), ref) <= TOL
    conv.close()


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_nan_reaches_the_passes_whose_pairs_hold_it(neo_gpu, oracle, method):
    """A block of NaN in one input (neo_hip.h, "Inf / NaN"): the blocks of the passes whose pairs
    hold it may be NaN on the outputs routed from that input, and nothing else is. Passes at blocks
    0, 256, 512 and 768 (two windows each), two segments: block 300 is in the pass at 256 and in the
    pairs of the first window of the pass at 512 (512 - 256 <= 300): both windows at 256 and the
    window at 512 are all NaN; the pass at 768 reads back to 512 and is clean. Overlap-add carries
    the last tail of the pass before into its first block: one block more."""
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 130, 1024
    routes = [(0, 0), (1, 0), (1, 1)]  # lower-triangular: input 1 feeds output 1 alone
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb, tuple(routes))
    clean, _ = run(neo, I, O, B, P, parts, routes, x, method)
    at, first_clean = 300, 768 + (1 if method == "upola" else 0)
    for bad_in, fed, free in ((0, (0, 1), ()), (1, (1,), (0,))):
        bad = np.array(x)
        bad[bad_in, at * B:(at + 1) * B] = np.nan
        y, _ = run(neo, I, O, B, P, parts, routes, bad, method)
        want, _ = run(neo, I, O, B, P, parts, routes, bad, method, False)
        for o in fed:
            nan_y, nan_w = np.isnan(y[o]), np.isnan(want[o])
            assert nan_w[at * B:(at + 1) * B].all() and (nan_y | ~nan_w).all(), (bad_in, o)
            assert nan_y[256 * B:640 * B].all() and not nan_y[:256 * B].any(), (bad_in, o)
            assert np.isfinite(y[o, first_clean * B:]).all() and np.isfinite(want[o, first_clean * B:]).all(), (bad_in, o)
            scale = np.abs(want[o][np.isfinite(want[o])]).max()
            d = np.abs(y[o, first_clean * B:].astype(np.float64) - want[o, first_clean * B:]).max()
            print(f"{method} NaN in input {bad_in}, output {o}: {d / scale:.3g} of peak after the last poisoned pass")
            assert d <= TOL * scale
        for o in free:
            assert_same_bits(y[o:o + 1], clean[o:o + 1], f"output {o} beside a NaN block of input {bad_in}")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_io_contract(neo_gpu, oracle, method):
    import torch

    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 130, 420
    n = nb * B
    rt, x, _, _, parts = problem(oracle, I, O, B, P, 840)
    x = x[:, :n]
    ref = reference(oracle, I, O, B, P, 840, method)[:, :n]
    want, _ = run(neo, I, O, B, P, parts, rt, x, method, True, 0, True)
    assert peak_err(want, ref) <= TOL
    ld_in, ld_out = n + 36, n + 4
    ia = _arena(torch, I, ld_in, IN_FILL)
    ia.view(torch.float32)[1:I + 1, :n] = torch.from_numpy(np.array(x)).cuda()
    oa = _arena(torch, O, ld_out, OUT_FILL)
    before = ia.cpu().numpy()
    conv = make(neo, I, O, B, P, parts, rt, method, True, 0, True)
    ip, op = ia.data_ptr() + 4 * ld_in, oa.data_ptr() + 4 * ld_out
    conv.process_device(ip, ld_in, op, ld_out, nb)
    torch.cuda.synchronize()
    assert np.array_equal(ia.cpu().numpy(), before), "the call changed its input"
    assert_same_bits(check_regions(oa.cpu().numpy(), O, n, OUT_FILL), want, "separate strided arenas")

    # refused calls leave an offline stream as it was: the next blocks continue it
    conv.reset()
    oa.fill_(OUT_FILL)
    first = 256  # one two-window pass, then 164 more blocks
    half = first * B
    conv.process_device(ip, ld_in, op, ld_out, first)
    for bad in ((ip + 4 * half, ld_in + 2, op + 4 * half, ld_out, nb - first),      # ld_in no multiple of 4
                (ip + 4 * half, ld_in, op + 4 * half, ld_out - 2, nb - first),      # ld_out no multiple of 4
                (ip + 4 * half + 4, ld_in, op + 4 * half, ld_out, nb - first),      # misaligned input
                (ip + 4 * half, ld_in, op + 4 * half + 8, ld_out, nb - first),      # misaligned output
                (ip + 4 * half, B * (nb - first) - 4, op + 4 * half, ld_out, nb - first),  # ld_in too small
                (ip + 4 * half, ld_in, op + 4 * half, B, 130)):                     # ld_out too small
        with pytest.raises(neo._native.NeoHipError):
            conv.process_device(*bad)
    conv.process_device(ip + 4 * half, ld_in, op + 4 * half, ld_out, nb - first)
    torch.cuda.synchronize()
    assert np.array_equal(ia.cpu().numpy(), before), "the calls changed their input"
    # (256 + 128 + 32 + 4 either way: the same passes at the same blocks)
    assert_same_bits(check_regions(oa.cpu().numpy(), O, n, OUT_FILL), want, "two calls after refused ones")
    conv.close()

    # in == out inside one padded arena
    ld = n + 4
    a = _arena(torch, I, ld, OUT_FILL)
    a.view(torch.float32)[1:I + 1, :n] = torch.from_numpy(np.array(x)).cuda()
    conv = make(neo, I, O, B, P, parts, rt, method, True, 0, True)
    conv.process_device(a.data_ptr() + 4 * ld, ld, a.data_ptr() + 4 * ld, ld, nb)
    torch.cuda.synchronize()
    conv.close()
    assert_same_bits(check_regions(a.cpu().numpy(), O, n, OUT_FILL), want, "in == out")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_reset_and_second_filter_restart_cleanly(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 130, 420
    rt, x, _, _, parts = problem(oracle, I, O, B, P, 840)
    x = x[:, :nb * B]
    fresh, _ = run(neo, I, O, B, P, parts, rt, x, method, True, 0, True)
    conv = make(neo, I, O, B, P, parts, rt, method, True, 0, True)
    conv.process(x[:, :300 * B])
    conv.reset()
    assert_same_bits(conv.process(x), fresh, "after reset")
    conv.process(x[:, :139 * B])
    # another route list in mid-stream, then the first one again: offline stays on, the spectra follow
    conv.filter(parts[:1], [(1, 0)])
    info = conv.offline_info()
    assert info["blocks_per_pass"] == 256 and info["ring_rows"] == 513 and info["spectra_bytes"] == 0
    y = conv.process(x[:, :260 * B])
    assert not y[0].any() and y[1].any()
    assert conv.info()["routes"] == 1 and conv.offline_info()["spectra_bytes"] == 2 * 256 * B * 8
    conv.filter(parts, rt)
    assert_same_bits(conv.process(x), fresh, "after a second set_filter")
    assert conv.offline_info()["spectra_bytes"] == 4 * 2 * 256 * B * 8
    conv.close()


def test_torch_tensors_and_one_shot(neo_gpu, oracle):
    import torch

    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 260, 384
    rt, x, ir, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, "upols")
    want, _ = run(neo, I, O, B, P, parts, rt, x, "upols")
    conv = neo.MatrixConvolver(I, O, B, P)
    conv.filter(torch.from_numpy(np.array(parts)).cuda().reshape(O, I, P, B + 1))
    conv.set_offline(True)
    y = conv.process(torch.from_numpy(np.array(x)).cuda())
    assert y.is_cuda and tuple(y.shape) == (O, nb * B)
    assert_same_bits(y.cpu().numpy(), want, "device tensors")
    conv.close()
    # the one-shot, host arrays and device tensors
    dense_ir = ir.reshape(O, I, -1)
    off = neo.matrix_convolve(x, dense_ir, B)
    on = neo.matrix_convolve(x, dense_ir, B, offline=True)
    print(f"one shot: offline {peak_err(on, ref):.3g} against the reference, {peak_err(on, off):.3g} against offline=False")
    assert peak_err(on, ref) <= TOL and peak_err(on, off) <= TOL
    xt, irt = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(dense_ir)).cuda()
    ont = neo.matrix_convolve(xt, irt, B, offline=True)
    assert ont.is_cuda and tuple(ont.shape) == (O, nb * B)
    assert peak_err(ont.cpu().numpy(), ref) <= TOL
