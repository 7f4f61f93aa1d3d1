"""Batched passes of the matrix convolver on the device (neo_hip_matrix_set_batch,
MatrixConvolver.set_batch, k_matrix_batch_mac). Reference and bar are those of
tests/test_matrix_gpu.py: per output the float64 sum, in ascending input order, of
oracle.dense_convolve over its routes; conftest.peak_err <= 1e-5 (the project's bar; the GPU paths
measure 3-5e-7 against the oracle, so the reference alone leaves room)."""
import numpy as np
import pytest

from conftest import peak_err
from test_io_contract_gpu import IN_FILL, OUT_FILL, _arena, assert_same_bits, check_regions
from test_matrix_gpu import ROUTE_LISTS, ROUTE_SHAPE, problem, reference

pytestmark = pytest.mark.gpu
TOL = 1e-5

# (I, O, B, P, blocks): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (1, 1, 16, 3, 95),     # P < T: every chunk ends early; 16 live bins of 64 lanes; passes 32 32 16 8 4 2 + 1
    (2, 2, 32, 37, 120),   # the ring of 68 rows wraps; P no multiple of T; window reload at the input change
    (3, 5, 128, 9, 70),    # I != O; three short runs per output
    (4, 3, 512, 70, 67),   # two bin chunks per row; automatic splits and a cut inside an input
    (2, 2, 1024, 20, 40),  # four bin chunks
    (1, 2, 4096, 3, 34),   # sixteen bin chunks
]


def inside_cut_target(neo, I, O, B, P, routes=None):
    """A split_workgroups whose plan has more than one split and a run that starts inside an input."""
    for S in range(2, 12):
        target = S * O * max(1, B // 256)
        p = neo.matrix_batch_plan(I, O, B, P, routes=routes, split_workgroups=target)
        if p["splits"] > 1 and any(a for o in p["outputs"] for s in o["splits"] for _, a, _ in s):
            return target
    raise AssertionError("no forced target cuts inside an input")


def make(neo, I, O, B, P, parts, routes, method, batch=True, split=0):
    conv = neo.MatrixConvolver(I, O, B, P, method=method)
    conv.filter(parts, routes)
    if batch:
        conv.set_batch(True, split)
    return conv


def run(neo, I, O, B, P, parts, routes, x, method, batch=True, split=0):
    conv = make(neo, I, O, B, P, parts, routes, method, batch, split)
    y = conv.process(x)
    info = conv.batch_info()
    info["fdl_bytes"] = conv.info()["fdl_bytes"]
    conv.close()
    return y, info


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("I,O,B,P,nb", SHAPES)
def test_shapes_automatic_and_forced_splits(neo_gpu, oracle, I, O, B, P, nb, method):
    neo = neo_gpu
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    forced = inside_cut_target(neo, I, O, B, P)
    for split in (0, forced):
        y, info = run(neo, I, O, B, P, parts, rt, x, method, True, split)
        err = peak_err(y, ref)
        print(f"{(I, O, B, P, nb)} {method} split_workgroups {split}: Sb {info['splits']} err {err:.3g}")
        assert info["blocks_per_pass"] == 32 and info["ring_rows"] == P + 31
        assert info["fdl_bytes"] == I * (P + 31) * B * 8
        assert info["splits"] == neo.matrix_batch_plan(I, O, B, P, split_workgroups=split)["splits"]
        if split:
            assert info["splits"] > 1
        assert err <= TOL, (split, err)


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("name", list(ROUTE_LISTS))
def test_route_lists(neo_gpu, oracle, name, method):
    neo = neo_gpu
    I, O, B, P, _ = ROUTE_SHAPE
    nb = 70
    routes = ROUTE_LISTS[name]
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb, routes)
    ref = reference(oracle, I, O, B, P, nb, method, routes)
    perm = [int(k) for k in np.random.default_rng(3).permutation(len(routes))]
    for split in (0, inside_cut_target(neo, I, O, B, P, routes)):
        y, info = run(neo, I, O, B, P, parts, routes, x, method, True, split)
        err = peak_err(y, ref)
        print(f"{name} {method} split_workgroups {split}: Sb {info['splits']} err {err:.3g}")
        assert err <= TOL, (split, err)
        if name == "no_output_1":
            assert not y[1].any(), "an output without a route must be exactly zero"
        ys, _ = run(neo, I, O, B, P, parts[perm], [routes[k] for k in perm], x, method, True, split)
        assert_same_bits(ys, y, f"{name} shuffled")
        y2, _ = run(neo, I, O, B, P, parts, routes, x, method, True, split)
        assert_same_bits(y2, y, f"{name}: two fresh handles")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_batched_and_single_passes_mix(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 9, 70
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    whole, _ = run(neo, I, O, B, P, parts, rt, x, method, True)
    assert peak_err(whole, ref) <= TOL
    single, _ = run(neo, I, O, B, P, parts, rt, x, method, False)
    # on and off again before any block: the bits of a handle that was never touched
    conv = make(neo, I, O, B, P, parts, rt, method, True)
    conv.set_batch(False)
    assert conv.batch_info() == {"blocks_per_pass": 1, "splits": 0, "ring_rows": P + 31}
    assert_same_bits(conv.process(x), single, "set_batch(True) then set_batch(False)")
    conv.close()
    # calls of 5, 40, 1 and 24 blocks, batching toggled between them: one stream, never reset
    conv = make(neo, I, O, B, P, parts, rt, method, False)
    assert conv.batch_info()["ring_rows"] == P
    out, t = [], 0
    for k, (n, on) in enumerate([(5, False), (40, True), (1, False), (24, True)]):
        conv.set_batch(on, 0 if k < 3 else 2 * O)
        out.append(conv.process(x[:, t * B:(t + n) * B]))
        t += n
    assert t == nb
    conv.close()
    mixed = np.concatenate(out, axis=1)
    err = peak_err(mixed, ref)
    print(f"{method}: one call {peak_err(whole, ref):.3g}, mixed calls {err:.3g}")
    assert err <= TOL
    assert_same_bits(mixed[:, :5 * B], single[:, :5 * B], "the single steps before the first batched pass")
    # refused settings leave the state untouched
    conv = make(neo, I, O, B, P, parts, rt, method, True, 3 * O)
    before = conv.batch_info()
    for bad in ((2, 0), (-1, 0), (1, -1)):
        with pytest.raises(neo._native.NeoHipError):
            neo._native.check(neo._native.load().neo_hip_matrix_set_batch(conv._h, *bad))
    assert conv.batch_info() == before and before["splits"] == 3
    assert peak_err(conv.process(x), ref) <= TOL
    conv.close()


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_nan_leaves_with_the_filters_reach(neo_gpu, oracle, method):
    """A block of NaN in one input: the batched pass poisons what single steps poison and nothing
    else. Rows older than the filter reaches stay in the ring of P + 31 rows (and P = 5 < T, so most
    steps of a chunk are past the run's end): they must be skipped, not multiplied by zero."""
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 5, 40
    routes = [(0, 0), (1, 0), (1, 1)]  # lower-triangular: input 1 feeds output 1 alone
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb, tuple(routes))
    clean, _ = run(neo, I, O, B, P, parts, routes, x, method, True)
    for bad_in, fed, free in ((0, (0, 1), ()), (1, (1,), (0,))):
        bad = np.array(x)
        bad[bad_in, 2 * B:3 * B] = np.nan
        y, _ = run(neo, I, O, B, P, parts, routes, bad, method, True)
        want, _ = run(neo, I, O, B, P, parts, routes, bad, method, False)
        for o in fed:
            assert np.array_equal(np.isnan(y[o]), np.isnan(want[o])), (bad_in, o)
            assert np.isnan(y[o, 2 * B:3 * B]).all()
            # finite again once the block has left the filter (P blocks) and the overlap (one more)
            assert np.isfinite(y[o, (2 + P + 1) * B:]).all(), (bad_in, o)
            ok = np.isfinite(want[o])
            scale = np.abs(want[o][ok]).max()
            assert np.abs(y[o][ok].astype(np.float64) - want[o][ok]).max() <= TOL * scale
        for o in free:
            assert_same_bits(y[o:o + 1], clean[o:o + 1], f"output {o} beside a NaN block of input {bad_in}")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_io_contract(neo_gpu, oracle, method):
    import torch

    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 9, 70
    n = nb * B
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    split = inside_cut_target(neo, I, O, B, P)
    want, _ = run(neo, I, O, B, P, parts, rt, x, method, True, split)
    assert peak_err(want, ref) <= TOL
    ld_in, ld_out = n + 36, n + 4
    ia = _arena(torch, I, ld_in, IN_FILL)
    ia.view(torch.float32)[1:I + 1, :n] = torch.from_numpy(np.array(x)).cuda()
    oa = _arena(torch, O, ld_out, OUT_FILL)
    before = ia.cpu().numpy()
    conv = make(neo, I, O, B, P, parts, rt, method, True, split)
    ip, op = ia.data_ptr() + 4 * ld_in, oa.data_ptr() + 4 * ld_out
    conv.process_device(ip, ld_in, op, ld_out, nb)
    torch.cuda.synchronize()
    assert np.array_equal(ia.cpu().numpy(), before), "the call changed its input"
    assert_same_bits(check_regions(oa.cpu().numpy(), O, n, OUT_FILL), want, "separate strided arenas")

    # refused calls leave a batched stream as it was: the next blocks continue it
    conv.reset()
    oa.fill_(OUT_FILL)
    first = 37  # passes of 32, 4 and a single step, then 33 more blocks
    half = first * B
    conv.process_device(ip, ld_in, op, ld_out, first)
    for bad in ((ip + 4 * half, ld_in + 2, op + 4 * half, ld_out, nb - first),      # ld_in no multiple of 4
                (ip + 4 * half, ld_in, op + 4 * half, ld_out - 2, nb - first),      # ld_out no multiple of 4
                (ip + 4 * half + 4, ld_in, op + 4 * half, ld_out, nb - first),      # misaligned input
                (ip + 4 * half, ld_in, op + 4 * half + 8, ld_out, nb - first),      # misaligned output
                (ip + 4 * half, B * (nb - first) - 4, op + 4 * half, ld_out, nb - first),  # ld_in too small
                (ip + 4 * half, ld_in, op + 4 * half, B, 2)):                       # ld_out too small
        with pytest.raises(neo._native.NeoHipError):
            conv.process_device(*bad)
    conv.process_device(ip + 4 * half, ld_in, op + 4 * half, ld_out, nb - first)
    torch.cuda.synchronize()
    assert np.array_equal(ia.cpu().numpy(), before), "the calls changed their input"
    got = check_regions(oa.cpu().numpy(), O, n, OUT_FILL)
    assert peak_err(got, ref) <= TOL  # (passes of other sizes than one call of 70: another summation order)
    assert_same_bits(got[:, :32 * B], want[:, :32 * B], "the first pass of 32 blocks")
    conv.close()


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_in_place(neo_gpu, oracle, method):
    import torch

    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 37, 120
    n = nb * B
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    for split in (0, inside_cut_target(neo, I, O, B, P)):
        want, _ = run(neo, I, O, B, P, parts, rt, x, method, True, split)
        ld = n + 4
        a = _arena(torch, I, ld, OUT_FILL)
        a.view(torch.float32)[1:I + 1, :n] = torch.from_numpy(np.array(x)).cuda()
        conv = make(neo, I, O, B, P, parts, rt, method, True, split)
        conv.process_device(a.data_ptr() + 4 * ld, ld, a.data_ptr() + 4 * ld, ld, nb)
        torch.cuda.synchronize()
        conv.close()
        assert_same_bits(check_regions(a.cpu().numpy(), O, n, OUT_FILL), want, "in == out")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_reset_and_second_filter_restart_cleanly(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 37, 120
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    split = inside_cut_target(neo, I, O, B, P)
    fresh, _ = run(neo, I, O, B, P, parts, rt, x, method, True, split)
    conv = make(neo, I, O, B, P, parts, rt, method, True, split)
    conv.process(x[:, :45 * B])
    conv.reset()
    assert_same_bits(conv.process(x), fresh, "after reset")
    conv.process(x[:, :39 * B])
    # another route list in mid-stream, then the first one again: batching stays on, the plan follows
    conv.filter(parts[:1], [(1, 0)])
    assert conv.batch_info()["blocks_per_pass"] == 32 and conv.batch_info()["ring_rows"] == P + 31
    y = conv.process(x[:, :35 * B])
    assert not y[0].any() and y[1].any()
    assert conv.info()["routes"] == 1
    conv.filter(parts, rt)
    assert_same_bits(conv.process(x), fresh, "after a second set_filter")
    conv.close()


def test_torch_tensors_and_one_shot(neo_gpu, oracle):
    import torch

    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 9, 70
    rt, x, ir, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, "upols")
    want, _ = run(neo, I, O, B, P, parts, rt, x, "upols", True)
    conv = neo.MatrixConvolver(I, O, B, P)
    conv.filter(torch.from_numpy(np.array(parts)).cuda().reshape(O, I, P, B + 1))
    conv.set_batch(True)
    y = conv.process(torch.from_numpy(np.array(x)).cuda())
    assert y.is_cuda and tuple(y.shape) == (O, nb * B)
    assert_same_bits(y.cpu().numpy(), want, "device tensors")
    conv.close()
    # the one-shot, host arrays and device tensors
    dense_ir = ir.reshape(O, I, -1)
    off = neo.matrix_convolve(x, dense_ir, B)
    on = neo.matrix_convolve(x, dense_ir, B, batch=True)
    assert peak_err(on, ref) <= TOL and peak_err(on, off) <= TOL
    xt, irt = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(dense_ir)).cuda()
    ont = neo.matrix_convolve(xt, irt, B, batch=True)
    assert ont.is_cuda and tuple(ont.shape) == (O, nb * B)
    assert peak_err(ont.cpu().numpy(), ref) <= TOL
    assert peak_err(ont.cpu().numpy(), neo.matrix_convolve(xt, irt, B).cpu().numpy()) <= TOL
