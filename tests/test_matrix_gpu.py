"""The matrix convolver on the device (neo_hip_matrix_*, neo.MatrixConvolver). Reference: per output
the float64 sum, in ascending input order, of oracle.dense_convolve(x_in, parts_route, method) over
its routes -- the reference's upols_convolver / upola_convolver applied route by route. Bar: the
project's, conftest.peak_err <= 1e-5. Signals and impulse responses are oracle.noise, the impulse
responses normalized with oracle.normalize_impulse over all routes."""
import numpy as np
import pytest

from conftest import peak_err
from test_io_contract_gpu import IN_FILL, OUT_FILL, _arena, assert_same_bits, check_regions

pytestmark = pytest.mark.gpu
TOL = 1e-5

# (I, O, B, P, blocks): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    (1, 1, 16, 3, 20),     # degenerate; 32 row groups fold
    (2, 2, 32, 37, 80),    # true stereo; more blocks than ring rows: the ring wraps
    (3, 5, 128, 9, 40),    # I != O; tiles of 4 and 1
    (4, 3, 512, 70, 20),   # one row per 256 lanes; several splits
    (2, 2, 1024, 20, 12),  # two float4 per lane; out_tile clamps to 2
    (1, 2, 4096, 3, 8),    # out_tile clamps to 1
]

_cache = {}


def dense(I, O):
    return [(o, i) for o in range(O) for i in range(I)]


def problem(oracle, I, O, B, P, nb, routes=None):
    """x [I][nb B], the routes' partitions [nroutes][P][B+1] and the normalized impulse responses."""
    key = ("p", I, O, B, P, nb, None if routes is None else tuple(routes))
    if key not in _cache:
        rt = dense(I, O) if routes is None else list(routes)
        x = np.stack([oracle.noise(1000 + 7 * B + i, nb * B) for i in range(I)])
        ir = np.stack([oracle.noise(5000 + 11 * B + 64 * o + i, P * B) for o, i in rt])
        irn = oracle.normalize_impulse(ir)
        parts = oracle.uniform_partition(irn, B)
        for a in (x, ir, irn, parts):
            a.setflags(write=False)
        _cache[key] = (rt, x, ir, irn, parts)
    return _cache[key]


def reference(oracle, I, O, B, P, nb, method, routes=None):
    key = ("r", I, O, B, P, nb, method, None if routes is None else tuple(routes))
    if key not in _cache:
        rt, x, _, _, parts = problem(oracle, I, O, B, P, nb, routes)
        per_route = oracle.dense_convolve(x[[i for _, i in rt]], parts, method=method)
        ref = np.zeros((O, nb * B), np.float64)
        for o in range(O):
            for i in range(I):  # ascending input order
                if (o, i) in rt:
                    ref[o] += per_route[rt.index((o, i))]
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def inside_cut_split(neo, I, O, B, P, routes, out_tile):
    """A split_workgroups that gives S > 1 with a cut inside one input's partitions (None: one row)."""
    tiles = len(neo.matrix_plan(I, O, B, P, routes=routes, options={"out_tile": out_tile})["tiles"])
    for k in range(2, 12):
        p = neo.matrix_plan(I, O, B, P, routes=routes, options={"out_tile": out_tile, "split_workgroups": tiles * k})
        if p["splits"] > 1 and any(c % P for t in p["tiles"] for c in t["cuts"]):
            return tiles * k
    return None


def run(neo, I, O, B, P, parts, routes, x, method="upols", options=None):
    conv = neo.MatrixConvolver(I, O, B, P, method=method, options=options)
    conv.filter(parts, routes)
    y = conv.process(x)
    info = conv.info()
    conv.close()
    return y, info


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("I,O,B,P,nb", SHAPES)
def test_shapes_and_options(neo_gpu, oracle, I, O, B, P, nb, method):
    neo = neo_gpu
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    cap = 4 if B <= 512 else 2 if B == 1024 else 1
    seen_split = False
    for out_tile in (1, 2, 4):
        forced = inside_cut_split(neo, I, O, B, P, rt, out_tile)
        for fused in (0, 1):
            for split in (0, forced):
                if split is None:
                    continue
                opts = {"fused": fused, "out_tile": out_tile, "split_workgroups": split}
                y, info = run(neo, I, O, B, P, parts, rt, x, method, opts)
                err = peak_err(y, ref)
                print(f"{(I, O, B, P, nb)} {method} {opts}: S {info['splits']} tiles {info['tiles']} err {err:.3g}")
                assert info["out_tile"] == min(out_tile, cap) and info["fused"] == fused
                assert info["tiles"] == -(-O // info["out_tile"])
                if split:
                    assert info["splits"] > 1
                    seen_split = True
                assert err <= TOL, (opts, err)
    assert seen_split or P * I == 1
    # the defaults
    y, info = run(neo, I, O, B, P, parts, rt, x, method)
    assert peak_err(y, ref) <= TOL
    assert info["routes"] == I * O and info["fdl_bytes"] == I * P * B * 8 and info["filter_bytes"] == I * O * P * B * 8


ROUTE_SHAPE = (4, 4, 64, 5, 30)
ROUTE_LISTS = {
    "diagonal": [(k, k) for k in range(4)],
    "lower": [(o, i) for o in range(4) for i in range(o + 1)],
    "no_output_1": [(0, 0), (0, 3), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3)],
    "no_input_2": [(0, 0), (0, 1), (1, 1), (1, 3), (2, 0), (2, 3), (3, 0), (3, 1), (3, 3)],
}


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("name", list(ROUTE_LISTS))
def test_route_lists(neo_gpu, oracle, name, method):
    neo = neo_gpu
    I, O, B, P, nb = ROUTE_SHAPE
    routes = ROUTE_LISTS[name]
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb, routes)
    ref = reference(oracle, I, O, B, P, nb, method, routes)
    rng = np.random.default_rng(3)
    perm = [int(k) for k in rng.permutation(len(routes))]
    for out_tile in (1, 2, 4):
        for fused in (0, 1):
            opts = {"out_tile": out_tile, "fused": fused, "split_workgroups": 3 * -(-O // out_tile)}
            y, info = run(neo, I, O, B, P, parts, routes, x, method, opts)
            err = peak_err(y, ref)
            print(f"{name} {method} {opts}: S {info['splits']} err {err:.3g}")
            assert err <= TOL, (opts, err)
            if name == "no_output_1":
                assert not y[1].any(), "an output without a route must be exactly zero"
            # the same list in another order: the same bits
            ys, _ = run(neo, I, O, B, P, parts[perm], [routes[k] for k in perm], x, method, opts)
            assert_same_bits(ys, y, f"{name} shuffled")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_repeatable_and_blockwise(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 9, 40
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    for opts in ({"out_tile": 4, "fused": 1, "split_workgroups": 6}, {"out_tile": 2, "fused": 0, "split_workgroups": 9}):
        y0, _ = run(neo, I, O, B, P, parts, rt, x, method, opts)
        y1, _ = run(neo, I, O, B, P, parts, rt, x, method, opts)
        assert_same_bits(y1, y0, "two fresh handles")
        conv = neo.MatrixConvolver(I, O, B, P, method=method, options=opts)
        conv.filter(parts, rt)
        yb = np.concatenate([conv.process(x[:, t * B:(t + 1) * B]) for t in range(nb)], axis=1)
        conv.close()
        assert_same_bits(yb, y0, "n calls of one block against one call of n blocks")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_reset_and_second_filter_restart_cleanly(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 37, 80
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    opts = {"out_tile": 2, "split_workgroups": 5}
    fresh, _ = run(neo, I, O, B, P, parts, rt, x, method, opts)
    conv = neo.MatrixConvolver(I, O, B, P, method=method, options=opts)
    conv.filter(parts, rt)
    conv.process(x[:, :13 * B])
    conv.reset()
    assert_same_bits(conv.process(x), fresh, "after reset")
    conv.process(x[:, :7 * B])
    # another route list in mid-stream, then the first one again
    conv.filter(parts[:1], [(1, 0)])
    y = conv.process(x[:, :3 * B])
    assert not y[0].any() and y[1].any()
    assert conv.info()["routes"] == 1
    conv.filter(parts, rt)
    assert_same_bits(conv.process(x), fresh, "after a second set_filter")
    conv.close()


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_set_impulse_against_filter(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 9, 40
    rt, x, ir, irn, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    opts = {"out_tile": 4}
    want, _ = run(neo, I, O, B, P, parts, rt, x, method, opts)
    conv = neo.MatrixConvolver(I, O, B, P, method=method, options=opts)
    conv.set_impulse(ir.reshape(O, I, -1))  # dense [O][I][L], normalized over all routes
    got = conv.process(x)
    assert peak_err(got, want) <= TOL and peak_err(got, ref) <= TOL
    conv.set_impulse(irn, routes=rt, normalize=False)
    got = conv.process(x)
    assert peak_err(got, want) <= TOL and peak_err(got, ref) <= TOL
    conv.close()
    # the one-shot
    got = neo.matrix_convolve(x, ir.reshape(O, I, -1), B, method=method)
    assert peak_err(got, ref) <= TOL
    sub = [(0, 0), (2, 1), (4, 2)]
    rs = reference(oracle, I, 5, B, P, nb, method, tuple(sub))
    _, _, irs, _, _ = problem(oracle, I, 5, B, P, nb, tuple(sub))
    assert peak_err(neo.matrix_convolve(x, irs, B, routes=sub, method=method), rs) <= TOL


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("fused", [0, 1])
def test_io_contract(neo_gpu, oracle, method, fused):
    import torch

    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 9, 40
    n = nb * B
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    opts = {"out_tile": 4, "fused": fused, "split_workgroups": 6}
    want, _ = run(neo, I, O, B, P, parts, rt, x, method, opts)
    assert peak_err(want, ref) <= TOL
    ld_in, ld_out = n + 36, n + 4
    ia = _arena(torch, I, ld_in, IN_FILL)
    ia.view(torch.float32)[1:I + 1, :n] = torch.from_numpy(np.array(x)).cuda()
    oa = _arena(torch, O, ld_out, OUT_FILL)
    before = ia.cpu().numpy()
    conv = neo.MatrixConvolver(I, O, B, P, method=method, options=opts)
    conv.filter(parts, rt)
    conv.process_device(ia.data_ptr() + 4 * ld_in, ld_in, oa.data_ptr() + 4 * ld_out, ld_out, nb)
    torch.cuda.synchronize()
    assert np.array_equal(ia.cpu().numpy(), before), "the call changed its input"
    assert_same_bits(check_regions(oa.cpu().numpy(), O, n, OUT_FILL), want, "separate strided arenas")

    # refused calls leave the state as it was: the next blocks continue the stream
    conv.reset()
    half = (nb // 2) * B
    ip, op = ia.data_ptr() + 4 * ld_in, oa.data_ptr() + 4 * ld_out
    conv.process_device(ip, ld_in, op, ld_out, nb // 2)
    for bad in ((ip + 4 * half, ld_in + 2, op + 4 * half, ld_out, nb - nb // 2),      # ld_in no multiple of 4
                (ip + 4 * half, ld_in, op + 4 * half, ld_out - 2, nb - nb // 2),      # ld_out no multiple of 4
                (ip + 4 * half + 4, ld_in, op + 4 * half, ld_out, nb - nb // 2),      # misaligned input
                (ip + 4 * half, ld_in, op + 4 * half + 8, ld_out, nb - nb // 2),      # misaligned output
                (ip + 4 * half, B * (nb - nb // 2) - 4, op + 4 * half, ld_out, nb - nb // 2),  # ld_in too small
                (ip + 4 * half, ld_in, op + 4 * half, B, 2)):                         # ld_out too small
        with pytest.raises(neo._native.NeoHipError):
            conv.process_device(*bad)
    conv.process_device(ip + 4 * half, ld_in, op + 4 * half, ld_out, nb - nb // 2)
    torch.cuda.synchronize()
    assert_same_bits(check_regions(oa.cpu().numpy(), O, n, OUT_FILL), want, "after refused calls")
    conv.close()


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_in_place(neo_gpu, oracle, method):
    import torch

    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 37, 80
    n = nb * B
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    for opts in ({"out_tile": 2, "fused": 1, "split_workgroups": 5}, {"out_tile": 1, "fused": 0}):
        want, _ = run(neo, I, O, B, P, parts, rt, x, method, opts)
        ld = n + 4
        a = _arena(torch, I, ld, OUT_FILL)
        a.view(torch.float32)[1:I + 1, :n] = torch.from_numpy(np.array(x)).cuda()
        conv = neo.MatrixConvolver(I, O, B, P, method=method, options=opts)
        conv.filter(parts, rt)
        conv.process_device(a.data_ptr() + 4 * ld, ld, a.data_ptr() + 4 * ld, ld, nb)
        torch.cuda.synchronize()
        conv.close()
        assert_same_bits(check_regions(a.cpu().numpy(), O, n, OUT_FILL), want, "in == out")


def test_torch_tensors(neo_gpu, oracle):
    import torch

    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 9, 40
    rt, x, ir, _, parts = problem(oracle, I, O, B, P, nb)
    want, _ = run(neo, I, O, B, P, parts, rt, x)
    conv = neo.MatrixConvolver(I, O, B, P)
    conv.filter(torch.from_numpy(np.array(parts)).cuda().reshape(O, I, P, B + 1))
    y = conv.process(torch.from_numpy(np.array(x)).cuda())
    assert y.is_cuda and tuple(y.shape) == (O, nb * B)
    assert_same_bits(y.cpu().numpy(), want, "device tensors")
    conv.set_impulse(torch.from_numpy(np.array(ir)).cuda())
    y2 = conv.process(torch.from_numpy(np.array(x)).cuda())
    assert peak_err(y2.cpu().numpy(), want) <= TOL
    conv.close()
    with pytest.raises(neo._native.NeoHipError):
        neo.MatrixConvolver(2, 2, 64, 3).process(np.zeros((2, 64), np.float32))  # no filter set


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_input_reaches_only_the_outputs_it_feeds(neo_gpu, oracle, method):
    """An input full of NaN poisons the outputs it is routed to and no other, also where they share
    a tile with such an output (the FDL row is loaded for the tile; an output without a route from
    that input takes no term from it, not 0 * NaN)."""
    neo = neo_gpu
    I, O, B, P, nb = ROUTE_SHAPE
    routes = ROUTE_LISTS["lower"]  # input 3 feeds output 3 alone
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb, routes)
    bad = np.array(x)
    bad[3] = np.nan
    for out_tile in (1, 2, 4):
        for fused in (0, 1):
            opts = {"out_tile": out_tile, "fused": fused, "split_workgroups": 3 * -(-O // out_tile)}
            clean, _ = run(neo, I, O, B, P, parts, routes, x, method, opts)
            y, _ = run(neo, I, O, B, P, parts, routes, bad, method, opts)
            assert_same_bits(y[:3], clean[:3], f"outputs 0..2 beside a NaN input, {opts}")
            assert np.isnan(y[3]).all()
