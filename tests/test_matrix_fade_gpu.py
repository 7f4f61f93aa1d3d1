"""Live filter updates of the matrix convolver on the device (neo_hip_matrix_update_filter,
neo.MatrixConvolver.update_filter). Definition: a handle with filter A that has processed blocks
0 .. k-1 gets an update to filter B over F blocks; with y_A, y_B the outputs of two convolvers with A
and B fed the whole input, the blocks before k are y_A, sample n of the fade is
(1 - g[n]) y_A + g[n] y_B with g = neo.matrix_fade_gains, the blocks from k + F on are y_B.
Reference: that mix, in float64, of the two per-route oracle sums of test_matrix_gpu.reference. Bar:
the project's, conftest.peak_err <= 1e-5. The sharp checks are the bit comparisons: no state is
touched, so after the fade the handle equals one that had B from block 0."""
import numpy as np
import pytest

from conftest import peak_err
from test_io_contract_gpu import OUT_FILL, _arena, assert_same_bits, check_regions
from test_matrix_gpu import dense, problem, reference

pytestmark = pytest.mark.gpu
TOL = 1e-5

# (I, O, B, P, blocks, update at block k)
SHAPES = [
    (1, 1, 16, 3, 20, 7),      # degenerate; 32 row groups fold
    (2, 2, 32, 37, 80, 50),    # the ring has wrapped at the update
    (3, 5, 128, 9, 40, 11),    # I != O
    (4, 3, 512, 70, 20, 6),    # several splits
    (2, 2, 1024, 20, 12, 5),   # two float4 per lane
    (1, 2, 4096, 3, 8, 3),     # the largest block: four column chunks per row
]

_cache = {}


def bank_b(oracle, I, O, B, P, routes=None, off=100000):
    """A second filter for the same route list: other seeds, normalized like the first."""
    key = (I, O, B, P, None if routes is None else tuple(routes), off)
    if key not in _cache:
        rt = dense(I, O) if routes is None else list(routes)
        ir = np.stack([oracle.noise(off + 5000 + 11 * B + 64 * o + i, P * B) for o, i in rt])
        irn = oracle.normalize_impulse(ir)
        parts = oracle.uniform_partition(irn, B)
        for a in (ir, irn, parts):
            a.setflags(write=False)
        _cache[key] = (ir, irn, parts)
    return _cache[key]


def reference_b(oracle, I, O, B, P, nb, method, routes=None, off=100000):
    key = ("r", I, O, B, P, nb, method, None if routes is None else tuple(routes), off)
    if key not in _cache:
        rt, x, _, _, _ = problem(oracle, I, O, B, P, nb, routes)
        parts = bank_b(oracle, I, O, B, P, routes, off)[2]
        per_route = oracle.dense_convolve(x[[i for _, i in rt]], parts, method=method)
        ref = np.zeros((O, nb * B), np.float64)
        for o in range(O):
            for i in range(I):
                if (o, i) in rt:
                    ref[o] += per_route[rt.index((o, i))]
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def mixed(neo, ya, yb, B, k, F, curve):
    """The definition's output for an update at block k: float64."""
    g = neo.matrix_fade_gains(B, F, curve).astype(np.float64)
    ref = np.array(ya, dtype=np.float64)
    ref[:, k * B:(k + F) * B] = (1.0 - g) * ya[:, k * B:(k + F) * B] + g * yb[:, k * B:(k + F) * B]
    ref[:, (k + F) * B:] = yb[:, (k + F) * B:]
    return ref


def split_opts(I, O, B, P):
    """out_tile 1 and a workgroup target that gives the step and the fade several splits (one row: none)."""
    return {"out_tile": 1, "split_workgroups": 3 * O * (B // 1024 if B > 1024 else 1)} if I * P > 1 else {"out_tile": 1}


def plain(neo, I, O, B, P, parts, rt, x, method, opts):
    conv = neo.MatrixConvolver(I, O, B, P, method=method, options=opts)
    conv.filter(parts, rt)
    y = conv.process(x)
    conv.close()
    return y


def faded(neo, I, O, B, P, pa, pb, rt, x, method, opts, k, F, curve, tensors=False):
    """Filter A, blocks 0 .. k-1, the update, the rest in one call."""
    conv = neo.MatrixConvolver(I, O, B, P, method=method, options=opts)
    conv.filter(pa, rt)
    assert conv.fade_info() == {"remaining_blocks": 0, "fade_blocks": 0, "bank_bytes": 0}
    if tensors:
        import torch

        xt = torch.from_numpy(np.array(x)).cuda()
        head = conv.process(xt[:, :k * B].contiguous()) if k else None
        conv.update_filter(torch.from_numpy(np.array(pb)).cuda(), fade_blocks=F, curve=curve)
        info = conv.fade_info()
        tail = conv.process(xt[:, k * B:].contiguous())
        y = (torch.cat([head, tail], dim=1) if k else tail).cpu().numpy()
    else:
        head = conv.process(x[:, :k * B]) if k else np.zeros((O, 0), np.float32)
        conv.update_filter(pb, fade_blocks=F, curve=curve)
        info = conv.fade_info()
        y = np.concatenate([head, conv.process(x[:, k * B:])], axis=1)
    assert info == {"remaining_blocks": F, "fade_blocks": F, "bank_bytes": conv.info()["filter_bytes"]}
    assert conv.fade_info()["remaining_blocks"] == 0
    conv.close()
    return y


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("I,O,B,P,nb,k", SHAPES)
def test_shapes_curves_and_lengths(neo_gpu, oracle, I, O, B, P, nb, k, method):
    neo = neo_gpu
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb)
    pb = bank_b(oracle, I, O, B, P)[2]
    ya, yb = reference(oracle, I, O, B, P, nb, method), reference_b(oracle, I, O, B, P, nb, method)
    for opts in ({}, split_opts(I, O, B, P)):
        never = plain(neo, I, O, B, P, pa, rt, x, method, opts)
        always = plain(neo, I, O, B, P, pb, rt, x, method, opts)
        assert peak_err(never, ya) <= TOL and peak_err(always, yb) <= TOL
        for F in (1, 3):
            for curve in ("linear", "cosine"):
                y = faded(neo, I, O, B, P, pa, pb, rt, x, method, opts, k, F, curve)
                err = peak_err(y, mixed(neo, ya, yb, B, k, F, curve))
                print(f"{(I, O, B, P, nb)} {method} {opts} k {k} F {F} {curve}: err {err:.3g}")
                assert err <= TOL, (opts, F, curve, err)
                # no state was touched: before the update the handle that never got one, after the
                # fade the handle that had B from block 0 (overlap-add: its first block after the
                # fade carries a tail summed in the fade kernel's order)
                assert_same_bits(y[:, :k * B], never[:, :k * B], "blocks before the update")
                first = k + F + (1 if method == "upola" else 0)
                assert_same_bits(y[:, first * B:], always[:, first * B:], "blocks after the fade")
                assert first < nb


def test_device_tensors(neo_gpu, oracle):
    neo = neo_gpu
    I, O, B, P, nb, k = 3, 5, 128, 9, 40, 11
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb)
    pb = bank_b(oracle, I, O, B, P)[2]
    for method in ("upols", "upola"):
        want = faded(neo, I, O, B, P, pa, pb, rt, x, method, {}, k, 3, "cosine")
        got = faded(neo, I, O, B, P, pa, pb, rt, x, method, {}, k, 3, "cosine", tensors=True)
        assert_same_bits(got, want, "device tensors against host arrays")


SPARSE_SHAPE = (4, 4, 64, 5, 30)
SPARSE_ROUTES = [(0, 0), (0, 3), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3)]  # output 1: none; input 3: outputs 0, 3


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_sparse_routes_and_nan_isolation(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = SPARSE_SHAPE
    k, F = 9, 3
    routes = SPARSE_ROUTES
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb, routes)
    pb = bank_b(oracle, I, O, B, P, routes)[2]
    ya = reference(oracle, I, O, B, P, nb, method, routes)
    yb = reference_b(oracle, I, O, B, P, nb, method, tuple(routes))
    for opts in ({}, {"out_tile": 4, "split_workgroups": 3}):
        y = faded(neo, I, O, B, P, pa, pb, rt, x, method, opts, k, F, "linear")
        assert peak_err(y, mixed(neo, ya, yb, B, k, F, "linear")) <= TOL
        assert not y[1].any(), "an output without a route must be exactly zero"
        bad = np.array(x)
        bad[3, (k + 1) * B:(k + 2) * B] = np.nan  # inside the fade
        yn = faded(neo, I, O, B, P, pa, pb, rt, bad, method, opts, k, F, "linear")
        assert_same_bits(yn[[1, 2]], y[[1, 2]], "outputs 1, 2 beside a NaN in input 3")
        assert np.isnan(yn[0]).any() and np.isnan(yn[3]).any()


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_in_place_across_a_fade(neo_gpu, oracle, method):
    import torch

    neo = neo_gpu
    I, O, B, P, nb, k, F = 2, 2, 32, 37, 80, 50, 3
    n = nb * B
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb)
    pb = bank_b(oracle, I, O, B, P)[2]
    want = faded(neo, I, O, B, P, pa, pb, rt, x, method, {}, k, F, "cosine")
    ld = n + 4
    a = _arena(torch, I, ld, OUT_FILL)
    a.view(torch.float32)[1:I + 1, :n] = torch.from_numpy(np.array(x)).cuda()
    conv = neo.MatrixConvolver(I, O, B, P, method=method)
    conv.filter(pa, rt)
    p = a.data_ptr() + 4 * ld
    conv.process_device(p, ld, p, ld, k)
    conv.update_filter(torch.from_numpy(np.array(pb)).cuda(), fade_blocks=F, curve="cosine")
    conv.process_device(p + 4 * k * B, ld, p + 4 * k * B, ld, nb - k)
    torch.cuda.synchronize()
    conv.close()
    assert_same_bits(check_regions(a.cpu().numpy(), O, n, OUT_FILL), want, "in == out across a fade")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_two_updates_and_an_update_before_the_first_block(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 9, 40
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb)
    pb = bank_b(oracle, I, O, B, P)[2]
    pc = bank_b(oracle, I, O, B, P, off=200000)[2]
    ya, yb = reference(oracle, I, O, B, P, nb, method), reference_b(oracle, I, O, B, P, nb, method)
    yc = reference_b(oracle, I, O, B, P, nb, method, off=200000)
    k1, F1, k2, F2 = 6, 3, 20, 2
    conv = neo.MatrixConvolver(I, O, B, P, method=method)
    conv.filter(pa, rt)
    bank = conv.info()["filter_bytes"]
    parts = [conv.process(x[:, :k1 * B])]
    conv.update_filter(pb, fade_blocks=F1, curve="linear")
    parts.append(conv.process(x[:, k1 * B:k2 * B]))
    assert conv.fade_info() == {"remaining_blocks": 0, "fade_blocks": 0, "bank_bytes": bank}
    conv.update_filter(pc, fade_blocks=F2, curve="cosine")
    parts.append(conv.process(x[:, k2 * B:]))
    conv.close()
    y = np.concatenate(parts, axis=1)
    ref = mixed(neo, ya, yb, B, k1, F1, "linear")
    ref[:, k2 * B:] = mixed(neo, yb, yc, B, k2, F2, "cosine")[:, k2 * B:]
    assert peak_err(y, ref) <= TOL
    always_c = plain(neo, I, O, B, P, pc, rt, x, method, {})
    first = k2 + F2 + (1 if method == "upola" else 0)
    assert_same_bits(y[:, first * B:], always_c[:, first * B:], "after the second fade")
    # an update before the first block ever processed
    y0 = faded(neo, I, O, B, P, pa, pb, rt, x, method, {}, 0, 3, "linear")
    assert peak_err(y0, mixed(neo, ya, yb, B, 0, 3, "linear")) <= TOL
    always_b = plain(neo, I, O, B, P, pb, rt, x, method, {})
    first = 3 + (1 if method == "upola" else 0)
    assert_same_bits(y0[:, first * B:], always_b[:, first * B:], "after a fade from block 0")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_refused_updates_leave_the_fade_intact(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb, k, F = 2, 2, 32, 37, 80, 50, 3
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb)
    pb = bank_b(oracle, I, O, B, P)[2]
    pc = bank_b(oracle, I, O, B, P, off=200000)[2]
    want = faded(neo, I, O, B, P, pa, pb, rt, x, method, {}, k, F, "linear")
    conv = neo.MatrixConvolver(I, O, B, P, method=method)
    with pytest.raises(neo._native.NeoHipError):
        conv.update_filter(pb)  # before a filter is set
    conv.filter(pa, rt)
    parts = [conv.process(x[:, :k * B])]
    for bad in ({"fade_blocks": 0}, {"fade_blocks": -2}, {"curve": 7}):
        with pytest.raises(neo._native.NeoHipError):
            conv.update_filter(pb, **bad)
        assert conv.fade_info() == {"remaining_blocks": 0, "fade_blocks": 0, "bank_bytes": 0}
    with pytest.raises(ValueError):
        conv.update_filter(pb[:1])
    conv.update_filter(pb, fade_blocks=F)
    parts.append(conv.process(x[:, k * B:(k + 1) * B]))
    with pytest.raises(neo._native.NeoHipError):
        conv.update_filter(pc, fade_blocks=2)  # a fade is running
    with pytest.raises(neo._native.NeoHipError):
        conv.update_impulse(np.zeros((I * O, P * B), np.float32))
    assert conv.fade_info()["remaining_blocks"] == F - 1
    parts.append(conv.process(x[:, (k + 1) * B:]))
    conv.close()
    assert_same_bits(np.concatenate(parts, axis=1), want, "a refused update changed the running fade")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_reset_and_set_filter_in_mid_fade(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb, k = 2, 2, 32, 37, 80, 50
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb)
    pb = bank_b(oracle, I, O, B, P)[2]
    fresh_a = plain(neo, I, O, B, P, pa, rt, x, method, {})
    fresh_b = plain(neo, I, O, B, P, pb, rt, x, method, {})
    conv = neo.MatrixConvolver(I, O, B, P, method=method)
    conv.filter(pa, rt)
    conv.process(x[:, :k * B])
    conv.update_filter(pb, fade_blocks=5)
    conv.process(x[:, k * B:(k + 2) * B])
    conv.reset()  # clears the state and completes the fade
    assert conv.fade_info()["remaining_blocks"] == 0
    assert_same_bits(conv.process(x), fresh_b, "reset in mid-fade: a fresh handle with B")
    conv.update_filter(pa, fade_blocks=5)
    conv.process(x[:, :2 * B])
    conv.filter(pa, rt)  # cancels the fade, resets as ever
    assert conv.fade_info() == {"remaining_blocks": 0, "fade_blocks": 0, "bank_bytes": 0}
    assert_same_bits(conv.process(x), fresh_a, "set_filter in mid-fade")
    conv.close()


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_update_impulse(neo_gpu, oracle, method):
    import torch

    neo = neo_gpu
    I, O, B, P, nb, k, F = 3, 5, 128, 9, 40, 11, 3
    rt, x, ir_a, _, pa = problem(oracle, I, O, B, P, nb)
    ir_b, irn_b, pb = bank_b(oracle, I, O, B, P)
    want = faded(neo, I, O, B, P, pa, pb, rt, x, method, {}, k, F, "cosine")
    for form in ("normalize", "given", "tensor"):
        conv = neo.MatrixConvolver(I, O, B, P, method=method)
        conv.set_impulse(ir_a, routes=rt)
        head = conv.process(x[:, :k * B])
        if form == "normalize":
            conv.update_impulse(ir_b, fade_blocks=F, curve="cosine")
        elif form == "given":
            conv.update_impulse(irn_b, normalize=False, fade_blocks=F, curve="cosine")
        else:
            conv.update_impulse(torch.from_numpy(np.array(ir_b)).cuda(), fade_blocks=F, curve="cosine")
        assert conv.fade_info()["remaining_blocks"] == F
        y = np.concatenate([head, conv.process(x[:, k * B:])], axis=1)
        conv.close()
        assert peak_err(y, want) <= TOL, form


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_batching_and_offline_windows_follow_the_new_filter(neo_gpu, oracle, method):
    """Batching and offline windows on: an update, then ONE call of 1 + 256 + 40 blocks with F = 3:
    three fade steps, an offline pass of 256 blocks whose segment spectra must be the new filter's,
    batched passes and steps. Turning both on in mid-fade (the ring re-laid twice) keeps the fade."""
    neo = neo_gpu
    I, O, B, P = 2, 2, 16, 5
    k, F, rest = 256 + 4, 3, 1 + 256 + 40  # the head runs an offline pass with A's segment spectra
    nb = k + rest + 3
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb)
    pb = bank_b(oracle, I, O, B, P)[2]
    ya, yb = reference(oracle, I, O, B, P, nb, method), reference_b(oracle, I, O, B, P, nb, method)
    # gears on before the update
    conv = neo.MatrixConvolver(I, O, B, P, method=method)
    conv.filter(pa, rt)
    conv.set_batch(True)
    conv.set_offline(True)
    head = conv.process(x[:, :k * B])
    assert conv.offline_info()["spectra_bytes"] > 0, "no offline pass ran with the first filter"
    conv.update_filter(pb, fade_blocks=F, curve="linear")
    body = conv.process(x[:, k * B:(k + rest) * B])
    assert conv.fade_info()["remaining_blocks"] == 0
    tail = conv.process(x[:, (k + rest) * B:])
    conv.close()
    y = np.concatenate([head, body, tail], axis=1)
    ref = mixed(neo, ya, yb, B, k, F, "linear")
    err = peak_err(y[:, k * B:(k + rest) * B], ref[:, k * B:(k + rest) * B])
    print(f"{method}: the call of {rest} blocks err {err:.3g}")
    assert err <= TOL
    assert peak_err(y, ref) <= TOL
    # gears turned on in mid-fade: the ring is re-laid, the fade goes on
    conv = neo.MatrixConvolver(I, O, B, P, method=method)
    conv.filter(pa, rt)
    parts = [conv.process(x[:, :k * B])]
    conv.update_filter(pb, fade_blocks=F, curve="linear")
    parts.append(conv.process(x[:, k * B:(k + 1) * B]))
    conv.set_batch(True)
    parts.append(conv.process(x[:, (k + 1) * B:(k + 2) * B]))
    conv.set_offline(True)
    assert conv.fade_info()["remaining_blocks"] == 1
    parts.append(conv.process(x[:, (k + 2) * B:]))
    conv.close()
    assert peak_err(np.concatenate(parts, axis=1), ref) <= TOL


GEARS_R1 = [(0, 0), (0, 2), (1, 1)]


@pytest.mark.parametrize("r2", [None, [(1, 0)]], ids=["dense", "one-route"])
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_every_gear_on_one_handle_across_a_change_of_route_list(neo_gpu, oracle, method, r2):
    """Batching and offline windows on before the first filter; route list R1: ONE call of 163 blocks
    (an offline window, a pass of 32, passes of 2 and 1); an update over 3 blocks, calls of 5 and 160
    blocks (the second offline pass runs on the new filter's spectra); then filter() with another
    route list R2 (all six routes, or (1, 0) alone: output 0 has none) and 163 blocks more. The
    buffers of the three gears follow the filter: gone at that filter(), back at the next use, and
    the handle equals one that only ever saw R2."""
    neo = neo_gpu
    I, O, B, P = 3, 2, 16, 129  # two offline segments
    n1, F, n2, n3, n4 = 163, 3, 5, 160, 163
    nb = n1 + n2 + n3
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb, GEARS_R1)
    pb = bank_b(oracle, I, O, B, P, GEARS_R1)[2]
    ref = mixed(neo, reference(oracle, I, O, B, P, nb, method, GEARS_R1),
                reference_b(oracle, I, O, B, P, nb, method, tuple(GEARS_R1)), B, n1, F, "cosine")
    rt2, x2, _, _, p2 = problem(oracle, I, O, B, P, n4 + 2, r2)
    ref2 = reference(oracle, I, O, B, P, n4 + 2, method, r2)

    def geared():
        c = neo.MatrixConvolver(I, O, B, P, method=method)
        c.set_batch(True)
        c.set_offline(True)
        return c

    conv = geared()
    conv.filter(pa, rt)
    assert conv.offline_info()["spectra_bytes"] == 0 and conv.fade_info()["bank_bytes"] == 0
    cuts = np.cumsum([0, n1, n2, n3]) * B
    ys = [conv.process(x[:, cuts[0]:cuts[1]])]
    spectra = len(rt) * 2 * 256 * B * 8
    assert conv.offline_info()["spectra_bytes"] == spectra
    conv.update_filter(pb, fade_blocks=F, curve="cosine")
    assert conv.fade_info() == {"remaining_blocks": F, "fade_blocks": F, "bank_bytes": conv.info()["filter_bytes"]}
    ys += [conv.process(x[:, cuts[1]:cuts[2]]), conv.process(x[:, cuts[2]:cuts[3]])]
    assert conv.fade_info()["remaining_blocks"] == 0
    for k, y in enumerate(ys):
        err = peak_err(y, ref[:, cuts[k]:cuts[k + 1]])
        print(f"{method} R1 stage {k}: err {err:.3g}")
        assert err <= TOL, (k, err)
    # another route list: the three groups are freed with the filter
    conv.filter(p2, rt2)
    assert conv.info()["routes"] == len(rt2)
    assert conv.fade_info() == {"remaining_blocks": 0, "fade_blocks": 0, "bank_bytes": 0}
    assert conv.offline_info()["spectra_bytes"] == 0
    y4 = conv.process(x2[:, :n4 * B])
    err = peak_err(y4, ref2[:, :n4 * B])
    print(f"{method} R2 {len(rt2)} routes: err {err:.3g}")
    assert err <= TOL
    assert conv.offline_info()["spectra_bytes"] == len(rt2) * 2 * 256 * B * 8
    fresh = geared()
    fresh.filter(p2, rt2)
    assert_same_bits(y4, fresh.process(x2[:, :n4 * B]), "after filter() with another route list: a fresh handle")
    fresh.close()
    if r2 is not None:
        assert not y4[0].any(), "an output without a route must be exactly zero"
    # the fade's buffers at their next use: an update to the same filter changes nothing
    conv.update_filter(p2, fade_blocks=1)
    assert conv.fade_info()["bank_bytes"] == conv.info()["filter_bytes"] == len(rt2) * P * B * 8
    y5 = conv.process(x2[:, n4 * B:])
    conv.close()
    assert peak_err(np.concatenate([y4, y5], axis=1), ref2) <= TOL
