"""Window levels of the matrix convolver on the device (neo_hip_matrix_set_levels,
MatrixConvolver.set_levels): long filters one block per call. Reference and bar are those of
tests/test_matrix_gpu.py: per output the float64 sum over its routes of the oracle's dense_convolve,
conftest.peak_err <= 1e-5. Both methods everywhere."""
import numpy as np
import pytest

from conftest import peak_err
from test_io_contract_gpu import IN_FILL, OUT_FILL, _arena, assert_same_bits, check_regions
from test_matrix_fade_gpu import bank_b, mixed, reference_b
from test_matrix_gpu import ROUTE_LISTS, ROUTE_SHAPE, problem, reference

pytestmark = pytest.mark.gpu
TOL = 1e-5
METHODS = ["upols", "upola"]
FOUR = (4, 8, 16, 32)  # the issue's list; None is the default, which became (8, 32) with the sweep

# (I, O, B, P, blocks, window lists)
SHAPES = [
    (1, 1, 16, 9, 40, (FOUR,)),      # one level with a one-partition band; 16 live bins of 64 lanes
    (2, 2, 32, 70, 140, (FOUR, (32,), (8, 32), None)),  # all four levels; last band shorter than T; ring wraps; > 4 windows of 32
    (3, 5, 128, 37, 100, (FOUR,)),   # I != O; T = 32 dropped
    (4, 3, 512, 100, 80, (FOUR, None)),   # two bin chunks; a forced split that cuts inside an input
    (1, 2, 1024, 20, 40, (FOUR,)),   # four bin chunks
    (1, 2, 4096, 12, 20, (FOUR,)),   # sixteen bin chunks
]


def inside_cut_target(neo, I, O, B, P, routes=None, windows=FOUR):
    """A split_workgroups (per part) that gives some level S > 1 with a run that starts or ends inside
    an input's band (None: no such target)."""
    for wgs in range(1, 40):
        p = neo.matrix_level_plan(I, O, B, P, routes=routes, windows=windows, split_workgroups=wgs)
        for lv in p["levels"]:
            if lv["splits"] > 1 and any(a != lv["first"] or b != lv["last"] for out in lv["outputs"] for s in out for _, a, b in s):
                return wgs
    return None


def make(neo, I, O, B, P, parts, routes, method, levels=True, windows=FOUR, split=0):
    conv = neo.MatrixConvolver(I, O, B, P, method=method)
    conv.filter(parts, routes)
    if levels:
        conv.set_levels(True, windows, split)
    return conv


def run(neo, I, O, B, P, parts, routes, x, method, levels=True, windows=FOUR, split=0):
    conv = make(neo, I, O, B, P, parts, routes, method, levels, windows, split)
    y = conv.process(x)
    info = conv.levels_info()
    conv.close()
    return y, info


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("I,O,B,P,nb,window_lists", SHAPES)
def test_shapes_windows_and_forced_splits(neo_gpu, oracle, I, O, B, P, nb, window_lists, method):
    neo = neo_gpu
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    for windows in window_lists:
        plan = neo.matrix_level_plan(I, O, B, P, windows=windows)
        assert plan["levels"], "the shape must have a level"
        forced = inside_cut_target(neo, I, O, B, P, windows=windows)
        assert forced or I * (P - plan["head"]) == 1
        for split in (0, forced):
            if split is None:
                continue
            y, info = run(neo, I, O, B, P, parts, rt, x, method, True, windows, split)
            err = peak_err(y, ref)
            print(f"{(I, O, B, P, nb)} {method} windows {windows} split {split}: levels "
                  f"{[(lv['window'], lv['splits']) for lv in info['levels']]} err {err:.3g}")
            want = neo.matrix_level_plan(I, O, B, P, windows=windows, split_workgroups=split)
            assert info["enabled"] and info["primed"] and info["head"] == want["head"]
            assert info["levels"] == [{k: lv[k] for k in ("window", "first", "last", "splits")} for lv in want["levels"]]
            assert err <= TOL, (windows, split, err)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(ROUTE_LISTS))
def test_route_lists(neo_gpu, oracle, name, method):
    neo = neo_gpu
    I, O, B, _, _ = ROUTE_SHAPE
    P, nb = 37, 90
    routes = ROUTE_LISTS[name]
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb, tuple(routes))
    ref = reference(oracle, I, O, B, P, nb, method, tuple(routes))
    y, info = run(neo, I, O, B, P, parts, routes, x, method)
    assert len(info["levels"]) == 3 and peak_err(y, ref) <= TOL
    for o in range(O):
        if not any(oo == o for oo, _ in routes):
            assert not y[o].view(np.int32).any(), f"output {o} has no route: exactly zero"
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(routes))
    ys, _ = run(neo, I, O, B, P, np.ascontiguousarray(parts[perm]), [routes[k] for k in perm], x, method)
    assert_same_bits(ys, y, f"{name} shuffled")
    y2, _ = run(neo, I, O, B, P, parts, routes, x, method)
    assert_same_bits(y2, y, f"{name}: two fresh handles")


@pytest.mark.parametrize("method", METHODS)
def test_one_call_and_one_call_per_block(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 70, 140
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    whole, _ = run(neo, I, O, B, P, parts, rt, x, method)
    conv = make(neo, I, O, B, P, parts, rt, method)
    single = np.concatenate([conv.process(x[:, n * B:(n + 1) * B]) for n in range(nb)], axis=1)
    assert conv.levels_info()["primed"]
    conv.close()
    assert_same_bits(single, whole, "one call per block")


@pytest.mark.parametrize("method", METHODS)
def test_toggling_reset_and_filter(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 70, 140
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    always, _ = run(neo, I, O, B, P, parts, rt, x, method)
    assert peak_err(always, ref) <= TOL
    # overlap-add: the first block after a switch adds the tail of the block before, whose spectrum was
    # summed in the plain step's order (as after a fade, tests/test_matrix_fade_gpu.py); from the next on
    skip = 1 if method == "upola" else 0
    for k in (5, 33, 70):
        conv = make(neo, I, O, B, P, parts, rt, method, levels=False)
        conv.process(x[:, :k * B])
        conv.set_levels(True, FOUR)
        assert not conv.levels_info()["primed"]
        y = conv.process(x[:, k * B:])
        assert conv.levels_info()["primed"]
        assert peak_err(y, ref[:, k * B:]) <= TOL
        assert_same_bits(y[:, skip * B:], always[:, (k + skip) * B:], f"levels turned on after {k} blocks")
        conv.close()
    # turned off again: the plain step continues; on again: the bits of the handle that never left
    conv = make(neo, I, O, B, P, parts, rt, method)
    a = conv.process(x[:, :50 * B])
    conv.set_levels(False)
    assert not conv.levels_info()["enabled"]
    b = conv.process(x[:, 50 * B:75 * B])
    conv.set_levels(True, FOUR)
    c = conv.process(x[:, 75 * B:])
    assert peak_err(np.concatenate([a, b, c], axis=1), ref) <= TOL
    assert_same_bits(a, always[:, :50 * B], "before the mode was turned off")
    assert_same_bits(c[:, skip * B:], always[:, (75 + skip) * B:], "after it was turned on again")
    # bad windows are refused and touch nothing
    before = conv.levels_info()
    for bad in ((8, 4), (3,), (4, 6), ()):
        with pytest.raises(neo._native.NeoHipError):
            conv.set_levels(True, bad)
    with pytest.raises(neo._native.NeoHipError):
        conv.set_levels(True, None, -1)
    assert conv.levels_info() == before
    # reset and a second filter restart cleanly
    conv.reset()
    assert conv.levels_info()["primed"]
    assert_same_bits(conv.process(x), always, "after reset")
    conv.process(x[:, :39 * B])
    conv.filter(parts[:1], [(1, 0)])
    assert conv.levels_info()["enabled"] and len(conv.levels_info()["levels"]) == 4
    y = conv.process(x[:, :35 * B])
    assert not y[0].any() and y[1].any()
    conv.filter(parts, rt)
    assert_same_bits(conv.process(x), always, "after a second set_filter")
    # another window list in mid-stream
    conv.reset()
    a = conv.process(x[:, :41 * B])
    conv.set_levels(True, (8, 32), 3)
    b = conv.process(x[:, 41 * B:])
    assert peak_err(np.concatenate([a, b], axis=1), ref) <= TOL
    conv.close()
    # a filter too short for a level: the ordinary step, 0 levels
    rt9, x9, _, _, parts9 = problem(oracle, 2, 2, 32, 8, 20)
    y, info = run(neo, 2, 2, 32, 8, parts9, rt9, x9, method)
    plain, _ = run(neo, 2, 2, 32, 8, parts9, rt9, x9, method, levels=False)
    assert info["enabled"] and info["levels"] == [] and info["head"] == 8
    assert_same_bits(y, plain, "P <= 2 T0: the ordinary step")


@pytest.mark.parametrize("method", METHODS)
def test_mixing_with_batched_passes(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 70, 140
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    conv = make(neo, I, O, B, P, parts, rt, method)
    conv.set_batch(True)
    assert conv.batch_info()["ring_rows"] == P + 31 == conv.levels_info()["ring_rows"]
    out, t = [], 0
    for n in (1, 40, 1, 1, 24, 3, nb - 70):  # single steps re-prime after each pass
        out.append(conv.process(x[:, t * B:(t + n) * B]))
        t += n
        assert conv.levels_info()["primed"] == (n in (1, 3))  # 40 = 32 + 8, 24 = 16 + 8, 3 = 2 + 1
    conv.close()
    y = np.concatenate(out, axis=1)
    err = peak_err(y, ref)
    print(f"{method} mixed with batched passes: err {err:.3g}")
    assert err <= TOL


@pytest.mark.parametrize("method", METHODS)
def test_live_updates_while_levels_are_on(neo_gpu, oracle, method):
    neo = neo_gpu
    I, O, B, P, nb, k = 2, 2, 32, 70, 140, 45
    rt, x, _, _, pa = problem(oracle, I, O, B, P, nb)
    pb = bank_b(oracle, I, O, B, P)[2]
    ya, yb = reference(oracle, I, O, B, P, nb, method), reference_b(oracle, I, O, B, P, nb, method)
    never, _ = run(neo, I, O, B, P, pa, rt, x, method)
    always, _ = run(neo, I, O, B, P, pb, rt, x, method)
    assert peak_err(always, yb) <= TOL
    for F in (1, 7):
        conv = make(neo, I, O, B, P, pa, rt, method)
        head = conv.process(x[:, :k * B])
        conv.update_filter(pb, fade_blocks=F, curve="cosine")
        # one block per call, as a real-time caller runs it
        tail = [conv.process(x[:, n * B:(n + 1) * B]) for n in range(k, nb)]
        assert conv.fade_info()["remaining_blocks"] == 0 and conv.levels_info()["primed"]
        conv.close()
        y = np.concatenate([head] + tail, axis=1)
        err = peak_err(y, mixed(neo, ya, yb, B, k, F, "cosine"))
        print(f"{method} fade of {F} blocks with levels on: err {err:.3g}")
        assert err <= TOL, (F, err)
        assert_same_bits(y[:, :k * B], never[:, :k * B], "blocks before the update")
        first = k + F + (1 if method == "upola" else 0)  # overlap-add: one tail in the fade kernel's order
        assert_same_bits(y[:, first * B:], always[:, first * B:], "blocks after the fade")


@pytest.mark.parametrize("method", METHODS)
def test_nan_leaves_with_the_filters_reach(neo_gpu, oracle, method):
    """A block of NaN in one input reaches only the outputs it feeds, through the head and every
    level, for as long as the filter reaches (P blocks, one more for the overlap); once its row has
    left every band those outputs are clean again."""
    neo = neo_gpu
    I, O, B, P, nb = 2, 2, 32, 70, 140
    routes = [(0, 0), (1, 0), (1, 1)]  # lower-triangular: input 1 feeds output 1 alone
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb, tuple(routes))
    clean, _ = run(neo, I, O, B, P, parts, routes, x, method)
    at = 21
    for bad_in, fed, free in ((0, (0, 1), ()), (1, (1,), (0,))):
        bad = np.array(x)
        bad[bad_in, at * B:(at + 1) * B] = np.nan
        y, _ = run(neo, I, O, B, P, parts, routes, bad, method)
        want, _ = run(neo, I, O, B, P, parts, routes, bad, method, levels=False)
        for o in fed:
            assert np.array_equal(np.isnan(y[o]), np.isnan(want[o])), (bad_in, o)
            assert np.isnan(y[o, at * B:(at + P) * B]).all()
            assert np.isfinite(y[o, (at + P + 1) * B:]).all(), (bad_in, o)
            ok = np.isfinite(want[o])
            scale = np.abs(want[o][ok]).max()
            assert np.abs(y[o][ok].astype(np.float64) - want[o][ok]).max() <= TOL * scale
            assert_same_bits(y[o:o + 1, (at + P + 1) * B:], clean[o:o + 1, (at + P + 1) * B:], "clean again")
        for o in free:
            assert_same_bits(y[o:o + 1], clean[o:o + 1], f"output {o} beside a NaN block of input {bad_in}")


@pytest.mark.parametrize("method", METHODS)
def test_io_contract_and_in_place(neo_gpu, oracle, method):
    import torch

    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 37, 100
    n = nb * B
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    ref = reference(oracle, I, O, B, P, nb, method)
    split = inside_cut_target(neo, I, O, B, P)
    want, _ = run(neo, I, O, B, P, parts, rt, x, method, True, FOUR, split)
    assert peak_err(want, ref) <= TOL
    ld_in, ld_out = n + 36, n + 4
    ia = _arena(torch, I, ld_in, IN_FILL)
    ia.view(torch.float32)[1:I + 1, :n] = torch.from_numpy(np.array(x)).cuda()
    oa = _arena(torch, O, ld_out, OUT_FILL)
    before = ia.cpu().numpy()
    conv = make(neo, I, O, B, P, parts, rt, method, True, FOUR, split)
    ip, op = ia.data_ptr() + 4 * ld_in, oa.data_ptr() + 4 * ld_out
    first = 37
    conv.process_device(ip, ld_in, op, ld_out, first)
    for bad in ((ip + 4 * first * B, ld_in + 2, op + 4 * first * B, ld_out, nb - first),  # ld_in no multiple of 4
                (ip + 4 * first * B + 4, ld_in, op + 4 * first * B, ld_out, nb - first),  # misaligned input
                (ip + 4 * first * B, ld_in, op + 4 * first * B, B, 2)):                   # ld_out too small
        with pytest.raises(neo._native.NeoHipError):
            conv.process_device(*bad)
    conv.process_device(ip + 4 * first * B, ld_in, op + 4 * first * B, ld_out, nb - first)
    torch.cuda.synchronize()
    conv.close()
    assert np.array_equal(ia.cpu().numpy(), before), "the calls changed their input"
    assert_same_bits(check_regions(oa.cpu().numpy(), O, n, OUT_FILL), want, "separate strided arenas")
    # in == out (I < O: the arena has the outputs' rows; every read of a block precedes its writes)
    ld = n + 4
    a = _arena(torch, O, ld, OUT_FILL)
    a.view(torch.float32)[1:I + 1, :n] = torch.from_numpy(np.array(x)).cuda()
    conv = make(neo, I, O, B, P, parts, rt, method, True, FOUR, split)
    conv.process_device(a.data_ptr() + 4 * ld, ld, a.data_ptr() + 4 * ld, ld, nb)
    torch.cuda.synchronize()
    conv.close()
    assert_same_bits(check_regions(a.cpu().numpy(), O, n, OUT_FILL), want, "in == out")


def test_info_calls_report_the_plan(neo_gpu, oracle):
    neo = neo_gpu
    I, O, B, P, nb = 3, 5, 128, 37, 100
    rt, x, _, _, parts = problem(oracle, I, O, B, P, nb)
    conv = neo.MatrixConvolver(I, O, B, P)
    off = conv.levels_info()
    assert off == {"enabled": False, "head": 0, "levels": [], "ring_rows": P, "primed": False, "partial_bytes": 0,
                   "head_bank_bytes": 0}
    conv.set_levels(True, (4, 16), 2)  # before the filter: kept, the plan follows the filter
    assert conv.levels_info()["enabled"] and conv.levels_info()["levels"] == []
    conv.filter(parts, rt)
    plan = neo.matrix_level_plan(I, O, B, P, windows=(4, 16), split_workgroups=2)
    li, info = conv.levels_info(), conv.info()
    assert li["levels"] == [{k: lv[k] for k in ("window", "first", "last", "splits")} for lv in plan["levels"]]
    assert [(lv["window"], lv["first"], lv["last"]) for lv in li["levels"]] == [(4, 8, 32), (16, 32, 37)]
    assert li["head"] == plan["head"] == 8 and li["ring_rows"] == plan["ring_rows"] == P
    assert li["partial_bytes"] == plan["partial_bytes"] and li["head_bank_bytes"] == plan["head_bank_bytes"]
    assert info["fdl_bytes"] == I * plan["ring_rows"] * B * 8 and info["filter_bytes"] == I * O * P * B * 8
    before = dict(info)
    conv.process(x[:, :10 * B])
    assert conv.info() == before and conv.levels_info() == li
    conv.close()
