"""The matrix convolver's host side, no GPU: neo_hip_matrix_plan on hand-checked cases (the same
function the handle is built from) and the argument checks that run before a device is touched."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")


def dense(I, O):
    return [(o, i) for o in range(O) for i in range(I)]


def test_dense_4x4_tiles_and_loads():
    import neo

    p = neo.matrix_plan(4, 4, 64, 5, options={"out_tile": 4})
    assert p["out_tile"] == 4 and len(p["tiles"]) == 1
    assert p["tiles"][0]["first"] == 0 and p["tiles"][0]["count"] == 4 and p["tiles"][0]["rows"] == 20
    assert p["fdl_row_loads"] == 20 and p["filter_row_loads"] == 80
    p = neo.matrix_plan(4, 4, 64, 5, options={"out_tile": 1})
    assert p["out_tile"] == 1 and len(p["tiles"]) == 4
    assert p["fdl_row_loads"] == 80 and p["filter_row_loads"] == 80
    # the bytes model: 8 B per row load plus the block I/O
    assert p["bytes"] == 8 * 64 * 160 + 4 * 64 * 8
    # the dense list is what routes=None means
    assert neo.matrix_plan(4, 4, 64, 5, routes=dense(4, 4), options={"out_tile": 1}) == p


def test_lower_triangular_unions():
    import neo

    tri = [(o, i) for o in range(4) for i in range(o + 1)]
    p = neo.matrix_plan(4, 4, 64, 5, routes=tri, options={"out_tile": 2})
    assert [t["inputs"] for t in p["tiles"]] == [[0, 1], [0, 1, 2, 3]]
    assert [t["rows"] for t in p["tiles"]] == [10, 20]
    assert p["filter_row_loads"] == len(tri) * 5 and p["fdl_row_loads"] == 30
    # the order of the list plays no part
    rng = np.random.default_rng(1)
    shuffled = [tri[k] for k in rng.permutation(len(tri))]
    q = neo.matrix_plan(4, 4, 64, 5, routes=shuffled, options={"out_tile": 2})
    assert q == p


def test_five_outputs_tiles_of_4_and_1():
    import neo

    p = neo.matrix_plan(3, 5, 128, 9, options={"out_tile": 4})
    assert [(t["first"], t["count"]) for t in p["tiles"]] == [(0, 4), (4, 1)]
    assert p["fdl_row_loads"] == 2 * 27 and p["filter_row_loads"] == 15 * 9


def test_output_and_input_without_routes():
    import neo

    # output 1 has no route, input 2 feeds nothing
    routes = [(0, 0), (0, 1), (2, 1), (3, 0), (3, 3)]
    p = neo.matrix_plan(4, 4, 64, 5, routes=routes, options={"out_tile": 1})
    assert [t["inputs"] for t in p["tiles"]] == [[0, 1], [], [1], [0, 3]]
    assert [t["rows"] for t in p["tiles"]] == [10, 0, 5, 10]
    assert all(c == 0 for c in p["tiles"][1]["cuts"])
    assert p["fdl_row_loads"] == 25 and p["filter_row_loads"] == 25
    p = neo.matrix_plan(4, 4, 64, 5, routes=routes, options={"out_tile": 4})
    assert [t["inputs"] for t in p["tiles"]] == [[0, 1, 3]]


@pytest.mark.parametrize("I,O,P,ot,wgs", [(4, 4, 5, 4, 3), (3, 5, 9, 4, 8), (4, 3, 70, 1, 39), (2, 2, 37, 2, 7),
                                          (1, 1, 3, 1, 64), (4, 4, 5, 2, 200)])
def test_split_cuts_cover_every_row_once(I, O, P, ot, wgs):
    import neo

    p = neo.matrix_plan(I, O, 64, P, options={"out_tile": ot, "split_workgroups": wgs})
    S = p["splits"]
    assert 1 <= S <= 64
    longest = max(t["rows"] for t in p["tiles"])
    for t in p["tiles"]:
        c = t["cuts"]
        assert len(c) == S + 1 and c[0] == 0 and c[-1] == t["rows"]
        assert all(a <= b for a, b in zip(c, c[1:]))
        seen = np.zeros(t["rows"], int)
        for a, b in zip(c, c[1:]):
            seen[a:b] += 1
        assert (seen == 1).all()
        per = -(-t["rows"] // S)  # equal row counts, the last split takes the rest
        assert all(b - a in (per, t["rows"] - a, 0) for a, b in zip(c, c[1:]))
        if t["rows"] == longest:
            assert all(b > a for a, b in zip(c, c[1:]))  # no empty split in the longest tile
    if wgs == 3:
        assert S == 3 and longest % S  # 20 rows in 3 splits: 7, 7, 6
        assert p["tiles"][0]["cuts"] == [0, 7, 14, 20]


def test_default_splits_follow_the_plain_step_rule():
    import neo

    # unfused: at least 8 rows per split; fused up to B = 512: 16
    p = neo.matrix_plan(4, 3, 512, 70, options={"out_tile": 1, "fused": 0})
    assert p["splits"] == 35 and not p["fused"]  # 280 rows per tile, 8 per split
    p = neo.matrix_plan(4, 3, 512, 70, options={"out_tile": 1, "fused": 1})
    assert p["splits"] == 18 and p["fused"]  # ceil(280 / 16) = 18 -> 16 rows per split
    assert neo.matrix_plan(1, 1, 16, 3)["splits"] == 1


def test_out_tile_is_clamped_by_block():
    import neo

    for B, want in [(16, 4), (512, 4), (1024, 2), (2048, 1), (4096, 1)]:
        assert neo.matrix_plan(2, 4, B, 3, options={"out_tile": 4})["out_tile"] == want
    assert neo.matrix_plan(2, 4, 1024, 3, options={"out_tile": 2})["out_tile"] == 2
    assert neo.matrix_plan(2, 4, 512, 3, options={"out_tile": 2})["out_tile"] == 2
    assert neo.matrix_plan(2, 4, 4096, 3, options={"out_tile": 2})["out_tile"] == 1


def test_automatic_out_tile():
    """4 where the sweep has it ahead (B = 512, every output of a tile fed by every input of the tile's
    union, at least 8 tiles and 2048 rows in the longest tile), else 1."""
    import neo

    banded = [(o, (o + k) % 64) for o in range(64) for k in range(8)]
    for I, O, B, P, routes, want in [(32, 32, 512, 64, None, 4), (32, 32, 512, 63, None, 1), (8, 32, 512, 256, None, 4),
                                     (8, 32, 512, 128, None, 1), (32, 32, 256, 128, None, 1), (32, 32, 1024, 128, None, 1),
                                     (64, 64, 512, 938, banded, 1), (2, 2, 512, 938, None, 1), (2, 2, 512, 1024, None, 1), (8, 28, 512, 256, None, 1),
                                     (32, 32, 512, 64, dense(32, 32)[1:], 1)]:
        p = neo.matrix_plan(I, O, B, P, routes=routes)
        assert p["out_tile"] == want, (I, O, B, P, p["out_tile"])
        assert p == neo.matrix_plan(I, O, B, P, routes=routes, options={"out_tile": want})


def test_host_validation_without_gpu():
    import neo

    lib = neo._native.load()
    E = neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 600

    def err():
        return lib.neo_hip_last_error()

    def plan(I, O, B, P, ro, ri, n=None, opts=None):
        ro, ri = np.asarray(ro, np.int32), np.asarray(ri, np.int32)
        info = neo._native.MatrixPlanInfo()
        o = neo._native.MatrixOpts(**opts) if opts else None
        return lib.neo_hip_matrix_plan(I, O, B, P, ro.ctypes.data_as(ctypes.c_void_p), ri.ctypes.data_as(ctypes.c_void_p),
                                       len(ro) if n is None else n, ctypes.byref(o) if o else None, ctypes.byref(info),
                                       None, None, None, None, None, None)

    assert plan(2, 2, 64, 3, [0, 1], [0, 1]) == 0
    assert plan(2, 2, 64, 3, [0, 0], [1, 1]) == E and b"duplicate route" in err()
    assert plan(2, 2, 64, 3, [0, 2], [0, 1]) == E and b"out of range" in err()
    assert plan(2, 2, 64, 3, [0, 1], [0, -1]) == E and b"out of range" in err()
    assert plan(2, 2, 64, 3, [0, 1], [0, 2]) == E and b"out of range" in err()
    assert plan(2, 2, 64, 3, [0], [0], n=0) == E and b"nroutes" in err()
    assert plan(2, 2, 500, 3, [0], [0]) == E and b"block" in err()
    assert plan(2, 2, 8, 3, [0], [0]) == E and b"block" in err()
    assert plan(2, 2, 8192, 3, [0], [0]) == E and b"block" in err()
    assert plan(0, 2, 64, 3, [0], [0]) == E and err()
    assert plan(2, 2, 64, 0, [0], [0]) == E and b"partitions" in err()
    assert plan(2, 2, 64, 3, [0], [0], opts={"fused": -1, "split_workgroups": 0, "out_tile": 3}) == E and b"out_tile" in err()
    assert lib.neo_hip_matrix_plan(2, 2, 64, 3, None, None, 1, None, None, None, None, None, None, None, None) == E and err()

    h = ctypes.c_void_p()
    assert lib.neo_hip_matrix_create(2, 2, 64, 3, 0, 2, None, ctypes.byref(h)) == E and b"method" in err()
    assert lib.neo_hip_matrix_create(2, 2, 64, 3, 0, -1, None, ctypes.byref(h)) == E and b"method" in err()
    assert lib.neo_hip_matrix_create(2, 2, 500, 3, 0, 0, None, ctypes.byref(h)) == E and b"block" in err()
    assert lib.neo_hip_matrix_create(2, 0, 64, 3, 0, 0, None, ctypes.byref(h)) == E and err()
    assert lib.neo_hip_matrix_create(2, 2, 64, 3, 0, 0, None, None) == E and err()
    assert not h.value
    assert lib.neo_hip_matrix_process(None, None, 0, None, 0, 1, 1, None) == E and err()
    assert lib.neo_hip_matrix_info(None, None) == E and err()
    assert lib.neo_hip_matrix_reset(None) == E and err()
    assert lib.neo_hip_matrix_destroy(None) == 0
    with pytest.raises(ValueError):
        neo.MatrixConvolver(2, 2, 64, 3, method="upola_v2")
    with pytest.raises(neo._native.NeoHipError):
        neo.matrix_plan(2, 2, 64, 3, routes=[(0, 0), (0, 0)])


def test_python_exports():
    import neo

    for name in ("MatrixConvolver", "matrix_plan", "matrix_convolve"):
        assert name in neo.__all__ and hasattr(neo, name) and name in neo.convolution.__all__


def test_matrix_plan_host_program_under_sanitizers():
    """csrc/matrix_plan.hpp alone (it includes no HIP header), in a program of its own built with the
    address and undefined-behaviour sanitizers: random route lists, the plan against a restatement
    and the step kernel's row walk replayed on the host (every (route, partition) met exactly once,
    every index in range, the loads equal to the plan's totals); exit status 0."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    os.makedirs(os.path.join(CPP, "bin"), exist_ok=True)
    out = os.path.join(CPP, "bin", "matrix_plan_main")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", out,
                           os.path.join(CPP, "matrix_plan_main.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "300 cases, 0 failed" in r.stdout
