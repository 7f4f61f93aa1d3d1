"""Batched passes of the matrix convolver, the part that needs no GPU: neo_hip_matrix_batch_plan on
hand-checked cases (the function the handle is built from), the new symbols, the stand-alone
sanitizer program for the plan and the kernel's walk, and the spill check of every instantiation of
k_matrix_batch_mac together with the block step's register counts."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "bin")
NEW_SYMBOLS = ("neo_hip_matrix_set_batch", "neo_hip_matrix_batch_info", "neo_hip_matrix_batch_plan")


def runs(p):
    return [[s for s in o["splits"]] for o in p["outputs"]]


def test_dense_4x4_one_run_per_input_and_the_warm_up_rows():
    import neo

    p = neo.matrix_batch_plan(4, 4, 64, 5, blocks=32)
    assert p["blocks"] == 32 and p["splits"] == 1 and p["chunks"] == 1  # 20 rows per output: fewer than 32
    assert [o["rows"] for o in p["outputs"]] == [20] * 4
    for o in p["outputs"]:
        assert o["splits"] == [[(0, 0, 5), (1, 0, 5), (2, 0, 5), (3, 0, 5)]]
    assert p["runs"] == 16
    assert p["filter_row_loads"] == 16 * 5
    assert p["fdl_row_loads"] == 16 * (5 + 31)  # every run reloads its window of T - 1 rows
    assert p["slab_rows"] == 4 * 1 * 32
    assert p["bytes"] == 8 * 64 * (80 + 576 + 2 * 128) + 4 * 64 * 32 * 8
    # fewer blocks per pass: the same runs, a shorter window
    q = neo.matrix_batch_plan(4, 4, 64, 5, blocks=4)
    assert runs(q) == runs(p) and q["fdl_row_loads"] == 16 * (5 + 3) and q["slab_rows"] == 16
    # rows wider than 256 bins take several workgroups
    assert [neo.matrix_batch_plan(1, 1, B, 3)["chunks"] for B in (16, 256, 512, 1024, 4096)] == [1, 1, 2, 4, 16]


def test_lower_triangular_and_shuffled():
    import neo

    tri = [(o, i) for o in range(4) for i in range(o + 1)]
    p = neo.matrix_batch_plan(4, 4, 64, 5, routes=tri)
    assert [o["rows"] for o in p["outputs"]] == [5, 10, 15, 20]
    assert [o["splits"][0] for o in p["outputs"]] == [[(i, 0, 5) for i in range(o + 1)] for o in range(4)]
    assert p["filter_row_loads"] == 50 and p["fdl_row_loads"] == 10 * 36
    rng = np.random.default_rng(1)
    shuffled = [tri[k] for k in rng.permutation(len(tri))]
    assert neo.matrix_batch_plan(4, 4, 64, 5, routes=shuffled) == p


def test_output_without_routes_has_no_run():
    import neo

    routes = [(0, 0), (0, 1), (2, 1), (3, 0), (3, 3)]
    p = neo.matrix_batch_plan(4, 4, 64, 5, routes=routes, split_workgroups=8)
    assert p["splits"] == 2  # 8 workgroups over 4 outputs
    assert p["outputs"][1] == {"rows": 0, "splits": [[], []]}
    assert p["outputs"][0]["splits"] == [[(0, 0, 5)], [(1, 0, 5)]]
    assert p["outputs"][2]["splits"] == [[(1, 0, 2)], [(1, 2, 5)]]  # 5 rows: 2 + 3
    assert p["outputs"][3]["splits"] == [[(0, 0, 5)], [(3, 0, 5)]]


def test_forced_split_cuts_inside_an_input():
    import neo

    # 2 x 2, P = 37: 74 rows per output; 6 workgroups over 2 outputs: 3 splits of 24, 25, 25 rows
    p = neo.matrix_batch_plan(2, 2, 32, 37, split_workgroups=6)
    assert p["splits"] == 3
    for o in p["outputs"]:
        assert o["splits"] == [[(0, 0, 24)], [(0, 24, 37), (1, 0, 12)], [(1, 12, 37)]]
    assert p["fdl_row_loads"] == 2 * (74 + 4 * 31)
    # the automatic choice: at least 32 rows in every split of the longest output
    a = neo.matrix_batch_plan(2, 2, 32, 37)
    assert a["splits"] == 2 and a["outputs"][0]["splits"] == [[(0, 0, 37)], [(1, 0, 37)]]
    # a target is taken as given, up to 64 splits and never more than rows
    assert neo.matrix_batch_plan(1, 1, 64, 3, split_workgroups=1000)["splits"] == 3
    assert neo.matrix_batch_plan(2, 2, 64, 100, split_workgroups=100000)["splits"] == 64
    # bin chunks count as workgroups: B = 1024 has four per row
    assert neo.matrix_batch_plan(2, 2, 1024, 37, split_workgroups=24)["splits"] == 3
    # the automatic target: 512 workgroups
    assert neo.matrix_batch_plan(32, 32, 512, 32)["splits"] == 8      # 512 / (32 x 2)
    assert neo.matrix_batch_plan(2, 2, 512, 938)["splits"] == 58      # 1876 rows / 32, under 128
    assert neo.matrix_batch_plan(2, 2, 512, 8)["splits"] == 1


@pytest.mark.parametrize("I,O,P,wgs", [(4, 4, 5, 12), (3, 5, 9, 0), (4, 3, 70, 39), (2, 2, 37, 7), (1, 1, 3, 64),
                                       (4, 4, 5, 2000)])
def test_every_row_of_every_output_is_covered_once(I, O, P, wgs):
    import neo

    routes = [(o, i) for o in range(O) for i in range(I) if (o + 2 * i) % 3 != 1 or I == 1]
    p = neo.matrix_batch_plan(I, O, 64, P, routes=routes, split_workgroups=wgs)
    S = p["splits"]
    assert 1 <= S <= 64
    longest = max(o["rows"] for o in p["outputs"])
    total = 0
    for o, out in enumerate(p["outputs"]):
        ins = sorted(i for oo, i in routes if oo == o)
        assert out["rows"] == len(ins) * P and len(out["splits"]) == S
        seen = {i: np.zeros(P, int) for i in ins}
        order = []
        for s in out["splits"]:
            n = sum(b - a for _, a, b in s)
            assert n in (out["rows"] // S, out["rows"] // S + 1)  # equal row counts, to one row
            if out["rows"] == longest:
                assert n > 0  # no empty split in the longest output
            for i, a, b in s:
                assert 0 <= a < b <= P
                seen[i][a:b] += 1
                order.append((i, a))
                total += b - a + p["blocks"] - 1
        assert all((v == 1).all() for v in seen.values())
        assert order == sorted(order)  # inputs ascending, partitions ascending
    assert p["fdl_row_loads"] == total and p["filter_row_loads"] == len(routes) * P


def test_plan_refuses_bad_arguments():
    import neo

    for bad in ({"blocks": 1}, {"blocks": 3}, {"blocks": 64}, {"split_workgroups": -1}):
        with pytest.raises(neo._native.NeoHipError):
            neo.matrix_batch_plan(2, 2, 64, 3, **bad)
    with pytest.raises(neo._native.NeoHipError):
        neo.matrix_batch_plan(2, 2, 64, 3, routes=[(0, 0), (0, 0)])
    lib = neo._native.load()
    E = neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_matrix_set_batch(None, 1, 0) == E and lib.neo_hip_last_error()
    assert lib.neo_hip_matrix_batch_info(None, None, None, None) == E
    one = np.zeros(1, np.int32)
    ptr = one.ctypes.data_as(ctypes.c_void_p)
    # every output array is optional
    assert lib.neo_hip_matrix_batch_plan(1, 1, 64, 3, ptr, ptr, 1, 32, 0, None, None, None, None, None, None) == 0


def test_new_symbols_declared_exported_bound():
    import neo

    hdr = open(os.path.join(REPO, "include", "neo_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", neo._native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (neo_hip_\w+)", out))
    lib = neo._native.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"NEO_HIP_API\s+int\s+" + s + r"\s*\(", hdr), s
        assert s in exported and s in neo._native.SIGNATURES, s
        assert getattr(lib, s).argtypes is not None
    assert hasattr(neo, "matrix_batch_plan") and "matrix_batch_plan" in neo.__all__
    assert "matrix_batch_plan" in neo.convolution.__all__
    assert hasattr(neo.MatrixConvolver, "set_batch") and hasattr(neo.MatrixConvolver, "batch_info")
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 700
    assert int(re.search(r"#define NEO_HIP_VERSION (\d+)", hdr).group(1)) >= 700
    assert "do not apply to this handle type" in hdr and "Batching, streaming levels" not in hdr
    cpp = open(os.path.join(REPO, "include", "neo", "convolution.hpp")).read()
    assert "auto batch(bool on, int split_workgroups = 0)" in cpp and "batch_info()" in cpp
    import inspect

    assert inspect.signature(neo.matrix_convolve).parameters["batch"].default is False


def test_batch_plan_host_program_under_sanitizers():
    """csrc/matrix_plan.hpp alone (it includes no HIP header), in a program of its own built with the
    address and undefined-behaviour sanitizers and run directly: random route lists, the batch plan
    against a restatement, and k_matrix_batch_mac's walk replayed with row numbers; exit status 0."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    os.makedirs(BIN, exist_ok=True)
    out = os.path.join(BIN, "matrix_batch_plan_main")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", out,
                           os.path.join(CPP, "matrix_batch_plan_main.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "300 cases, 0 failed" in r.stdout


def _kernels():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import spill_check
    finally:
        sys.path.pop(0)
    return spill_check.kernels(os.path.join(REPO, "neo-dsp_amd", "lib", "libneo_hip.so"))


def test_matrix_batch_mac_does_not_spill():
    """Every instantiation of k_matrix_batch_mac (lanes 64 / 128 / 256 x T = 2 .. 32) in the built
    library: no spilled VGPR or SGPR, no scratch, at most 256 VGPRs (tools/spill_check.py; no GPU)."""
    mine = {n: v for n, v in _kernels().items() if "k_matrix_batch_mac" in n}
    inst = sorted(tuple(map(int, re.search(r"k_matrix_batch_macILi(\d+)ELi(\d+)E", n).groups())) for n in mine)
    assert inst == sorted((L, T) for L in (64, 128, 256) for T in (2, 4, 8, 16, 32)), inst
    bad = {n: v for n, v in mine.items() if v["vgpr_spill"] or v["sgpr_spill"] or v["scratch"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 256 for v in mine.values())  # two waves per SIMD


# DESIGN 5.8, "Registers and loads in flight": VGPRs per block size, the larger of the overlap-save
# and overlap-add forms
BLOCKS = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
WINDOW_VGPRS = (47, 47, 47, 54, 56, 56, 56, 56, 100)
STEP_VGPRS = {  # (out_tile, fused)
    (1, 0): (60, 60, 60, 60, 60, 64, 64, 62, 128),
    (1, 1): (58, 60, 60, 60, 60, 64, 64, 84, 158),
    (2, 0): (74, 74, 74, 76, 72, 74, 92),
    (2, 1): (74, 74, 74, 76, 72, 72, 92),
    (4, 0): (98, 98, 98, 106, 102, 82),
    (4, 1): (98, 98, 98, 106, 102, 82),
}


def test_block_step_registers_are_those_of_the_design_table():
    """The batched pass is a gear beside the block step, not a change to it: k_matrix_window and every
    k_matrix_step instantiation keep the VGPR counts of DESIGN 5.8's table and spill nothing."""
    k = _kernels()
    window, step = {}, {}
    for n, v in k.items():
        m = re.search(r"k_matrix_windowILi(\d+)ELb([01])E", n)
        if m:
            assert not (v["vgpr_spill"] or v["sgpr_spill"] or v["scratch"]), n
            window[int(m.group(1))] = max(window.get(int(m.group(1)), 0), v["vgpr"])
        m = re.search(r"k_matrix_stepILi(\d+)ELi(\d+)ELb([01])ELb([01])E", n)
        if m:
            assert not (v["vgpr_spill"] or v["sgpr_spill"] or v["scratch"]), n
            key = (int(m.group(1)), int(m.group(2)), int(m.group(3)))
            step[key] = max(step.get(key, 0), v["vgpr"])
    assert window == dict(zip(BLOCKS, WINDOW_VGPRS)), window
    want = {(B, ot, fu): n for (ot, fu), row in STEP_VGPRS.items() for B, n in zip(BLOCKS, row)}
    assert step == want, {key: (step.get(key), want.get(key)) for key in set(step) | set(want) if step.get(key) != want.get(key)}
