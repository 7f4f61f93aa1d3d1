"""Batched passes of the sparse convolvers, the part that needs no GPU: the window plan
(neo_hip_upols_sparse_window_plan: which FDL tiles the row entering a T-block pass at partition p is
needed for) against a brute-force numpy OR over the masks of tests/test_sparse_gpu.py; its argument
checks; the stand-alone sanitizer program for it; the new symbols; and the spill check of every
instantiation of k_sparse_batch_mac."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_sparse_gpu import masks

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "bin")
NEW_SYMBOLS = ("neo_hip_upols_sparse_window_plan", "neo_hip_upols_sparse_batch_info")


def window_numpy(tile_mask, window):
    """win[c][p] = OR of tile_mask[c][q] over q in [p, min(P, p + window)), one row at a time."""
    C, P, NW = tile_mask.shape
    win = np.zeros_like(tile_mask)
    for p in range(P):
        win[:, p] = np.bitwise_or.reduce(tile_mask[:, p:min(P, p + window)], axis=1)
    return win


def popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).sum())


@pytest.mark.parametrize("B", [16, 512, 1024, 4096])
@pytest.mark.parametrize("window", [2, 16, 32])
def test_window_plan_matches_brute_force(B, window):
    import neo

    C = 2
    for P in (window - 1, window, 2 * window + 5):
        for name, mask in masks(C, B, P).items():
            tm = neo.sparse_plan(mask, B)["tile_mask"]
            got = neo.sparse_window_plan(tm, B, window)
            want = window_numpy(tm, window)
            assert got["win_mask"].shape == (C, P, max(1, B // 512)) and got["win_mask"].dtype == np.uint32
            assert np.array_equal(got["win_mask"], want), (name, B, P, window)
            assert got["window_tiles"] == popcount(want), (name, B, P, window)
            # a window's tiles contain the row's own, and a wider window contains a narrower one
            assert np.array_equal(got["win_mask"] & tm, tm)
            if window > 2:
                half = neo.sparse_window_plan(tm, B, window // 2)
                assert np.array_equal(got["win_mask"] & half["win_mask"], half["win_mask"])
                assert half["window_tiles"] <= got["window_tiles"]


def test_window_plan_all_true_all_false_and_single_tiles():
    import neo

    C, B, P, W = 1, 512, 37, 16
    k = np.arange(B + 1)
    full = neo.sparse_plan(np.ones((C, P, B + 1), bool), B)["tile_mask"]
    got = neo.sparse_window_plan(full, B, W)
    assert got["window_tiles"] == C * P * (B // 16) and np.all(got["win_mask"] == 0xFFFFFFFF)
    none = neo.sparse_plan(np.zeros((C, P, B + 1), bool), B)["tile_mask"]
    got = neo.sparse_window_plan(none, B, W)
    assert got["window_tiles"] == 0 and not got["win_mask"].any()
    last = np.zeros((C, P, B + 1), bool)
    last[:, P - 1, B - 1] = True  # the last partition's last tile: seen by the W rows that end there
    got = neo.sparse_window_plan(neo.sparse_plan(last, B)["tile_mask"], B, W)
    assert got["window_tiles"] == W and np.all(got["win_mask"][0, P - W:, 0] == 1 << 31)
    assert not got["win_mask"][0, :P - W].any()
    first = np.broadcast_to((np.arange(P) == 0)[None, :, None] & (k >= 0)[None, None, :], (C, P, B + 1))
    got = neo.sparse_window_plan(neo.sparse_plan(first, B)["tile_mask"], B, W)
    assert got["window_tiles"] == B // 16 and not got["win_mask"][0, 1:].any()


def test_window_plan_refuses_bad_arguments():
    import neo

    lib = neo._native.load()
    E = neo._native.NEO_HIP_EINVAL
    tm = np.full((1, 4, 1), 5, np.uint32)
    wm = np.full((1, 4, 1), 9, np.uint32)
    wt = ctypes.c_int64(-3)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.neo_hip_upols_sparse_window_plan(None, 1, 512, 4, 2, p(wm), ctypes.byref(wt)) == E
    assert b"sparse_window_plan" in lib.neo_hip_last_error()
    assert lib.neo_hip_upols_sparse_window_plan(p(tm), 1, 512, 4, 2, None, ctypes.byref(wt)) == E
    for window in (0, 3, 64):
        assert lib.neo_hip_upols_sparse_window_plan(p(tm), 1, 512, 4, window, p(wm), ctypes.byref(wt)) == E
        assert b"window" in lib.neo_hip_last_error()
    assert np.all(wm == 9) and wt.value == -3  # a refused call writes nothing
    assert lib.neo_hip_upols_sparse_window_plan(p(tm), 1, 512, 4, 2, p(wm), None) == 0  # the count is optional
    assert np.all(wm == 5)
    assert lib.neo_hip_upols_sparse_batch_info(None, None, None, None) == E
    with pytest.raises(ValueError):
        neo.sparse_window_plan(np.zeros((1, 4, 2), np.uint32), 512, 2)  # NW = 1 at B = 512
    with pytest.raises(RuntimeError):
        neo.sparse_window_plan(tm, 512, 3)


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
    assert hasattr(neo, "sparse_window_plan") and "sparse_window_plan" in neo.__all__
    assert hasattr(neo.SparseUpolsConvolver, "sparse_batch_info")
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 500
    cpp = open(os.path.join(REPO, "include", "neo", "convolution.hpp")).read()
    assert "auto batch(bool on)" in cpp and "inline auto sparse_convolve(" in cpp


def test_window_plan_host_program_under_sanitizers():
    """csrc/sparse_plan.hpp alone (it includes no HIP header), in a program of its own built with
    the address and undefined-behaviour sanitizers and run directly; exit status 0."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    os.makedirs(BIN, exist_ok=True)
    out = os.path.join(BIN, "sparse_window_main")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", out,
                           os.path.join(CPP, "sparse_window_main.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "216 cases, 0 failed" in r.stdout


def test_sparse_batch_mac_does_not_spill():
    """Every instantiation of k_sparse_batch_mac (lanes 64 / 128 / 256 x T = 2 .. 32) in the built
    library: no spilled VGPR or SGPR, no scratch (tools/spill_check.py; no GPU)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import spill_check
    finally:
        sys.path.pop(0)
    k = spill_check.kernels(os.path.join(REPO, "neo-dsp_amd", "lib", "libneo_hip.so"))
    mine = {n: v for n, v in k.items() if "k_sparse_batch_mac" in n}
    inst = {tuple(map(int, re.search(r"k_sparse_batch_macILi(\d+)ELi(\d+)E", n).groups())) for n in mine}
    assert inst == {(L, T) for L in (64, 128, 256) for T in (2, 4, 8, 16, 32)}, sorted(inst)
    bad = {n: v for n, v in mine.items() if v["vgpr_spill"] or v["sgpr_spill"] or v["scratch"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 256 for v in mine.values())  # two waves per SIMD
    win = [v for n, v in k.items() if "k_sparse_win" in n]
    assert len(win) == 1 and not (win[0]["vgpr_spill"] or win[0]["scratch"])
