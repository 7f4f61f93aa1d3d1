"""The double-precision UPOLS / UPOLA convolvers without a GPU: the host-only plan header
(csrc/upols_f64_plan.hpp, through tests/cpp/upols_f64_plan_main.cpp), the C ABI's argument checks
before any device call, and the numpy truth of the GPU tests against itself (the two statements of
tests/upols_f64_truth.py agree within 1e-13 at every test shape, so the 1e-12 bar of
tests/test_upols_f64_gpu.py tests the kernels, not the reference)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import upols_f64_truth as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")


@pytest.fixture(scope="module")
def plan_program():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "f64.mk", "bin/upols_f64_plan_main"])
    exe = os.path.join(CPP, "bin", "upols_f64_plan_main")

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = [json.loads(x) for x in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    return run


GRID = [(C, P, sw) for C in (1, 2, 3, 16, 256, 1000, 2000) for P in (1, 3, 7, 8, 9, 17, 70, 188, 511, 512, 513, 938, 3750)
        for sw in (0, 1, 4, 12, 100, 1024, 5000)]


def test_split_rule_is_the_float_plain_steps(plan_program):
    out = plan_program([f"plan {C} 64 {P} 0 {sw}" for C, P, sw in GRID])
    short = 0
    for (C, P, sw), got in zip(GRID, out):
        S, rows = T.float_rule(C, P, sw)
        assert (got["S"], got["rows"]) == (S, rows), (C, P, sw, got)
        # every split but the last has `rows` partitions, the last one the rest: 1..rows of them
        assert 1 <= S <= 64 and (S - 1) * rows < P <= S * rows, (C, P, sw, got)
        short += P < S * rows
    assert short > 50  # the grid does reach shapes whose last split is the short one
    # the shapes the GPU tests force
    assert T.float_rule(1, 9, T.forced_split(1)) == (3, 3) and T.float_rule(3, 9, T.forced_split(3)) == (3, 3)
    assert T.float_rule(1, 70, T.forced_split(1)) == (4, 18) and T.float_rule(3, 70, T.forced_split(3)) == (4, 18)
    assert 70 - 3 * 18 == 16


def test_plan_agrees_with_the_float_planner(plan_program):
    """The same (S, rows) as csrc/upols_plan.hpp gives a float handle in its two-launch form
    (fused = 0), through that header's own host program."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "f64.mk", "bin/upols_f64_float_plan_main"])
    exe = os.path.join(CPP, "bin", "upols_f64_float_plan_main")
    grid = GRID
    lines = [f"dense 0 {C} 64 {P} 11 0 {sw} 0 0 0 -1 0 0 0 0 0" for C, P, sw in grid]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want = [json.loads(x) for x in r.stdout.splitlines()]
    got = plan_program([f"plan {C} 64 {P} 0 {sw}" for C, P, sw in grid])
    assert len(want) == len(got) == len(grid)
    for g, a, b in zip(grid, want, got):
        assert (a["S"], a["rows"]) == (b["S"], b["rows"]), (g, a, b)


def test_byte_counts(plan_program):
    cases = [(1, 16, 1, 0), (3, 128, 9, 12), (256, 512, 938, 0), (256, 256, 3750, 0), (1, 4096, 3, 0), (2, 4096, 40000, 0)]
    out = plan_program([f"plan {C} {B} {P} 1 {sw}" for C, B, P, sw in cases])
    for (C, B, P, sw), got in zip(cases, out):
        S, _ = T.float_rule(C, P, sw)
        assert got["ola"] == 1
        assert got["filter_bytes"] == got["fdl_bytes"] == 16 * C * P * B
        assert got["prev_bytes"] == 8 * C * B and got["slab_bytes"] == 16 * C * S * B
        assert got["state_bytes"] == 32 * C * P * B + 8 * C * B + 16 * C * S * B
        assert got["step_bytes"] == 32 * C * P * B + 32 * C * S * B + 32 * C * B
    assert out[-1]["filter_bytes"] > 2 ** 32  # 64-bit counts: a channel's ring may exceed 2 GiB


def test_every_refusal_text(plan_program):
    out = plan_program(["plan 0 64 3 0 0", "plan 1 24 3 0 0", "plan 1 8192 3 0 0", "plan 1 8 3 0 0", "plan 1 64 0 0 0",
                        "plan 1 64 3 2 0", "plan 1 64 3 -1 0", "plan 1 64 3 0 -1",
                        "io 64 100 128 128", "io 64 128 127 128", "io 64 128 128 126", "io 64 -64 128 128",
                        "io 64 128 129 130", "io 64 128 130 131", "io 64 128 130 132", "io 64 0 0 0"])
    assert [o.get("refused") for o in out] == [
        "channels must be >= 1",
        "block must be a power of two in [16, 4096], got 24",
        "block must be a power of two in [16, 4096], got 8192",
        "block must be a power of two in [16, 4096], got 8",
        "partitions must be >= 1",
        "method must be 0 (upols) or 1 (upola)",
        "method must be 0 (upols) or 1 (upola)",
        "invalid convolver options",
        "upols/upola convolvers take whole blocks (100 samples, block 64)",
        "num_samples must be in [0, ld]",
        "num_samples must be in [0, ld]",
        "num_samples must be in [0, ld]",
        "I/O must be 16-byte aligned (ld multiple of 2 doubles)",
        "I/O must be 16-byte aligned (ld multiple of 2 doubles)",
        None,
        None,
    ]


def test_c_abi_validation_without_a_device():
    import neo

    lib = neo._native.load()
    EINVAL = neo._native.NEO_HIP_EINVAL
    h = ctypes.c_void_p()

    def create(C, B, P, method=0, sw=0):
        rc = lib.neo_hip_upols64_create(C, B, P, 0, method, sw, ctypes.byref(h))
        return rc, lib.neo_hip_last_error().decode()

    assert create(1, 24, 3) == (EINVAL, "block must be a power of two in [16, 4096], got 24")
    assert create(1, 8192, 3) == (EINVAL, "block must be a power of two in [16, 4096], got 8192")
    assert create(0, 64, 3) == (EINVAL, "channels must be >= 1")
    assert create(1, 64, 0) == (EINVAL, "partitions must be >= 1")
    assert create(1, 64, 3, method=2) == (EINVAL, "method must be 0 (upols) or 1 (upola)")
    assert create(1, 64, 3, sw=-1) == (EINVAL, "invalid convolver options")
    assert h.value is None
    assert lib.neo_hip_upols64_create(1, 64, 3, 0, 0, 0, None) == EINVAL
    s, r, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    assert lib.neo_hip_upols64_plan(1, 24, 3, 0, ctypes.byref(s), ctypes.byref(r), ctypes.byref(b)) == EINVAL
    assert lib.neo_hip_upols64_plan(3, 128, 70, 12, ctypes.byref(s), ctypes.byref(r), ctypes.byref(b)) == 0
    assert (s.value, r.value, b.value) == (4, 18, 32 * 3 * 70 * 128 + 8 * 3 * 128 + 16 * 3 * 4 * 128)
    assert neo.upols64_plan(3, 128, 70, 12) == {"splits": 4, "rows": 18, "state_bytes": b.value}
    for f in (lib.neo_hip_upols64_reset, lib.neo_hip_upols64_info):
        assert f(*([None] * len(f.argtypes))) == EINVAL
    assert lib.neo_hip_upols64_set_filter(None, None, 0) == EINVAL
    assert lib.neo_hip_upols64_set_impulse(None, None, 4, 1, 0) == EINVAL
    assert lib.neo_hip_upols64_process_samples(None, None, 0, None, 0, 0, 0, None) == EINVAL
    assert lib.neo_hip_upols64_destroy(None) == 0
    x = np.zeros(64)
    p = x.ctypes.data_as(ctypes.c_void_p)
    assert lib.neo_hip_uniform_partition_f64(p, 1, 64, 24, p, 0, 0) == EINVAL
    assert b"got 24" in lib.neo_hip_last_error()
    assert lib.neo_hip_uniform_partition_f64(None, 1, 64, 16, p, 0, 0) == EINVAL
    assert lib.neo_hip_normalize_impulse_f64(None, 1, 64, 0, 0) == EINVAL
    with pytest.raises(TypeError):
        neo.uniform_partition(x, 16, dtype=np.int32)
    with pytest.raises(ValueError):
        neo.UpolsConvolver64(1, 64, 3, method="upola_v2")


@pytest.mark.parametrize("B,P", sorted({(B, P) for _, B, P in T.VALUE_SHAPES}) + [T.BIG_SHAPE[1:]])
def test_the_two_numpy_statements_agree(B, P):
    """blockwise (rfft / irfft, the algorithm) against np.convolve of the whole signal, overlap-save
    and overlap-add, three channels (one channel is channel 0 of these), within 1e-13 of the peak."""
    nb = T.BIG_BLOCKS if B == T.BIG_SHAPE[1] else None
    C = 1 if B == T.BIG_SHAPE[1] else 3
    ir, H, x = T.problem(C, B, P, nb)
    assert H.shape == (C, P, B + 1) and x.shape[1] == (nb or P + 5) * B and ir.shape[1] == P * B - 3
    want = T.truth(C, B, P, "", nb, statement="whole")
    for method in ("upols", "upola"):
        err = T.peak_err(T.truth(C, B, P, method, nb), want)
        print(f"B {B} P {P} {method}: blockwise vs np.convolve {err:.3g}")
        assert err <= T.TRUTH_AGREE, (B, P, method, err)
