"""The offline windows of the double-precision UPOLS / UPOLA convolvers without a GPU: the window plan
and the row-source rule of csrc/upols_f64_plan.hpp (through tests/cpp/upols_f64_offline_plan_main.cpp,
built with the address and undefined-behaviour sanitizers) against rules stated here and in
tests/upols_f64_offline_replay.py; the float64 numpy replay of the pass against tests/upols_f64_truth.py
within 1e-13 of the peak at the GPU tests' shapes, so that the 1e-12 bar of
tests/test_upols_f64_offline_gpu.py tests the kernels and not the rule; and the new C ABI calls'
argument checks before any device call."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import upols_f64_offline_replay as R
import upols_f64_truth as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")


@pytest.fixture(scope="module")
def plan_program():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "f64_offline.mk", "bin/upols_f64_offline_plan_main"])
    exe = os.path.join(CPP, "bin", "upols_f64_offline_plan_main")

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = [json.loads(x) for x in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    return run


GRID = [(C, B, P, m) for C in (1, 3, 256, 2000) for B in (16, 256, 512, 4096) for P in (1, 3, 127, 128, 129, 257, 938, 3750)
        for m in (0, 1)]


def test_offline_plan_rules(plan_program):
    out = plan_program([f"offline {C} {B} {P} {m}" for C, B, P, m in GRID])
    for (C, B, P, m), got in zip(GRID, out):
        assert (got["W"], got["F"]) == (128, 256)
        nseg = got["nseg"]
        assert nseg == -(-P // 128) and 128 * (nseg - 1) < P <= 128 * nseg, (C, B, P, got)
        row = 16 * C * B
        assert got["spectra_bytes"] == 16 * C * nseg * 256 * B
        assert got["scratch_bytes"] == got["y_bytes"] == 128 * row
        assert got["tail_bytes"] == (8 * C * 128 * B if m else 0)
        assert got["extra_bytes"] == got["scratch_bytes"] + got["y_bytes"] + got["tail_bytes"]
        # the model: scratch written; the pair rows that are not zero; 256 nseg spectrum rows; Y written
        # and read; the commit read and written; the samples of a batched pass of 128 blocks
        loaded = 128 + min(128 * nseg, P - 1)
        assert got["pass_bytes"] == (row * (128 + loaded + 256 * nseg + 256 + 2 * min(128, P)) +
                                     8 * C * B * (128 * (6 if m else 3) + 1)), (C, B, P, m, got)
        want = R.plan_rule(C, B, P, bool(m))
        assert {k: got[k] for k in want} == want
        # the ring is what it was: exactly P rows
        assert got["filter_bytes"] == got["fdl_bytes"] == 16 * C * P * B
    # the C5 shard: a window pass moves about a quarter of what eight batched passes of 16 blocks move
    c5 = plan_program(["offline 256 512 938 0"])[0]
    assert c5["nseg"] == 8 and 55e6 < c5["pass_bytes"] / 128 < 70e6
    assert plan_program(["offline 2 4096 40000 1"])[0]["spectra_bytes"] > 2 ** 32


def test_offline_plan_refusals(plan_program):
    out = plan_program(["offline 1 24 3 0", "offline 0 64 3 0", "offline 1 64 0 0", "offline 1 64 3 2", "offline 1 64 1 1"])
    assert [o.get("refused") for o in out] == [
        "block must be a power of two in [16, 4096], got 24",
        "channels must be >= 1",
        "partitions must be >= 1",
        "method must be 0 (upols) or 1 (upola)",
        None,
    ]


@pytest.mark.parametrize("P", [1, 2, 127, 128, 129, 300])
def test_row_sources_equal_the_definition(plan_program, P):
    """Every w < P and every e in [-128 (nseg + 1), 127]: exactly the rows e <= -P are zero, every ring
    row lies in [0, P) and is (w + e) mod P, the scratch rows are e; the rows a pass commits are the
    last min(128, P) blocks' and distinct."""
    nseg = R.segments(P)
    first = -128 * (nseg + 1)
    got = plan_program([f"src {P} {w}" for w in range(P)])
    for w, g in enumerate(got):
        assert g["first"] == first and len(g["rows"]) == 128 - first
        for e, (kind, row) in zip(range(first, 128), g["rows"]):
            assert (kind, row) == R.offline_src(e, w, P), (P, w, e)
            assert (kind == R.ZERO) == (e <= -P), (P, w, e)  # the definition once more, spelt out
            if kind == R.RING:
                assert -P < e < 0 and 0 <= row < P and row == (w + e) % P, (P, w, e)
            elif kind == R.SCRATCH:
                assert row == e and 0 <= e < 128
            else:
                assert row == 0
        # the pairs of a pass reach back to e = -128 nseg: every row of the ring but the oldest, once
        ring = [row for e, (kind, row) in zip(range(first, 128), g["rows"]) if kind == R.RING and e >= -128 * nseg]
        assert len(ring) == len(set(ring)) == min(128 * nseg, P - 1)
    got = plan_program([f"commit {P} {w}" for w in range(P)])
    for w, g in enumerate(got):
        rows = g["rows"]
        k = min(128, P)
        assert rows[:128 - k] == [-1] * (128 - k), (P, w)
        last = rows[128 - k:]
        assert last == [(w + j) % P for j in range(128 - k, 128)] and len(set(last)) == k, (P, w)
        # after the pass the ring holds what 128 plain steps would have left
        ring = {}
        for j in range(128):
            ring[(w + j) % P] = j
        assert {r: j for j, r in enumerate(rows) if r >= 0} == ring


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb", R.VALUE_SHAPES)
def test_numpy_replay_of_the_window_is_the_algorithm(C, B, P, nb, method):
    """The GPU tests' shapes as whole windows on a replayed handle of a ring of exactly P rows,
    against blockwise within 1e-13."""
    ir, H, x = T.problem(C, B, P, nb)
    h = R.Replay(H, method)
    y = h.process(x)
    err = T.peak_err(y, T.truth(C, B, P, method, nb))
    print(f"{C} x {B} x {P}, {nb} blocks {method}: replay vs blockwise {err:.3g}")
    assert err <= T.TRUTH_AGREE, err
    assert h.w == nb % P and h.ring.shape[1] == P


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("P", [3, 129, 200])
def test_numpy_replay_mixes_windows_passes_and_steps(P, method):
    """5 plain steps (w = 5 mod P is not 0 and the ring wraps inside a pair), a call of 128 + 16 + 3 blocks
    (window, batched pass, three steps), then 256 blocks: against blockwise within 1e-13."""
    C, B = 2, 16
    calls = [(5, False), (128 + 16 + 3, True), (256, True)]
    nb = sum(k for k, _ in calls)
    ir, H, x = T.problem(C, B, P, nb)
    h = R.Replay(H, method)
    y = np.empty_like(x)
    o = 0
    for k, offline in calls:
        assert o == 0 or h.w == o % P
        y[:, o * B:(o + k) * B] = h.process(x[:, o * B:(o + k) * B], 16, offline=offline)
        o += k
    err = T.peak_err(y, T.truth(C, B, P, method, nb))
    print(f"P {P} {method}: mixed replay vs blockwise {err:.3g}")
    assert err <= T.TRUTH_AGREE, err


def test_c_abi_validation_without_a_device():
    import neo

    lib = neo._native.load()
    EINVAL = neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 1700
    for name in ("neo_hip_upols64_set_offline", "neo_hip_upols64_offline_info", "neo_hip_upols64_offline_plan"):
        assert name in neo._native.SIGNATURES and hasattr(lib, name)
    assert lib.neo_hip_upols64_set_offline(None, 1) == EINVAL
    assert lib.neo_hip_upols64_offline_info(None, None, None, None, None) == EINVAL
    t, g, sb, eb, pb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    refs = [ctypes.byref(v) for v in (t, g, sb, eb, pb)]
    assert lib.neo_hip_upols64_offline_plan(3, 24, 70, 0, *refs) == EINVAL
    assert lib.neo_hip_last_error().decode() == "block must be a power of two in [16, 4096], got 24"
    assert lib.neo_hip_upols64_offline_plan(0, 128, 70, 0, *refs) == EINVAL
    assert lib.neo_hip_upols64_offline_plan(3, 128, 0, 0, *refs) == EINVAL
    assert lib.neo_hip_upols64_offline_plan(3, 128, 70, 2, *refs) == EINVAL
    assert lib.neo_hip_upols64_offline_plan(3, 128, 200, 1, *refs) == 0
    want = R.plan_rule(3, 128, 200, True)
    assert (t.value, g.value, sb.value, eb.value, pb.value) == (128, 2, want["spectra_bytes"], want["extra_bytes"],
                                                                want["pass_bytes"])
    assert neo.upols64_offline_plan(3, 128, 200, "upola") == {"blocks_per_pass": 128, "segments": 2,
                                                              "spectra_bytes": want["spectra_bytes"],
                                                              "extra_bytes": want["extra_bytes"],
                                                              "pass_bytes": want["pass_bytes"]}
    assert neo.upols64_offline_plan(1, 16, 1)["extra_bytes"] == 2 * 16 * 16 * 128  # overlap-save: no tails
    assert lib.neo_hip_upols64_offline_plan(3, 128, 70, 0, None, None, None, None, None) == 0
    with pytest.raises(neo._native.NeoHipError):
        neo.upols64_offline_plan(3, 24, 70)
    with pytest.raises(ValueError):
        neo.upols64_offline_plan(3, 128, 70, method="upola_v2")
    with pytest.raises(ValueError):
        neo.dense_convolve(np.zeros((1, 64), np.float32), np.ones((1, 8), np.float32), 16, offline=True)
