"""The batched passes of the double-precision UPOLS / UPOLA convolvers without a GPU: the batch plan
and the two index rules of csrc/upols_f64_plan.hpp (through tests/cpp/upols_f64_batch_plan_main.cpp,
built with the address and undefined-behaviour sanitizers) against rules stated here; a float64 numpy
replay of the pass (tests/upols_f64_batch_replay.py) against tests/upols_f64_truth.py within 1e-13 of
the peak, so that the 1e-12 bar of tests/test_upols_f64_batch_gpu.py tests the kernels and not the
index rule; and the new C ABI calls' argument checks before any device call."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import upols_f64_batch_replay as R
import upols_f64_truth as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")


@pytest.fixture(scope="module")
def plan_program():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "f64_batch.mk", "bin/upols_f64_batch_plan_main"])
    exe = os.path.join(CPP, "bin", "upols_f64_batch_plan_main")

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = [json.loads(x) for x in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    return run


GRID = [(C, B, P, sw, blocks) for C in (1, 3, 16, 256, 2000) for B in (16, 256, 512, 4096)
        for P in (1, 3, 9, 15, 16, 17, 70, 188, 938, 3750) for sw in (0, 4, 12, 1024) for blocks in (0, 1, 8, 16)]


def test_batch_plan_rules(plan_program):
    out = plan_program([f"batch {C} {B} {P} 1 {sw} {blocks}" for C, B, P, sw, blocks in GRID])
    short = 0
    for (C, B, P, sw, blocks), got in zip(GRID, out):
        Tb = got["T"]
        assert Tb in (8, 16) and (blocks < 2 or Tb == blocks), (C, B, P, sw, blocks, got)
        S, rows = got["S"], got["rows"]
        assert (S, rows) == R.batch_rule(C, B, P, Tb, sw), (C, B, P, sw, blocks, got)
        # every split but the last has `rows` partitions, the last one the rest: 1..rows of them
        assert 1 <= S <= 64 and (S - 1) * rows < P <= S * rows, (C, B, P, sw, got)
        if not sw:
            assert rows >= min(Tb, P)  # the sliding window fills once per split
        short += P < S * rows
        row = 16 * B
        assert got["scratch_bytes"] == C * Tb * row
        assert got["slab_bytes"] == C * S * Tb * row
        assert got["tail_bytes"] == 8 * C * Tb * B  # overlap-add
        assert got["extra_bytes"] == got["scratch_bytes"] + got["slab_bytes"] + got["tail_bytes"]
        # the ring and the plain step's state are what they were
        assert got["filter_bytes"] == got["fdl_bytes"] == 16 * C * P * B
        assert got["state_bytes"] == 32 * C * P * B + 8 * C * B + 16 * C * T.float_rule(C, P, sw)[0] * B
        assert got["pass_bytes"] == (2 * 16 * C * P * B + C * Tb * row + C * S * Tb * row + 2 * C * S * Tb * row +
                                     2 * C * min(Tb, P) * row + 8 * C * B * (6 * Tb + 1))
    assert short > 50
    ols = plan_program(["batch 3 128 70 0 0 0", "batch 256 512 938 0 0 16", "batch 2 4096 40000 0 0 16"])
    assert ols[0]["tail_bytes"] == 0 and ols[0]["T"] in (8, 16)
    assert ols[0]["pass_bytes"] == (2 * 16 * 3 * 70 * 128 + 3 * ols[0]["T"] * 2048 * (1 + 3 * ols[0]["S"]) +
                                    2 * 3 * min(ols[0]["T"], 70) * 2048 + 8 * 3 * 128 * (3 * ols[0]["T"] + 1))
    assert (ols[1]["S"], ols[1]["rows"]) == (2, 469)
    assert ols[2]["pass_bytes"] > 2 ** 32
    # a pass of T blocks moves fewer bytes than T plain steps wherever the filter is longer than a pass
    assert ols[1]["pass_bytes"] * 8 < 16 * (32 * 256 * 938 * 512)
    # the shapes the GPU tests force: P = 70 in four splits, the last one short and p0 > 0
    assert R.batch_rule(1, 128, 70, 16, T.forced_split(1)) == R.batch_rule(3, 512, 70, 8, T.forced_split(3)) == (4, 18)


def test_batch_plan_refusals(plan_program):
    out = plan_program(["batch 1 24 3 0 0 0", "batch 0 64 3 0 0 0", "batch 1 64 3 0 0 4", "batch 1 64 3 0 0 32",
                        "batch 1 64 3 0 0 -1", "batch 1 64 3 0 0 8"])
    assert [o.get("refused") for o in out] == [
        "block must be a power of two in [16, 4096], got 24",
        "channels must be >= 1",
        "blocks per pass must be 0 (automatic), 8 or 16",
        "blocks per pass must be 0 (automatic), 8 or 16",
        "blocks per pass must be 0 (automatic), 8 or 16",
        None,
    ]


@pytest.mark.parametrize("Tb", [8, 16])
def test_index_rules_equal_the_definition(plan_program, Tb):
    """Over P in {1, 2, 3, T - 1, T, T + 1, 70}, every w and every p0: the source of each of the T rows
    a split's first window holds and of each row that enters later, and the rows a pass commits."""
    cases = [(P, w, p0) for P in (1, 2, 3, Tb - 1, Tb, Tb + 1, 70) for w in range(P) for p0 in range(P)]
    got = plan_program([f"window {Tb} {P} {w} {p0}" for P, w, p0 in cases])
    for (P, w, p0), g in zip(cases, got):
        want_first = [list(R.window_src(j - p0, w, P)) for j in range(Tb)]
        assert g["first"] == want_first, (P, w, p0)
        for j, (scratch, row) in enumerate(g["first"]):  # the definition once more, spelt out
            e = j - p0
            assert (scratch, row) == ((1, e) if e >= 0 else (0, (w + e) % P))
            assert 0 <= row < (Tb if scratch else P)
        # every row that enters later is a ring row, (w - p) mod P
        assert g["enter"] == [[0, (w - p) % P] for p in range(p0 + 1, P)], (P, w, p0)
    commits = [(P, w) for P in (1, 2, 3, Tb - 1, Tb, Tb + 1, 70) for w in range(P)]
    got = plan_program([f"commit {Tb} {P} {w}" for P, w in commits])
    for (P, w), g in zip(commits, got):
        rows = g["rows"]
        k = min(Tb, P)
        assert rows[:Tb - k] == [-1] * (Tb - k), (P, w)
        last = rows[Tb - k:]
        assert last == [(w + j) % P for j in range(Tb - k, Tb)] and len(set(last)) == k, (P, w)
        assert rows == [R.commit_row(j, Tb, P, w) for j in range(Tb)]
        # after the pass the ring holds what T plain steps would have left: block j in row (w + j) mod P,
        # a later block over an earlier one
        ring = {}
        for j in range(Tb):
            ring[(w + j) % P] = j
        assert {r: j for j, r in enumerate(rows) if r >= 0} == ring


@pytest.mark.parametrize("Tb", [8, 16])
@pytest.mark.parametrize("P", [1, 3, 9, 70])
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_numpy_replay_of_the_pass_is_the_algorithm(method, P, Tb):
    """(3 plain, T + 5 batched, 2 plain, 2T batched) blocks on one replayed handle, the MAC in splits
    of the forced rule (P = 70: 18, 18, 18, 16) and in one split, against blockwise within 1e-13."""
    C, B = 2, 16
    calls = R.sequence(Tb)
    nb = sum(k for k, _ in calls)
    ir, H, x = T.problem(C, B, P, nb)
    want = T.blockwise(x, H, method)
    for rows in sorted({R.batch_rule(C, B, P, Tb, T.forced_split(C))[1], P}):
        h = R.Replay(H, method)
        y = np.empty_like(x)
        o = 0
        for k, batched in calls:
            y[:, o * B:(o + k) * B] = h.process(x[:, o * B:(o + k) * B], Tb if batched else 1, rows)
            o += k
        err = T.peak_err(y, want)
        print(f"P {P} T {Tb} {method} rows {rows}: replay vs blockwise {err:.3g}")
        assert err <= T.TRUTH_AGREE, (rows, err)
        assert h.w == nb % P


def test_c_abi_validation_without_a_device():
    import neo

    lib = neo._native.load()
    EINVAL = neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_upols64_set_batch(None, 1) == EINVAL
    assert lib.neo_hip_upols64_batch_info(None, None, None, None) == EINVAL
    t, s, r, e, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    refs = [ctypes.byref(v) for v in (t, s, r, e, b)]
    assert lib.neo_hip_upols64_batch_plan(3, 24, 70, 0, 0, 0, *refs) == EINVAL
    assert lib.neo_hip_last_error().decode() == "block must be a power of two in [16, 4096], got 24"
    assert lib.neo_hip_upols64_batch_plan(3, 128, 70, 0, 0, 5, *refs) == EINVAL
    assert lib.neo_hip_upols64_batch_plan(3, 128, 70, 1, 0, 0, *refs) == 0
    Tb = t.value
    assert Tb in (8, 16)
    S, rows = R.batch_rule(3, 128, 70, Tb)
    extra = 16 * 3 * 128 * Tb * (1 + S) + 8 * 3 * 128 * Tb
    assert (s.value, r.value, e.value) == (S, rows, extra) and b.value > 2 * 16 * 3 * 70 * 128
    assert neo.upols64_batch_plan(3, 128, 70, "upola") == {"blocks_per_pass": Tb, "splits": S, "rows": rows,
                                                           "extra_bytes": extra, "pass_bytes": b.value}
    assert lib.neo_hip_upols64_batch_plan(3, 128, 70, 0, 12, 8, *refs) == 0
    assert (t.value, s.value, r.value) == (8, 4, 18)
    assert neo.upols64_batch_plan(3, 128, 70, split_workgroups=12, blocks=8)["rows"] == 18
    assert lib.neo_hip_upols64_batch_plan(3, 128, 70, 0, 0, 0, None, None, None, None, None) == 0
    with pytest.raises(neo._native.NeoHipError):
        neo.upols64_batch_plan(3, 24, 70)
    with pytest.raises(ValueError):
        neo.upols64_batch_plan(3, 128, 70, method="upola_v2")
    with pytest.raises(ValueError):
        neo.dense_convolve(np.zeros((1, 64), np.float32), np.ones((1, 8), np.float32), 16, batch=True)
