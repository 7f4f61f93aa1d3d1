"""Window levels of the matrix convolver, the part that needs no GPU: neo_hip_matrix_level_plan on
hand-checked cases (the function the handle is built from), a float64 replay of the schedule driven
by that plan (ring, parts at their steps, double-buffered slabs, priming) against the direct sum,
with mutations that the replay must catch, the new symbols, the stand-alone sanitizer program for the
plan and the kernel's walk, and the spill check of every new kernel instantiation."""
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
FOUR = (4, 8, 16, 32)  # the issue's list; the default became (8, 32) with the sweep
NEW_SYMBOLS = ("neo_hip_matrix_set_levels", "neo_hip_matrix_levels_info", "neo_hip_matrix_level_plan")


def bands(p):
    return [(lv["window"], lv["first"], lv["last"]) for lv in p["levels"]]


def test_head_and_bands_on_hand_checked_cases():
    import neo

    p = neo.matrix_level_plan(2, 2, 32, 70, windows=FOUR)
    assert p["head"] == 8 and bands(p) == [(4, 8, 16), (8, 16, 32), (16, 32, 64), (32, 64, 70)]
    assert p["ring_rows"] == 70 and p["chunks"] == 1
    p = neo.matrix_level_plan(1, 1, 16, 9, windows=FOUR)
    assert p["head"] == 8 and bands(p) == [(4, 8, 9)]
    assert p["levels"][0]["outputs"] == [[[(0, 8, 9)]]] and p["levels"][0]["part_cuts"] == [0, 0, 0, 0, 1]
    p = neo.matrix_level_plan(1, 1, 16, 8, windows=FOUR)
    assert p["levels"] == [] and p["head"] == 8 and p["partial_bytes"] == 0 and p["head_bank_bytes"] == 0
    assert neo.matrix_level_plan(1, 1, 16, 3, windows=FOUR)["levels"] == []
    p = neo.matrix_level_plan(2, 2, 32, 70, windows=(32,))
    assert p["head"] == 64 and bands(p) == [(32, 64, 70)]
    p = neo.matrix_level_plan(3, 5, 128, 37, windows=FOUR)
    assert bands(p) == [(4, 8, 16), (8, 16, 32), (16, 32, 37)]  # T = 32 dropped: its band is empty
    p = neo.matrix_level_plan(2, 2, 32, 70, windows=(8, 32))
    assert p["head"] == 16 and bands(p) == [(8, 16, 64), (32, 64, 70)]
    assert neo.matrix_level_plan(2, 2, 32, 70) == p  # the default list
    assert neo.matrix_level_plan(2, 2, 32, 16)["levels"] == [] and bands(neo.matrix_level_plan(2, 2, 32, 17)) == [(8, 16, 17)]
    p = neo.matrix_level_plan(2, 2, 32, 40, windows=(2, 32))  # the last level dropped: the one before runs to P
    assert p["head"] == 4 and bands(p) == [(2, 4, 40)]
    # the filter rows per route and block of the issue's example: 8 + 2 + 2 + 2 + 6 of 256
    p = neo.matrix_level_plan(32, 32, 512, 256, windows=FOUR)
    per = [lv["filter_rows"] // (32 * 32) / lv["window"] for lv in p["levels"]]
    assert p["head"] == 8 and per == [2, 2, 2, 6] and p["chunks"] == 2


def test_splits_parts_and_the_bytes_model_by_hand():
    import neo

    # 2 x 2, B = 64, P = 20, windows (4,): head 8, one level, band [8, 20): 12 partitions, 24 rows per
    # output. Automatic: 512 x 4 workgroups wanted over 2 outputs, but no split shorter than 4 rows: 6
    p = neo.matrix_level_plan(2, 2, 64, 20, windows=(4,))
    lv = p["levels"][0]
    assert lv["splits"] == 6 and lv["workgroups"] == 12 and lv["part_cuts"] == [0, 3, 6, 9, 12]
    assert lv["outputs"][0] == [[(0, 8, 12)], [(0, 12, 16)], [(0, 16, 20)], [(1, 8, 12)], [(1, 12, 16)], [(1, 16, 20)]]
    assert lv["outputs"][1] == lv["outputs"][0]
    assert lv["filter_rows"] == 4 * 12 and lv["fdl_rows"] == 12 * (4 + 3) and lv["runs"] == 12
    assert p["partial_bytes"] == 2 * 2 * 6 * 4 * 64 * 8 and p["head_bank_bytes"] == 4 * 8 * 64 * 8
    # the head: the ordinary plan of 8 partitions, unfused
    h = neo.matrix_plan(2, 2, 64, 8, options={"fused": 0})
    assert p["head_splits"] == h["splits"] and p["head_out_tile"] == h["out_tile"]
    assert p["head_filter_rows"] == 4 * 8 == h["filter_row_loads"] and p["head_fdl_rows"] == h["fdl_row_loads"] == 4 * 8
    # one block: head filter + FDL rows + its slabs written and read; the level's rows / 4 + 2 x 2 x 6
    # partial rows; block I/O
    want = 8 * 64 * (32 + 32 + 2 * 2 * h["splits"]) + 8 * 64 * (48 + 84) // 4 + 8 * 64 * 2 * 2 * 6 + 4 * 64 * 4
    assert p["bytes"] == want
    # an explicit target is per part and taken as given: 3 workgroups x 4 parts over 2 outputs: 6 splits;
    # 5 x 4 over 2: 10 splits, which cut inside an input (24 rows: 2.4 per split)
    assert neo.matrix_level_plan(2, 2, 64, 20, windows=(4,), split_workgroups=3)["levels"][0]["splits"] == 6
    q = neo.matrix_level_plan(2, 2, 64, 20, windows=(4,), split_workgroups=5)["levels"][0]
    assert q["splits"] == 10
    assert [sum(b - a for _, a, b in s) for s in q["outputs"][0]] == [2, 2, 3, 2, 3, 2, 2, 3, 2, 3]
    assert q["outputs"][0][4] == [(0, 17, 20)] and q["outputs"][0][5] == [(1, 8, 10)]
    # at most 64 splits, never more than rows; no level: the ordinary step's bytes
    assert neo.matrix_level_plan(2, 2, 64, 200, windows=(4,), split_workgroups=10 ** 6)["levels"][0]["splits"] == 64
    assert neo.matrix_level_plan(1, 1, 64, 10, windows=(4,), split_workgroups=10 ** 6)["levels"][0]["splits"] == 2
    assert neo.matrix_level_plan(2, 2, 64, 8, windows=FOUR)["bytes"] == neo.matrix_plan(2, 2, 64, 8)["bytes"]
    # bin chunks count as workgroups; parts with no workgroup at tiny shapes
    p = neo.matrix_level_plan(1, 2, 1024, 20, windows=FOUR)
    assert p["chunks"] == 4 and [lv["workgroups"] for lv in p["levels"]] == [2 * 2 * 4, 8]
    assert p["levels"][1]["splits"] == 1 and p["levels"][1]["part_cuts"] == list(range(9))
    assert neo.matrix_level_plan(1, 1, 16, 70, windows=FOUR)["levels"][3]["part_cuts"] == [0] * 32 + [1]


ROUTES = [(0, 0), (0, 1), (2, 1), (3, 0), (3, 3), (3, 2)]  # output 1 has none; output 3 takes three inputs


@pytest.mark.parametrize("I,O,B,P,windows,wgs", [(2, 2, 32, 70, FOUR, 0), (4, 4, 64, 37, FOUR, 0), (4, 4, 512, 100, None, 7),
                                                 (3, 5, 128, 9, FOUR, 0), (4, 4, 64, 131, (2, 4, 8, 16, 32), 3),
                                                 (4, 4, 64, 70, (32,), 1000)])
def test_every_partition_is_covered_once_and_the_parts_cover_every_workgroup(I, O, B, P, windows, wgs):
    import neo

    routes = ROUTES if (I, O) == (4, 4) else None
    rt = routes or [(o, i) for o in range(O) for i in range(I)]
    p = neo.matrix_level_plan(I, O, B, P, routes=routes, windows=windows, split_workgroups=wgs)
    seen = {r: np.zeros(P, int) for r in rt}
    for r in rt:
        seen[r][:p["head"]] += 1
    last = p["head"]
    for lv in p["levels"]:
        T, S = lv["window"], lv["splits"]
        assert lv["first"] == last >= 2 * T and lv["last"] > lv["first"]
        last = lv["last"]
        assert 1 <= S <= 64 and lv["workgroups"] == O * S * p["chunks"]
        cuts = lv["part_cuts"]
        assert len(cuts) == T + 1 and cuts[0] == 0 and cuts[-1] == lv["workgroups"]
        sizes = np.diff(cuts)
        assert (sizes >= 0).all() and sizes.max() - sizes.min() <= 1
        total = 0
        for o, out in enumerate(lv["outputs"]):
            order = []
            assert len(out) == S
            for s in out:
                for i, a, b in s:
                    assert lv["first"] <= a < b <= lv["last"]
                    seen[(o, i)][a:b] += 1  # a KeyError: an input the output has no route from
                    order.append((i, a))
                    total += b - a + T - 1
            assert order == sorted(order)
            if not any(oo == o for oo, _ in rt):
                assert out == [[] for _ in range(S)]  # an output without routes has no run in any level
        assert lv["fdl_rows"] == total and lv["filter_rows"] == len(rt) * (lv["last"] - lv["first"])
    assert last == P
    assert all((v == 1).all() for v in seen.values())
    # a shuffled route list gives the same plan
    rng = np.random.default_rng(3)
    shuffled = [rt[k] for k in rng.permutation(len(rt))]
    assert neo.matrix_level_plan(I, O, B, P, routes=shuffled, windows=windows, split_workgroups=wgs) == p


def test_plan_refuses_bad_windows_and_arguments():
    import neo

    for bad in ((3,), (1,), (64,), (4, 4), (8, 4), (4, 6), (0,), (), (2, 4, 8, 16, 32, 32)):
        with pytest.raises(neo._native.NeoHipError):
            neo.matrix_level_plan(2, 2, 64, 40, windows=bad)
    with pytest.raises(neo._native.NeoHipError):
        neo.matrix_level_plan(2, 2, 64, 40, split_workgroups=-1)
    with pytest.raises(neo._native.NeoHipError):
        neo.matrix_level_plan(2, 2, 64, 40, routes=[(0, 0), (0, 0)])
    lib = neo._native.load()
    E = neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_matrix_set_levels(None, 1, None, 0, 0) == E and lib.neo_hip_last_error()
    assert lib.neo_hip_matrix_levels_info(None, None) == E
    one = np.zeros(1, np.int32)
    ptr = one.ctypes.data_as(ctypes.c_void_p)
    # every output array is optional
    assert lib.neo_hip_matrix_level_plan(1, 1, 64, 40, ptr, ptr, 1, None, 0, 0, None, None, None, None, None, None) == 0


# -- the float64 replay ------------------------------------------------------------------------------

class Replay:
    """The schedule of upols_matrix.hip's level step on complex128 rows of NB bins, driven by the plan
    neo.matrix_level_plan returns: a ring of the plan's rows per input, per level two slab halves
    [O][S][T], the parts at their steps as ranges of workgroups (output, split, bin chunk), the finish
    summing the head and row n mod T of every level's current half, and priming when the slabs are
    stale. `order`: "after" runs a block's part after its row is written, as the handle does; "early"
    runs ALL parts of the next window ahead of the current window's first write, which the plan must
    survive as well: its bands need no row newer than the window before the current one, so a slab
    "may be computed at any step" of the window before its own."""

    def __init__(self, plan, I, O, P, rt, H, NB, order="after", ring_delta=0, band_shift=None, swap=False):
        self.p, self.I, self.O, self.P, self.rt, self.H, self.NB = plan, I, O, P, rt, H, NB
        self.R = plan["ring_rows"] + ring_delta
        self.G = plan["chunks"]
        self.order, self.swap = order, swap
        self.levels = [dict(lv) for lv in plan["levels"]]
        self.head = plan["head"]
        if band_shift is not None:  # level band_shift starts one partition early, what is before it ends there
            lv = self.levels[band_shift]
            f = lv["first"]
            lv["outputs"] = [[[(i, a - 1 if a == f else a, b) for i, a, b in s] for s in out] for out in lv["outputs"]]
            if band_shift == 0:
                self.head -= 1
            else:
                pv = self.levels[band_shift - 1]
                pv["outputs"] = [[[(i, a, b - 1 if b == f else b) for i, a, b in s if a < (b - 1 if b == f else b)]
                                  for s in out] for out in pv["outputs"]]
        self.route = {oi: r for r, oi in enumerate(rt)}
        self.reset()

    def reset(self):
        self.ring = np.zeros((self.I, self.R, self.NB), np.complex128)
        self.w, self.n, self.primed = 0, 0, True
        self.slab = [np.zeros((2, self.O, lv["splits"], lv["window"], self.NB), np.complex128) for lv in self.levels]

    def direct(self, upto):
        y = np.zeros((self.O, self.NB), np.complex128)
        for (o, i), r in self.route.items():
            for p in range(upto):
                y[o] += self.H[r, p] * self.ring[i, (self.w - p) % self.R]
        return y

    def mac(self, l, half, base, wg0, wg1):
        lv = self.levels[l]
        T, S = lv["window"], lv["splits"]
        for wg in range(wg0, wg1):
            os_, g = divmod(wg, self.G)
            o, s = divmod(os_, S)
            bins = slice(g * self.NB // self.G, (g + 1) * self.NB // self.G)
            acc = np.zeros((T, self.NB), np.complex128)
            for i, a, b in lv["outputs"][o][s]:
                r = self.route[(o, i)]
                for p in range(a, b):
                    for j in range(T):
                        acc[j] += self.H[r, p] * self.ring[i, (base + j - p) % self.R]
            self.slab[l][half, o, s, :, bins] = acc[:, bins]

    def parts(self):
        n, w = self.n, self.w  # the row block n is (or will be) written to
        for l, lv in enumerate(self.levels):
            T = lv["window"]
            k, W = n % T, n // T
            cur, nxt = W & 1, (W + 1) & 1
            cuts = lv["part_cuts"]
            if not self.primed:
                self.mac(l, cur, (w - k) % self.R, 0, cuts[-1])
            if self.order == "early":
                if k == 0 or not self.primed:
                    self.mac(l, nxt, (w + T - k) % self.R, 0, cuts[-1])
            else:
                self.mac(l, nxt, (w + T - k) % self.R, cuts[k] if self.primed else 0, cuts[k + 1])

    def step(self, x, levels=True):
        """one block: x [I][NB] -> y [O][NB]"""
        if levels and self.levels and self.order == "early":
            self.parts()
        self.ring[:, self.w] = x
        if levels and self.levels:
            if self.order == "after":
                self.parts()
            y = self.direct(self.head)
            for l, lv in enumerate(self.levels):
                T = lv["window"]
                k, W = self.n % T, self.n // T
                cur = (W & 1) if not self.swap else ((W + 1) & 1)  # swap: the finish reads the other half
                y += self.slab[l][cur, :, :, k].sum(axis=1)
            self.primed = True
        else:  # the plain step, a batched pass's block: time advances, the slabs go stale
            y = self.direct(self.P)
            self.primed = False
        self.w = (self.w + 1) % self.R
        self.n += 1
        return y


def problem(I, O, P, rt, NB, nb, seed):
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((len(rt), P, NB)) + 1j * rng.standard_normal((len(rt), P, NB))
    X = rng.standard_normal((nb, I, NB)) + 1j * rng.standard_normal((nb, I, NB))
    ref = np.zeros((nb, O, NB), np.complex128)
    for r, (o, i) in enumerate(rt):
        for p in range(P):
            ref[p:, o] += H[r, p] * X[:nb - p, i]
    return H, X, ref


def run(rp, X, on_from=0, off=()):
    """every block of X; levels on from block on_from, except the blocks in `off` (a batched pass)"""
    rp.reset()
    return np.stack([rp.step(X[n], levels=n >= on_from and n not in off) for n in range(len(X))])


def worst(y, ref):
    return float(np.abs(y - ref).max() / np.abs(ref).max())


REPLAYS = [
    # I, O, B (the plan's: bin chunks), P, routes, windows, split target, blocks
    (1, 1, 16, 9, None, FOUR, 0, 16),
    (2, 2, 32, 70, None, FOUR, 0, 110),           # all four levels, more than three windows of 32
    (2, 3, 512, 41, [(0, 0), (0, 1), (2, 1)], (2, 8), 5, 40),  # two bin chunks, forced splits, an output without routes
    (2, 2, 64, 67, None, (32,), 3, 100),
    (2, 1, 16, 70, None, None, 2, 100),          # the default list
]


@pytest.mark.parametrize("I,O,B,P,routes,windows,wgs,nb", REPLAYS)
def test_float64_replay_of_the_schedule(I, O, B, P, routes, windows, wgs, nb):
    import neo

    NB = 4
    rt = routes or [(o, i) for o in range(O) for i in range(I)]
    plan = neo.matrix_level_plan(I, O, B, P, routes=routes, windows=windows, split_workgroups=wgs)
    assert plan["levels"] and nb >= 3 * plan["levels"][-1]["window"]
    H, X, ref = problem(I, O, P, rt, NB, nb, 7)
    T0, TL = plan["levels"][0]["window"], plan["levels"][-1]["window"]
    mid = TL + TL // 2 + 1  # inside a window of every level
    cases = {"from block 0": dict(), "enabled mid-stream": dict(on_from=mid), "enabled at a window's last block": dict(on_from=2 * TL - 1),
             "a batched pass of 5 blocks": dict(off=range(mid, mid + 5)), "single plain steps": dict(off=(3, T0 + 1, 2 * TL, 2 * TL + 2))}
    for order in ("after", "early"):
        base = None
        for name, kw in cases.items():
            y = run(Replay(plan, I, O, P, rt, H, NB, order=order), X, **kw)
            assert worst(y, ref) < 1e-12, (order, name, worst(y, ref))
            base = y if base is None else base
    # the mutations, each of which the replay must catch (the same cases, the worst of them)
    def mutated(order, **mut):
        return max(worst(run(Replay(plan, I, O, P, rt, H, NB, order=order, **mut), X, **kw), ref) for kw in cases.values())

    # a ring one row short: priming after the block's write loses the oldest row of the slab rows to come
    assert mutated("after", ring_delta=-1) > 1e-3
    # the slab halves swapped
    assert mutated("after", swap=True) > 1e-3
    # a band that starts at 2 T - 1: slab row T - 1 of window W + 1 reads block W T, a row of the window
    # the slab is computed in
    for l in range(len(plan["levels"])):
        assert mutated("early", band_shift=l) > 1e-3, l
    # and a ring one row longer is as good
    assert mutated("after", ring_delta=1) < 1e-12


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
    assert hasattr(neo, "matrix_level_plan") and "matrix_level_plan" in neo.__all__
    assert "matrix_level_plan" in neo.convolution.__all__
    assert hasattr(neo.MatrixConvolver, "set_levels") and hasattr(neo.MatrixConvolver, "levels_info")
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 1000
    assert int(re.search(r"#define NEO_HIP_VERSION (\d+)", hdr).group(1)) >= 1000
    assert re.search(r"\* 0\.10\.0: window levels", hdr)
    cpp = open(os.path.join(REPO, "include", "neo", "convolution.hpp")).read()
    assert "auto levels(bool on, std::span<int const> windows = {}, int split_workgroups = 0)" in cpp and "levels_info()" in cpp
    # the structs the bindings mirror
    for name, cls in (("neo_hip_matrix_levels_desc", neo._native.MatrixLevelsDesc),
                      ("neo_hip_matrix_level_plan_info", neo._native.MatrixLevelPlanInfo)):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip().split("[")[0] for decl in body.split(";") if decl.strip()
                  for f in decl.strip().split(None, 1)[1].split(",")]
        assert fields == [n for n, _ in cls._fields_], name


def test_level_plan_host_program_under_sanitizers():
    """csrc/matrix_plan.hpp alone (it includes no HIP header), in a program of its own built with the
    address and undefined-behaviour sanitizers and run directly: random route lists and window lists,
    the level plan against a restatement, and k_matrix_lvl_mac's walk replayed part by part with row
    numbers; exit status 0."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    os.makedirs(BIN, exist_ok=True)
    out = os.path.join(BIN, "matrix_level_plan_main")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", out,
                           os.path.join(CPP, "matrix_level_plan_main.cpp")])
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


# DESIGN 5.8, "Window levels": VGPRs of k_matrix_lvl_mac per window length (the same for 64, 128 and 256 lanes)
LVL_MAC_VGPRS = {2: 22, 4: 48, 8: 96, 16: 116, 32: 210}


def test_new_kernels_do_not_spill():
    """Every instantiation of k_matrix_lvl_mac (lanes 64 / 128 / 256 x T = 2 .. 32) and of
    k_matrix_lvl_finish (9 block sizes x overlap-save / overlap-add) in the built library: no spilled
    VGPR or SGPR, no scratch (tools/spill_check.py; no GPU); the MAC within two waves per SIMD."""
    k = _kernels()
    mac = {n: v for n, v in k.items() if "k_matrix_lvl_mac" in n}
    fin = {n: v for n, v in k.items() if "k_matrix_lvl_finish" in n}
    inst = sorted(tuple(map(int, re.search(r"k_matrix_lvl_macILi(\d+)ELi(\d+)E", n).groups())) for n in mac)
    assert inst == sorted((L, T) for L in (64, 128, 256) for T in (2, 4, 8, 16, 32)), inst
    finst = sorted((int(a), int(b)) for a, b in (re.search(r"k_matrix_lvl_finishILi(\d+)ELb([01])E", n).groups() for n in fin))
    assert finst == sorted((B, o) for B in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096) for o in (0, 1)), finst
    bad = {n: v for n, v in {**mac, **fin}.items() if v["vgpr_spill"] or v["sgpr_spill"] or v["scratch"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 256 for v in mac.values()) and all(v["vgpr"] <= 128 for v in fin.values())
    for n, v in mac.items():
        T = int(re.search(r"k_matrix_lvl_macILi\d+ELi(\d+)E", n).group(1))
        assert v["vgpr"] == LVL_MAC_VGPRS[T], (n, v["vgpr"])
    # the names keep clear of the pinned kernels'
    assert not any("k_matrix_batch_mac" in n or "k_matrix_step" in n or "k_matrix_window" in n for n in {**mac, **fin})
