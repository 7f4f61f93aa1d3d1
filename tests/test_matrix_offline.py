"""Offline windows of the matrix convolver, the part that needs no GPU: neo_hip_matrix_offline_plan
on hand-checked cases (the function the pass takes its rows from), a float64 replay of the ring and
pair arithmetic with the plan's own rows against the direct block-axis convolution, the spill check
of the new kernels and the new symbols ("Offline windows")."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("neo_hip_matrix_set_offline", "neo_hip_matrix_offline_info", "neo_hip_matrix_offline_plan")
FT, FN = 128, 256


def test_plan_of_the_long_dense_matrix():
    import neo

    p = neo.matrix_offline_plan(32, 32, 512, 938)
    assert p["segments"] == 8 and p["windows"] == 2 and p["blocks_per_pass"] == 256
    assert p["min_ring_rows"] == p["ring_rows"] == 1281 and p["pairs"] == 9
    assert p["hf_bytes"] == 1024 * 8 * 256 * 512 * 8
    assert p["xf_bytes"] == 32 * 9 * 256 * 512 * 8
    # pair k starts 128 k rows before the write position (mod ring); window 1 takes pair q, window 0 pair q + 1
    assert p["pair_rows"] == [(-128 * k) % 1281 for k in range(9)]
    assert p["pair_of"] == [list(range(1, 9)), list(range(8))]
    assert p["spectrum_rows"] == 1024 * 8 * 256 and p["pair_cache_rows"] == 1024 * 9 * 256
    assert p["fdl_rows"] == p["pair_rows_written"] == 32 * 9 * 256 and p["output_rows"] == 32 * 256 * 2
    rows = p["spectrum_rows"] + p["pair_cache_rows"] + p["fdl_rows"] + p["pair_rows_written"] + p["output_rows"]
    assert p["bytes"] == 8 * 512 * rows + 4 * 512 * 256 * 64
    assert p["cache_bytes"] == 8 * 512 * p["pair_cache_rows"]


def test_segments_windows_and_the_ring():
    import neo

    assert [neo.matrix_offline_plan(2, 2, 64, P)["segments"] for P in (3, 128, 129)] == [1, 1, 2]
    one = neo.matrix_offline_plan(2, 3, 64, 300, windows=1, write_pos=70, ring_rows=700)
    assert one["segments"] == 3 and one["pairs"] == 3 and one["blocks_per_pass"] == 128 and one["windows"] == 1
    assert one["min_ring_rows"] == 641 and one["ring_rows"] == 700
    assert one["pair_rows"] == [(70 - 128 * (k + 1)) % 700 for k in range(3)] and one["pair_of"] == [[0, 1, 2]]
    two = neo.matrix_offline_plan(2, 3, 64, 300, routes=[(0, 0), (2, 1)], windows=2, write_pos=70, ring_rows=700)
    assert two["pairs"] == 4 and two["pair_rows"] == [(70 - 128 * k) % 700 for k in range(4)]
    assert two["hf_bytes"] == 2 * 3 * 256 * 64 * 8 and two["xf_bytes"] == 2 * 4 * 256 * 64 * 8
    assert neo.matrix_offline_plan(2, 3, 64, 300, windows=0) == neo.matrix_offline_plan(2, 3, 64, 300, windows=2)


def test_plan_refuses_bad_arguments():
    import neo

    for bad in ({"windows": 3}, {"windows": -1}, {"ring_rows": 640}, {"write_pos": -1}, {"write_pos": 641},
                {"ring_rows": 700, "write_pos": 700}):
        with pytest.raises(neo._native.NeoHipError):
            neo.matrix_offline_plan(2, 2, 64, 300, **bad)
    for shape in ((0, 2, 64, 3), (2, 2, 48, 3), (2, 2, 64, 0)):
        with pytest.raises(neo._native.NeoHipError):
            neo.matrix_offline_plan(*shape)
    with pytest.raises(neo._native.NeoHipError):
        neo.matrix_offline_plan(2, 2, 64, 3, routes=[(0, 0), (0, 0)])
    with pytest.raises(neo._native.NeoHipError):  # a ring of 2 GiB per input
        neo.matrix_offline_plan(1, 1, 4096, 65300)
    assert neo.matrix_offline_plan(1, 1, 4096, 65000)["ring_rows"] == 65281
    lib = neo._native.load()
    E = neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_matrix_set_offline(None, 1, 0) == E and lib.neo_hip_last_error()
    assert lib.neo_hip_matrix_offline_info(None, None, None, None, None) == E
    one = np.zeros(1, np.int32)
    ptr = one.ctypes.data_as(ctypes.c_void_p)
    # every output is optional
    assert lib.neo_hip_matrix_offline_plan(1, 1, 64, 3, ptr, ptr, 1, 0, 0, 0, None, None, None) == 0


def _replay(neo, I, O, routes, H, X, hist, ring, WP, shift_pair=None):
    """The passes of one bin with the plan's rows. H[(o, i)] [P], X [I][blocks]; `hist` blocks are in
    the ring before the first pass (row t mod ring holds block t). -> Y [O][blocks after hist]."""
    P = len(next(iter(H.values())))
    nseg = -(-P // FT)
    HF = {}
    for r, h in H.items():
        seg = np.zeros((nseg, FN), complex)
        for q in range(nseg):
            part = h[q * FT:(q + 1) * FT]
            seg[q, :len(part)] = part
        HF[r] = np.fft.fft(seg, axis=1)
    rings = np.zeros((I, ring), complex)
    for t in range(hist):
        rings[:, t % ring] = X[:, t]
    out = []
    t, w = hist, hist % ring
    T = FT * WP
    while t + T <= X.shape[1]:
        p = neo.matrix_offline_plan(I, O, 16, P, routes=routes, windows=WP, write_pos=w, ring_rows=ring)
        assert p["blocks_per_pass"] == T and p["pairs"] == nseg + WP - 1
        written = {(w + j) % ring for j in range(T)}
        for j in range(T):
            rings[:, (w + j) % ring] = X[:, t + j]
        rows = [[(r0 + r) % ring for r in range(FN)] for r0 in p["pair_rows"]]
        if shift_pair is not None:
            rows[shift_pair] = [(r + 1) % ring for r in rows[shift_pair]]
        read = {r for k in rows for r in k}
        # a pass writes its own blocks' rows and may read them, but never overwrites a row of older
        # blocks that it still reads: the rows it reads beyond the ones it wrote hold blocks t - 128 nseg .. t - 1
        older = {(w - d) % ring for d in range(1, FT * nseg + 1)}
        if shift_pair is None:
            assert read - written <= older and not (older & written), "a pass overwrote a row it reads"
        XF = np.fft.fft(rings[:, rows], axis=2)  # [I][pairs][256]
        y = np.zeros((O, T), complex)
        for win in range(WP):
            acc = np.zeros((O, FN), complex)
            for o in range(O):
                for i in range(I):  # ascending input order
                    if (o, i) in HF:
                        for q in range(nseg):
                            acc[o] += XF[i, p["pair_of"][win][q]] * HF[(o, i)][q]
            y[:, win * FT:(win + 1) * FT] = np.fft.ifft(acc, axis=1)[:, FT:]
        out.append(y)
        w = (w + T) % ring
        t += T
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("WP", [1, 2])
@pytest.mark.parametrize("P", [3, 130, 300])
def test_replay_of_the_plans_rows_matches_the_direct_sum(P, WP):
    """Sum over q of IDFT256(DFT256(pair) . DFT256(h_q))[128 + j], with the pair rows and the (window,
    segment) -> pair map taken from neo_hip_matrix_offline_plan, against the direct block-axis
    convolution Y_o[t] = sum over routes (o, i), p < P of H[p] X_i[t - p], in float64 at 1e-12 of
    the peak: a 2 x 3 route list with one route missing, history in the ring before the first pass,
    five consecutive passes on the least ring (it wraps). Shifting one pair by a row must fail."""
    import neo

    I, O = 2, 3
    routes = [(o, i) for o in range(O) for i in range(I) if (o, i) != (1, 0)]
    rng = np.random.default_rng(100 * P + WP)
    H = {r: rng.standard_normal(P) + 1j * rng.standard_normal(P) for r in routes}
    ring = neo.matrix_offline_plan(I, O, 16, P, routes=routes)["min_ring_rows"]
    hist, nb = ring - 200, 5 * FT * WP
    assert hist + nb > ring + FT * WP  # the write position wraps, and a pass follows the wrap
    X = rng.standard_normal((I, hist + nb)) + 1j * rng.standard_normal((I, hist + nb))
    Y = np.zeros((O, hist + nb), complex)
    for (o, i), h in H.items():
        Y[o] += np.convolve(X[i], h)[:hist + nb]
    got = _replay(neo, I, O, routes, H, X, hist, ring, WP)
    assert got.shape == (O, nb)
    err = np.abs(got - Y[:, hist:]).max() / np.abs(Y).max()
    assert err <= 1e-12, err
    nseg = -(-P // FT)
    bad = _replay(neo, I, O, routes, H, X, hist, ring, WP, shift_pair=nseg + WP - 2)
    assert np.abs(bad - Y[:, hist:]).max() / np.abs(Y).max() > 1e-3, "a shifted pair went unnoticed"


def _kernels():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import spill_check
    finally:
        sys.path.pop(0)
    return spill_check.kernels(os.path.join(REPO, "neo-dsp_amd", "lib", "libneo_hip.so"))


def test_offline_kernels_do_not_spill():
    """k_matrix_off_fwd and both instantiations of k_matrix_off_mac in the built library: no spilled
    VGPR or SGPR, no scratch, at most 256 VGPRs (tools/spill_check.py; no GPU)."""
    mine = {n: v for n, v in _kernels().items() if "k_matrix_off_" in n}
    names = sorted(re.search(r"k_matrix_off_(fwd|macILi\dE)", n).group(1) for n in mine)
    assert names == ["fwd", "macILi1E", "macILi2E"], sorted(mine)
    bad = {n: v for n, v in mine.items() if v["vgpr_spill"] or v["sgpr_spill"] or v["scratch"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 256 for v in mine.values()), mine


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
    assert hasattr(neo, "matrix_offline_plan") and "matrix_offline_plan" in neo.__all__
    assert "matrix_offline_plan" in neo.convolution.__all__
    assert hasattr(neo.MatrixConvolver, "set_offline") and hasattr(neo.MatrixConvolver, "offline_info")
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 800
    assert int(re.search(r"#define NEO_HIP_VERSION (\d+)", hdr).group(1)) >= 800
    assert "0.8.0" in hdr and "Inf / NaN" in hdr
    cpp = open(os.path.join(REPO, "include", "neo", "convolution.hpp")).read()
    assert "auto offline(bool on, int windows_per_pass = 0)" in cpp and "offline_info()" in cpp
    assert inspect.signature(neo.matrix_convolve).parameters["offline"].default is False
    assert inspect.signature(neo.MatrixConvolver.set_offline).parameters["windows_per_pass"].default == 0
