"""The perceptual sparsity predicate (neo_hip_perceptual_*), the part that needs no GPU: the symbols
are declared, exported and bound; argument checks run before any device is touched; the weight
table, the host mask and the host histograms (csrc/perceptual_plan.hpp, the definition the kernels
reproduce) against a float64 numpy restatement (tests/perceptual_common.py); the density helpers;
the stand-alone sanitizer program for perceptual_plan.hpp; the host part of the C++ test."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import perceptual_common as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "bin")
SYMBOLS = ("neo_hip_perceptual_weights", "neo_hip_perceptual_mask_host", "neo_hip_perceptual_hist_host",
           "neo_hip_perceptual_mask", "neo_hip_perceptual_histogram", "neo_hip_upols_set_filter_perceptual",
           "neo_hip_upols_set_impulse_perceptual")
NAMES = ("a_weighting", "amplitude_to_db", "PerceptualSparsity", "perceptual_weights", "perceptual_mask",
         "perceptual_mask_host", "perceptual_histogram", "perceptual_histogram_host", "tile_density_curve",
         "threshold_for_tile_density")
_cache = {}


def build_cpp_test():
    """tests/cpp/test_perceptual.cpp against libneo_hip.so (flags as tests/cpp/Makefile)."""
    os.makedirs(BIN, exist_ok=True)
    out = os.path.join(BIN, "test_perceptual")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(REPO, "include"),
                           "-o", out, os.path.join(CPP, "test_perceptual.cpp"),
                           "-L" + os.path.join(REPO, "neo-dsp_amd", "lib"), "-lneo_hip",
                           "-Wl,-rpath," + os.path.join(REPO, "neo-dsp_amd", "lib")])
    return out


def spectra(C, B, P):
    key = (C, B, P)
    if key not in _cache:
        parts = pc.host_spectra(pc.impulse(C, B, P), B)
        parts.setflags(write=False)
        _cache[key] = parts
    return _cache[key]


def test_perceptual_symbols_declared_exported_bound():
    import neo

    hdr = open(os.path.join(REPO, "include", "neo_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", neo._native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (neo_hip_\w+)", out))
    lib = neo._native.load()
    for s in SYMBOLS:
        assert re.search(r"NEO_HIP_API\s+int\s+" + s + r"\s*\(", hdr), s
        assert s in exported, s
        assert s in neo._native.SIGNATURES, s
        assert getattr(lib, s).argtypes is not None
    for name in NAMES:
        assert hasattr(neo, name) and name in neo.__all__, name
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 400
    assert lib.neo_hip_version() == int(re.search(r"#define NEO_HIP_VERSION (\d+)", hdr).group(1))
    assert ctypes.sizeof(neo._native.Perceptual) == 24  # double, float, int, int (+ padding)


def test_argument_checks_without_device():
    import neo

    lib = neo._native.load()
    E = neo._native.NEO_HIP_EINVAL
    P = neo._native.Perceptual
    C, B, Pn = 1, 16, 2
    H = np.zeros((C, Pn, B + 1), np.complex64)
    m = np.zeros((C, Pn, B + 1), np.uint8)
    hb = np.zeros((C, 144), np.int64)
    ht = np.zeros((C, 144), np.int64)
    w = np.zeros(B + 1, np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = P(48000.0, -40.0, 0, 1)
    bad = [(P(0.0, -40.0, 0, 1), b"sample_rate"), (P(-1.0, -40.0, 0, 1), b"sample_rate"),
           (P(float("inf"), -40.0, 0, 1), b"sample_rate"), (P(float("nan"), -40.0, 0, 1), b"sample_rate"),
           (P(48000.0, float("nan"), 0, 1), b"threshold_db"), (P(48000.0, float("-inf"), 0, 1), b"threshold_db"),
           (P(48000.0, -40.0, -1, 1), b"low_bins_to_keep"), (P(48000.0, -40.0, B + 1, 1), b"low_bins_to_keep"),
           (P(48000.0, -40.0, 0, 2), b"weighting"), (P(48000.0, -40.0, 0, -1), b"weighting")]

    def calls(p, filt=vp(H), c=C, b=B, pn=Pn, mask=vp(m), bins=vp(hb), tiles=vp(ht)):
        r = ctypes.byref(p) if p is not None else None
        yield lib.neo_hip_perceptual_mask_host(filt, c, b, pn, r, mask)
        yield lib.neo_hip_perceptual_hist_host(filt, c, b, pn, r, bins, tiles)
        yield lib.neo_hip_perceptual_mask(filt, c, b, pn, r, mask, 0, 0)
        yield lib.neo_hip_perceptual_histogram(filt, c, b, pn, r, bins, tiles, 0, 0)

    for p, word in bad:
        assert lib.neo_hip_perceptual_weights(B, ctypes.byref(p), vp(w)) == E
        assert word in lib.neo_hip_last_error(), (word, lib.neo_hip_last_error())
        for rc in calls(p):
            assert rc == E
            assert word in lib.neo_hip_last_error(), (word, lib.neo_hip_last_error())
    for kw, word in (({"p": None}, b"null"), ({"filt": None}, b"null"), ({"mask": None, "bins": None}, b"null"),
                     ({"mask": None, "tiles": None}, b"null"), ({"c": 0}, b"channels"), ({"pn": 0}, b"partitions"),
                     ({"b": 24}, b"power of two"), ({"b": 8}, b"power of two"), ({"b": 8192}, b"power of two")):
        for rc in calls(**dict({"p": good}, **kw)):
            assert rc == E
            assert word in lib.neo_hip_last_error(), (kw, lib.neo_hip_last_error())
    assert lib.neo_hip_perceptual_weights(B, ctypes.byref(good), None) == E
    assert lib.neo_hip_perceptual_weights(B, None, vp(w)) == E
    assert lib.neo_hip_perceptual_weights(24, ctypes.byref(good), vp(w)) == E
    assert b"power of two" in lib.neo_hip_last_error()
    # the handle calls refuse a null handle before anything else
    ir = np.zeros((1, 32), np.float32)
    assert lib.neo_hip_upols_set_filter_perceptual(None, vp(H), ctypes.byref(good), 0) == E
    assert lib.neo_hip_upols_set_impulse_perceptual(None, vp(ir), 32, 1, ctypes.byref(good), 0) == E
    # the Python layer
    with pytest.raises(ValueError):
        neo.PerceptualSparsity(48000.0, -40.0, weighting="b")
    with pytest.raises(neo._native.NeoHipError, match="low_bins_to_keep"):
        neo.perceptual_weights(16, neo.PerceptualSparsity(48000.0, -40.0, 17))
    with pytest.raises(neo._native.NeoHipError, match="sample_rate"):
        neo.perceptual_mask_host(H, neo.PerceptualSparsity(0.0, -40.0))
    with pytest.raises(ValueError):
        neo.perceptual_mask_host(np.zeros((2, 3), np.complex64)[:, :1], neo.PerceptualSparsity(48000.0, -40.0))


@pytest.mark.parametrize("B", [16, 512, 4096])
@pytest.mark.parametrize("rate", [44100.0, 48000.0])
def test_weights_table(B, rate):
    """neo_hip_perceptual_weights against a float64 evaluation of the formula: 1e-4 dB absolute on
    finite entries (a double result rounded to float; float resolution at |w| <= 150 is 1.5e-5)."""
    import neo

    for low in (0, 2, B):
        got = neo.perceptual_weights(B, neo.PerceptualSparsity(rate, -40.0, low, "a"))
        want = pc.weights64(B, rate, low, "a")
        assert got.dtype == np.float32 and got.shape == (B + 1,)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin)
        assert np.abs(got[fin] - want[fin]).max() <= 1e-4
        assert np.all(got[:low] == 100.0)
        if low == 0:
            assert got[0] == -np.inf and np.all(np.isfinite(got[1:]))
        none = neo.perceptual_weights(B, neo.PerceptualSparsity(rate, -40.0, low, "none"))
        assert np.all(none[:low] == 100.0) and np.all(none[low:] == 0.0)
    # the table is the curve users know: 0 dB at 1 kHz, strongly negative at the bottom
    w = neo.perceptual_weights(B, neo.PerceptualSparsity(rate, -40.0, 0, "a"))
    k1k = int(round(1000.0 * 2 * B / rate))
    if k1k >= 1:
        assert abs(w[k1k] - pc.a_weighting64(k1k * rate / (2.0 * B))) <= 1e-4
    assert w[1] < w[B // 8]


def test_scalar_helpers():
    import neo

    assert abs(neo.a_weighting(1000.0)) <= 0.01
    assert neo.amplitude_to_db(1.0) == 0
    assert abs(neo.amplitude_to_db(10.0) - 20.0) <= 1e-12
    assert abs(neo.amplitude_to_db(np.float32(10.0)) - np.float32(20.0)) <= 4e-6
    assert neo.amplitude_to_db(0.0) == -144
    assert neo.amplitude_to_db(1e-9) == -144  # -180 dB: the floor
    assert neo.amplitude_to_db(-1.0) == -144
    assert neo.amplitude_to_db(1e-9, -200.0) == pytest.approx(-180.0)
    x32 = np.array([0.0, 1e-9, 0.5, 1.0, 10.0], np.float32)
    assert neo.amplitude_to_db(x32).dtype == np.float32 and neo.a_weighting(x32 * 1000).dtype == np.float32
    assert neo.amplitude_to_db(x32.astype(np.float64)).dtype == np.float64
    assert np.allclose(neo.amplitude_to_db(x32), [-144, -144, 20 * np.log10(0.5), 0, 20], atol=1e-5)
    f = np.array([10.0, 100.0, 1000.0, 10000.0])
    assert np.allclose(neo.a_weighting(f), pc.a_weighting64(f), atol=1e-9)
    assert np.allclose(neo.a_weighting(f.astype(np.float32)), pc.a_weighting64(f), atol=1e-3)
    assert neo.a_weighting(0.0) == -np.inf
    # the published curve: -19.1 dB at 100 Hz, -2.5 dB at 10 kHz
    assert abs(neo.a_weighting(100.0) + 19.1) < 0.1 and abs(neo.a_weighting(10000.0) + 2.5) < 0.1


@pytest.mark.parametrize("C,B,P", pc.SHAPES)
def test_host_mask_matches_float64(C, B, P):
    import neo

    parts = spectra(C, B, P)
    for weighting in pc.WEIGHTINGS:
        for low in pc.low_bins(B):
            lv, exact = pc.levels64(parts, pc.weights64(B, pc.SAMPLE_RATE, low, weighting))
            for theta in pc.THRESHOLDS:
                got = neo.perceptual_mask_host(parts, neo.PerceptualSparsity(pc.SAMPLE_RATE, theta, low, weighting))
                assert got.dtype == np.bool_ and got.shape == parts.shape
                pc.check_mask(got, lv, exact, theta, f"{(C, B, P)} {weighting} low={low} theta={theta}")
                if theta == -80.0 and weighting == "none":
                    assert got.all()  # below the floor of -72: every bin, zeros included
                if low == B:
                    assert got[:, :, :B].all()
    if C >= 2:  # the scale is per channel: the weak channel keeps as much as the strong one
        sp = neo.PerceptualSparsity(pc.SAMPLE_RATE, -40.0, 0, "none")
        got = neo.perceptual_mask_host(parts, sp)
        alone = neo.perceptual_mask_host(parts[1:2], sp)
        assert np.array_equal(got[1:2], alone) and 0 < got[1].sum() < got[1].size
    if (C, B, P) == (3, 128, 9):
        got = neo.perceptual_mask_host(parts, neo.PerceptualSparsity(pc.SAMPLE_RATE, -60.0, 0, "none"))
        assert not got[2].any() and not got[0, 5:].any() and got[0, :5].any()


@pytest.mark.parametrize("C,B,P", pc.SHAPES)
def test_host_histogram_matches_float64(C, B, P):
    """Every bucket count lies between the counts of the float64 levels that are surely in it and
    those possibly in it (perceptual_common.hist_bounds); the sums are exact; the band is
    DELTA_HIST wide (narrower than the masks' DELTA, see perceptual_common) and holds at most
    0.1 % of the case's bins; the cumulative tile counts are the tiles sparse_plan keeps."""
    import neo

    parts = spectra(C, B, P)
    for weighting in pc.WEIGHTINGS:
        for low in pc.low_bins(B):
            what = f"{(C, B, P)} {weighting} low={low}"
            sp = neo.PerceptualSparsity(pc.SAMPLE_RATE, -40.0, low, weighting)
            lv, exact = pc.levels64(parts, pc.weights64(B, pc.SAMPLE_RATE, low, weighting))
            tl, texact = pc.tile_levels64(lv, exact)
            h = neo.perceptual_histogram_host(parts, sp)
            assert h["bins"].shape == h["tiles"].shape == (C, 144) and h["bins"].dtype == np.int64
            pc.check_hist(h["bins"], lv, exact, P * (B + 1), lv.size, what + " bins")
            pc.check_hist(h["tiles"], tl, texact, P * (B // 16), lv.size, what + " tiles")
            for theta in (-20.0, -40.0, -60.0):
                mask = neo.perceptual_mask_host(parts, neo.PerceptualSparsity(pc.SAMPLE_RATE, theta, low, weighting))
                k = int(-theta)
                for c in range(C):
                    kept = neo.sparse_plan(mask[c:c + 1], B)["kept_tiles"]
                    near = int(((np.abs(tl[c] - theta) <= pc.DELTA) & ~texact[c]).sum())
                    assert abs(int(h["tiles"][c, :k].sum()) - kept) <= near, (what, theta, c)
                    assert kept == int((tl[c] > theta).sum()) or near


def test_density_helpers():
    import neo

    h = np.zeros((2, 144), np.int64)
    h[0, [10, 30, 50]] = [1, 3, 6]  # channel 0: 10 tiles
    h[1, [20, 143]] = [5, 5]        # channel 1: 10 tiles, half of them silent
    curve = neo.tile_density_curve(h)
    assert curve.shape == (2, 144) and np.all(np.diff(curve, axis=1) >= 0)
    assert curve[0, 0] == 0 and curve[0, 10] == 0 and curve[0, 11] == 0.1 and curve[0, 31] == 0.4
    assert curve[0, 51] == 1.0 and curve[0, 143] == 1.0
    assert curve[1, 20] == 0 and curve[1, 21] == 0.5 and curve[1, 143] == 0.5  # bucket 143 is never kept
    assert np.array_equal(neo.tile_density_curve(h[0]), curve[:1])
    # over all 20 tiles: thresholds down to -10 keep 0, -11 .. -20 keep 1, -21 .. -30 keep 6, -31 .. -50 keep 9
    assert neo.threshold_for_tile_density(h, 0.0) == -10
    assert neo.threshold_for_tile_density(h, 0.05) == -20  # exactly the target: 1 of 20
    assert neo.threshold_for_tile_density(h, 0.049) == -10
    assert neo.threshold_for_tile_density(h, 0.3) == -30   # exactly 6 of 20
    assert neo.threshold_for_tile_density(h, 0.44) == -30
    assert neo.threshold_for_tile_density(h, 0.45) == -50
    assert neo.threshold_for_tile_density(h, 1.0) == -143
    top = np.zeros((1, 144), np.int64)
    top[0, 0] = 4  # everything above -1 dB (low_bins_to_keep's +100): kept at every threshold
    top[0, 100] = 4
    assert neo.threshold_for_tile_density(top, 0.4) is None
    assert neo.threshold_for_tile_density(top, 0.5) == -100
    assert neo.threshold_for_tile_density(np.zeros((1, 144), np.int64), 0.5) is None
    with pytest.raises(ValueError):
        neo.tile_density_curve(np.zeros((2, 100)))


def test_perceptual_plan_host_program_under_sanitizers():
    """csrc/perceptual_plan.hpp alone (it includes no HIP header), in a program of its own built
    with the address and undefined-behaviour sanitizers and run directly; exit status 0."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    os.makedirs(BIN, exist_ok=True)
    out = os.path.join(BIN, "perceptual_plan_main")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", out,
                           os.path.join(CPP, "perceptual_plan_main.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"\d+ cases, 0 failed", r.stdout), r.stdout


def test_cpp_perceptual_builds_and_host_checks():
    b = build_cpp_test()
    r = subprocess.run([b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "perceptual host checks passed" in r.stdout
