"""Live filter updates of the matrix convolver, the part that needs no GPU: the gain curve
(neo_hip_matrix_fade_gains, the expression the fade kernel evaluates) against its closed form, the
refused calls, the spill check of the new kernels and the new symbols ("Live filter
updates")."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("neo_hip_matrix_update_filter", "neo_hip_matrix_update_impulse", "neo_hip_matrix_fade_info",
               "neo_hip_matrix_fade_gains")


def closed_form(B, F, curve):
    t = np.arange(F * B, dtype=np.float64) / (F * B)
    return t if curve == "linear" else 0.5 - 0.5 * np.cos(np.pi * t)


@pytest.mark.parametrize("curve", ["linear", "cosine"])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("B", [16, 512])
def test_gains_against_the_closed_form(B, F, curve):
    import neo

    g = neo.matrix_fade_gains(B, F, curve)
    assert g.dtype == np.float32 and g.shape == (F * B,)
    want = closed_form(B, F, curve)
    # float64 evaluation rounded once: half an ulp of float32; allow 2 (another libm's cos)
    ulp = np.spacing(np.maximum(np.abs(want), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(g.astype(np.float64) - want) <= 2 * ulp), np.abs(g - want).max()
    assert g[0] == 0.0
    assert np.all(np.diff(g) >= 0) and g[-1] > g[0], "not monotone"
    assert np.all(g < 1.0)
    # the number and the name of a curve are the same thing
    assert np.array_equal(neo.matrix_fade_gains(B, F, {"linear": 0, "cosine": 1}[curve]), g)


def test_gains_refuse_bad_arguments():
    import neo

    for F in (0, -1, (1 << 20) + 1):
        with pytest.raises(neo._native.NeoHipError):
            neo.matrix_fade_gains(64, F, "linear")
    for curve in (2, -1):
        with pytest.raises(neo._native.NeoHipError):
            neo.matrix_fade_gains(64, 2, curve)
    with pytest.raises(ValueError):
        neo.matrix_fade_gains(64, 2, "cubic")
    for B in (0, 8, 48, 8192):
        with pytest.raises(neo._native.NeoHipError):
            neo.matrix_fade_gains(B, 2, "linear")
    lib = neo._native.load()
    assert lib.neo_hip_matrix_fade_gains(64, 2, 0, None) == neo._native.NEO_HIP_EINVAL


def test_null_handle_is_einval():
    import neo

    lib = neo._native.load()
    buf = np.zeros(8, np.complex64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.neo_hip_matrix_update_filter(None, p, 0, 1, 0, None) == neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_matrix_update_impulse(None, p, 8, 1, 0, 1, 0, None) == neo._native.NEO_HIP_EINVAL
    r = ctypes.c_int()
    assert lib.neo_hip_matrix_fade_info(None, ctypes.byref(r), None, None) == neo._native.NEO_HIP_EINVAL


def _kernels():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import spill_check
    finally:
        sys.path.pop(0)
    return spill_check.kernels(os.path.join(REPO, "neo-dsp_amd", "lib", "libneo_hip.so"))


def test_fade_kernels_do_not_spill():
    """Every instantiation of k_matrix_fade_step (two accumulator sets, pinned to 4 waves per SIMD:
    at most 128 VGPRs) and k_matrix_fade_finish in the built library: no spilled VGPR or SGPR, no
    scratch (tools/spill_check.py; no GPU)."""
    mine = {n: v for n, v in _kernels().items() if "k_matrix_fade_" in n}
    steps = {n: v for n, v in mine.items() if "k_matrix_fade_step" in n}
    fins = {n: v for n, v in mine.items() if "k_matrix_fade_finish" in n}
    assert len(steps) == 9 and len(fins) == 27, sorted(mine)  # 9 block sizes; x {ols, ola, prime}
    bad = {n: v for n, v in mine.items() if v["vgpr_spill"] or v["sgpr_spill"] or v["scratch"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 128 for v in steps.values()), steps
    assert all(v["vgpr"] <= 256 for v in fins.values()), fins


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
    assert hasattr(neo, "matrix_fade_gains") and "matrix_fade_gains" in neo.__all__
    assert "matrix_fade_gains" in neo.convolution.__all__
    for name in ("update_filter", "update_impulse", "fade_info"):
        assert hasattr(neo.MatrixConvolver, name), name
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 900
    assert int(re.search(r"#define NEO_HIP_VERSION (\d+)", hdr).group(1)) >= 900
    assert "0.9.0" in hdr and "STREAM CONTRACT" in hdr
    cpp = open(os.path.join(REPO, "include", "neo", "convolution.hpp")).read()
    assert "auto update_filter(" in cpp and "auto update_impulse(" in cpp and "fade_info()" in cpp
    assert "enum class fade_curve" in cpp
    sig = inspect.signature(neo.MatrixConvolver.update_filter).parameters
    assert sig["fade_blocks"].default == 1 and sig["curve"].default == "linear"
    sig = inspect.signature(neo.MatrixConvolver.update_impulse).parameters
    assert sig["normalize"].default is True and sig["fade_blocks"].default == 1
