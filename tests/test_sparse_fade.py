"""Live filter updates of the sparse UPOLS / UPOLA convolvers, the part that needs no GPU: the new
symbols, null handles, the host-only fade plan against a numpy statement, and the spill check of the
fade step ("Live filter updates")."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("neo_hip_upols_update_filter_sparse", "neo_hip_upols_update_filter_perceptual",
               "neo_hip_upols_update_impulse_perceptual", "neo_hip_upols_sparse_fade_plan")


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
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 1400
    assert int(re.search(r"#define NEO_HIP_VERSION (\d+)", hdr).group(1)) >= 1400
    assert "0.14.0" in hdr and hdr.count("STREAM CONTRACT") >= 3
    assert "sparse_fade_plan" in neo.__all__ and "sparse_fade_plan" in neo.convolution.__all__
    sig = inspect.signature(neo.SparseUpolsConvolver.update_filter).parameters
    assert list(sig)[1:] == ["partitions", "mask", "fade_blocks", "curve", "stream"]
    assert sig["mask"].default is None and sig["fade_blocks"].default == 1 and sig["curve"].default == "linear"
    assert sig["stream"].default == 0
    sig = inspect.signature(neo.SparseUpolsConvolver.update_impulse).parameters
    assert list(sig)[1:] == ["impulse_response", "sparsity", "normalize", "fade_blocks", "curve", "stream"]
    assert sig["sparsity"].default is None and sig["normalize"].default is True and sig["fade_blocks"].default == 1
    cpp = open(os.path.join(REPO, "include", "neo", "convolution.hpp")).read()
    for name in NEW_SYMBOLS[:3]:
        assert name in cpp, name


def test_null_handle_is_einval():
    import neo

    lib = neo._native.load()
    buf = np.zeros(8, np.complex64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    pp = neo.PerceptualSparsity(48000.0, -40.0)._c()
    E = neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_upols_update_filter_sparse(None, p, p, 0, 1, 0, None) == E
    assert lib.neo_hip_upols_update_filter_perceptual(None, p, ctypes.byref(pp), 0, 1, 0, None) == E
    assert lib.neo_hip_upols_update_impulse_perceptual(None, p, 8, 1, ctypes.byref(pp), 0, 1, 0, None) == E
    t = ctypes.c_int64()
    assert lib.neo_hip_upols_sparse_fade_plan(None, p, 1, 16, 1, ctypes.byref(t), None, None, None, None) == E
    assert lib.neo_hip_upols_sparse_fade_plan(p, None, 1, 16, 1, ctypes.byref(t), None, None, None, None) == E


def _tiles(mask, B):
    """kept 128-byte tiles per row [C][P][B / 16] bool: column k in tile k // 16, column B (Nyquist) in tile 0"""
    C, P, _ = mask.shape
    t = mask[:, :, :B].reshape(C, P, B // 16, 16).any(axis=3)
    t[:, :, 0] |= mask[:, :, B]
    return t


def _pairs(C, B, P):
    rng = np.random.default_rng(600 + B + P)
    u = rng.random((C, P, B + 1))
    return {"nested": (u < 0.1, u < 0.5), "disjoint": (u < 0.2, u >= 0.9),
            "one empty": (u < 0.3, np.zeros_like(u, bool)), "identical": (u < 0.25, u < 0.25)}


@pytest.mark.parametrize("B", [16, 512, 1024])
def test_sparse_fade_plan_against_numpy(B):
    import neo

    C, P = 3, 9
    for name, (ma, mb) in _pairs(C, B, P).items():
        r = neo.sparse_fade_plan(ma, mb, B)
        ta, tb = _tiles(ma, B), _tiles(mb, B)
        want = {"tiles_a": int(ta.sum()), "tiles_b": int(tb.sum()), "tiles_union": int((ta | tb).sum())}
        assert {k: r[k] for k in want} == want, (name, B, r, want)
        assert r["tiles_a"] == neo.sparse_plan(ma, B)["kept_tiles"] and r["tiles_b"] == neo.sparse_plan(mb, B)["kept_tiles"]
        if name == "nested":
            assert r["tiles_union"] == r["tiles_b"] >= r["tiles_a"]
        if name == "disjoint":  # disjoint columns may still share tiles
            assert max(r["tiles_a"], r["tiles_b"]) <= r["tiles_union"] <= r["tiles_a"] + r["tiles_b"]
        if name == "one empty":
            assert r["tiles_b"] == 0 and r["tiles_union"] == r["tiles_a"]
        if name == "identical":
            assert r["tiles_a"] == r["tiles_b"] == r["tiles_union"]
        S, nw = r["splits"], max(1, B // 512)
        assert 1 <= S <= 64 and S <= P
        # kept tiles of both banks and the FDL tiles of the union, both banks' bitmap words and offsets, the
        # inserted row, the slabs [C][S][2][B] written and read, the block in and out
        assert r["step_bytes"] == (128 * (want["tiles_a"] + want["tiles_b"] + want["tiles_union"]) + 2 * C * P * (nw + 1) * 4 +
                                   C * B * 8 + 2 * C * S * 2 * B * 8 + 2 * C * B * 4), (name, B, r)
    one = np.ones((P, B + 1), bool)  # [P][B+1] is one channel
    assert neo.sparse_fade_plan(one, one, B)["tiles_union"] == P * (B // 16)
    with pytest.raises(ValueError):
        neo.sparse_fade_plan(one, one[:-1], B)
    with pytest.raises(ValueError):
        neo.sparse_fade_plan(one, one, 2 * B)


def _kernels():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import spill_check
    finally:
        sys.path.pop(0)
    return spill_check.kernels(os.path.join(REPO, "neo-dsp_amd", "lib", "libneo_hip.so"))


def test_sparse_fade_step_does_not_spill():
    """Every instantiation of k_upols_sparse_fade_step (9 block sizes x {overlap-save, overlap-add}; two
    accumulator sets and two banks' bitmap arithmetic, pinned to 4 waves per SIMD) in the built
    library: no spilled VGPR or SGPR, no scratch, at most 128 VGPRs (tools/spill_check.py; no GPU)."""
    steps = {n: v for n, v in _kernels().items() if "k_upols_sparse_fade_step" in n}
    assert len(steps) == 18, sorted(steps)
    sizes = sorted({int(re.search(r"k_upols_sparse_fade_stepILi(\d+)E", n).group(1)) for n in steps})
    assert sizes == [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
    bad = {n: v for n, v in steps.items() if v["vgpr_spill"] or v["sgpr_spill"] or v["scratch"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 128 for v in steps.values()), steps
