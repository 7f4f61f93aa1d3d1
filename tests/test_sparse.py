"""Sparse convolvers, the part that needs no GPU: the symbols are declared, exported and bound;
argument checks run before any device is touched; the host plan (neo_hip_upols_sparse_plan, the
definition of the tile-compacted format) against a numpy restatement of it; the stand-alone
sanitizer program for csrc/sparse_plan.hpp; the host part of the C++ test."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "bin")
SPARSE_SYMBOLS = ("neo_hip_upols_create_sparse", "neo_hip_upols_set_filter_sparse", "neo_hip_upols_sparse_info",
                  "neo_hip_upols_sparse_plan")


def build_cpp_test():
    """tests/cpp/test_sparse.cpp against libneo_hip.so and the oracle (flags as tests/cpp/Makefile)."""
    os.makedirs(BIN, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "liboracle.so"])
    out = os.path.join(BIN, "test_sparse")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(REPO, "include"),
                           "-o", out, os.path.join(CPP, "test_sparse.cpp"),
                           "-L" + os.path.join(REPO, "neo-dsp_amd", "lib"), "-lneo_hip",
                           "-L" + os.path.join(REPO, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(REPO, "neo-dsp_amd", "lib"),
                           "-Wl,-rpath," + os.path.join(REPO, "oracle")])
    return out


def test_sparse_symbols_declared_exported_bound():
    import neo

    hdr = open(os.path.join(REPO, "include", "neo_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", neo._native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (neo_hip_\w+)", out))
    lib = neo._native.load()
    for s in SPARSE_SYMBOLS:
        assert re.search(r"NEO_HIP_API\s+int\s+" + s + r"\s*\(", hdr), s
        assert s in exported, s
        assert s in neo._native.SIGNATURES, s
        assert getattr(lib, s).argtypes is not None
    for name in ("SparseUpolsConvolver", "sparse_upols_convolver", "sparse_upola_convolver", "sparse_plan",
                 "sparse_convolve"):
        assert hasattr(neo, name) and name in neo.__all__, name
    assert issubclass(neo.SparseUpolsConvolver, neo.UpolsConvolver)
    cpp = open(os.path.join(REPO, "include", "neo", "convolution.hpp")).read()
    assert "using sparse_upols_convolver" in cpp and "using sparse_upola_convolver" in cpp
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 300


def test_create_sparse_validates_without_device():
    import neo

    lib = neo._native.load()
    h = ctypes.c_void_p()
    E = neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_upols_create_sparse(1, 500, 3, 0, 0, None, ctypes.byref(h)) == E
    assert b"power of two" in lib.neo_hip_last_error()
    assert lib.neo_hip_upols_create_sparse(1, 512, 3, 0, 2, None, ctypes.byref(h)) == E
    assert b"method" in lib.neo_hip_last_error()
    assert lib.neo_hip_upols_create_sparse(0, 512, 3, 0, 0, None, ctypes.byref(h)) == E
    assert b"channels" in lib.neo_hip_last_error()
    assert lib.neo_hip_upols_create_sparse(1, 512, 0, 0, 1, None, ctypes.byref(h)) == E
    assert not h.value
    assert lib.neo_hip_upols_sparse_info(None, None, None, None) == E
    assert lib.neo_hip_upols_set_filter_sparse(None, None, None, 0) == E
    m = np.ones((1, 2, 17), np.uint8)
    assert lib.neo_hip_upols_sparse_plan(m.ctypes.data_as(ctypes.c_void_p), 1, 500, 2, None, None, None, None) == E
    with pytest.raises(ValueError):
        neo.sparse_plan(np.ones((2, 5, 16), bool), 16)  # B + 1 columns
    with pytest.raises(ValueError):
        neo.SparseUpolsConvolver(1, 512, 3, method="upola_v2")
    with pytest.raises(ValueError):
        neo.SparseUpolsConvolver(1, 512, 3, options={"levels": 1})


def plan_numpy(mask, B):
    """The format of include/neo_hip.h restated: tile t of a row holds packed bins [16 t, 16 t + 16);
    packed bin 0 is {DC, Nyquist} (columns 0 and B), packed bin k is column k."""
    C, P, _ = mask.shape
    NT, NW = B // 16, max(1, B // 512)
    packed = mask[:, :, :B].copy()
    packed[:, :, 0] |= mask[:, :, B]
    keep = packed.reshape(C, P, NT, 16).any(axis=3)  # [C][P][NT]
    bits = np.zeros((C, P, NW * 32), dtype=bool)
    bits[:, :, :NT] = keep
    words = (bits.reshape(C, P, NW, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=3)
    counts = keep.sum(axis=2)
    off = np.zeros((C, P + 1), dtype=np.uint32)
    off[:, 1:] = np.cumsum(counts, axis=1)
    return words.astype(np.uint32), off, int(mask.sum()), int(keep.sum())


def plan_masks(C, P, B):
    rng = np.random.default_rng(1000 + B + C)
    k = np.arange(B + 1)
    shape = (C, P, B + 1)
    full = np.ones(shape, bool)
    yield "all-true", full
    yield "all-false", np.zeros(shape, bool)
    yield "dc-only", np.broadcast_to(k == 0, shape).copy()
    yield "nyquist-only", np.broadcast_to(k == B, shape).copy()
    m = np.broadcast_to((k % 5 == 0) & (k > 0) | (k == B), shape).copy()
    yield "dc-dropped-nyquist-kept", m
    m = np.zeros(shape, bool)
    for p in range(P):
        m[:, p, (k % 16 == (3 + p) % 16) & (k < B)] = True
    yield "one-column-per-tile", m
    yield "bernoulli-0.5", rng.random(shape) < 0.5
    yield "bernoulli-0.01", rng.random(shape) < 0.01
    m = rng.random(shape) < 0.3
    m[:, P // 2] = False
    yield "empty-row-middle", m
    m = rng.random(shape) < 0.3
    m[:, P - 1] = False
    yield "empty-row-end", m


@pytest.mark.parametrize("B", [16, 32, 512, 1024, 4096])
def test_sparse_plan_matches_format(B):
    import neo

    P = 5
    for C in (1, 3):
        for name, mask in plan_masks(C, P, B):
            got = neo.sparse_plan(mask, B)
            words, off, bins, tiles = plan_numpy(mask, B)
            assert got["tile_mask"].shape == (C, P, max(1, B // 512)), name
            assert np.array_equal(got["tile_mask"], words), (name, B, C)
            assert np.array_equal(got["row_off"], off), (name, B, C)
            assert got["kept_bins"] == bins and got["kept_tiles"] == tiles, (name, B, C)
            if name == "all-true":
                assert tiles == C * P * (B // 16) and bins == C * P * (B + 1)
            if name in ("dc-only", "nyquist-only"):
                assert tiles == C * P and bins == C * P and np.all(got["tile_mask"][:, :, 0] == 1)
    # a rank-2 mask is one channel
    m2 = np.arange(P * (B + 1)).reshape(P, B + 1) % 7 == 0
    assert np.array_equal(neo.sparse_plan(m2, B)["row_off"], neo.sparse_plan(m2[None], B)["row_off"])


def test_sparse_plan_host_program_under_sanitizers():
    """csrc/sparse_plan.hpp alone (it includes no HIP header), in a program of its own built with
    the address and undefined-behaviour sanitizers; the same mask set; exit status 0."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    os.makedirs(BIN, exist_ok=True)
    out = os.path.join(BIN, "sparse_plan_main")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", out, os.path.join(CPP, "sparse_plan_main.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "100 cases, 0 failed" in r.stdout


def test_cpp_sparse_builds_and_host_checks():
    b = build_cpp_test()
    r = subprocess.run([b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_sparse_on_gpu():
    """tests/cpp/test_sparse.cpp on the device: the reference's identity test through both sparse
    aliases, and a predicate against the dense alias on the zeroed filter (<= 1e-5 peak)."""
    b = build_cpp_test()
    r = subprocess.run([b], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sparse C++ tests passed" in r.stdout
