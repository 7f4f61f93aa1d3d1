"""Live filter updates of the sparse convolvers through the C++ header API
(include/neo/convolution.hpp: sparse_upola_convolver::update_filter with a predicate,
upols_multichannel::update_impulse_perceptual): tests/cpp/sparse_fade_main.cpp compiles against
libneo_hip.so and the oracle; its host part runs without a GPU; on the device its two runs (B = 32,
P = 5, 24 blocks, the update before block 7) must give the bits of the same calls through
neo.SparseUpolsConvolver."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "bin")
B, P, NB, AT = 32, 5, 24, 7  # as tests/cpp/sparse_fade_main.cpp


def build():
    """flags as tests/cpp/Makefile"""
    os.makedirs(BIN, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "liboracle.so"])
    out, src = os.path.join(BIN, "sparse_fade_main"), os.path.join(CPP, "sparse_fade_main.cpp")
    deps = [src, os.path.join(REPO, "include", "neo_hip.h"), os.path.join(REPO, "include", "neo", "convolution.hpp"),
            os.path.join(REPO, "neo-dsp_amd", "lib", "libneo_hip.so")]
    if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(REPO, "include"),
                           "-o", out, src,
                           "-L" + os.path.join(REPO, "neo-dsp_amd", "lib"), "-lneo_hip",
                           "-L" + os.path.join(REPO, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(REPO, "neo-dsp_amd", "lib"),
                           "-Wl,-rpath," + os.path.join(REPO, "oracle")])
    return out


def test_sparse_fade_cpp_builds_and_host_checks():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_sparse_fade_cpp_on_gpu(neo_gpu, oracle, tmp_path):
    neo = neo_gpu
    files = [str(tmp_path / "predicate.f32"), str(tmp_path / "impulse.f32")]
    r = subprocess.run([build()] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sparse fade C++ tests passed" in r.stdout, r.stdout + r.stderr

    def impulse(seed, C):
        return oracle.normalize_impulse(np.stack([oracle.noise(seed + c, B * P) for c in range(C)]))

    # 1. sparse_upola_convolver::update_filter(matrix, predicate)
    pa, pb = (oracle.uniform_partition(impulse(s, 1), B) for s in (6100, 6200))
    r_, c_ = np.meshgrid(np.arange(P), np.arange(B + 1), indexing="ij")
    ma, mb = ((r_ + c_) % 3 != 0)[None], ((c_ % 2 == 0) | (r_ == 1))[None]
    y = oracle.noise(6400, B * NB)[None].copy()
    conv = neo.SparseUpolsConvolver(1, B, P, method="upola")
    conv.filter(pa, ma)
    for b in range(NB):
        if b == AT:
            conv.update_filter(pb, mb, fade_blocks=3, curve="cosine")
        blk = np.ascontiguousarray(y[:, b * B:(b + 1) * B])
        conv(blk)
        y[:, b * B:(b + 1) * B] = blk
    conv.close()
    got = np.fromfile(files[0], dtype=np.float32).reshape(1, NB * B)
    assert got.any()
    assert np.array_equal(got.view(np.uint32), y.view(np.uint32)), "predicate: C++ and Python paths differ"

    # 2. upols_multichannel::update_impulse_perceptual
    C = 3
    ira, irb = impulse(6500, C), impulse(6600, C)
    sa, sb = neo.PerceptualSparsity(48000.0, -20.0, 0, "a"), neo.PerceptualSparsity(48000.0, -8.0, 2, "a")
    x = np.stack([oracle.noise(6700 + c, B * NB) for c in range(C)])
    conv = neo.SparseUpolsConvolver(C, B, P, method="upols")
    conv.set_impulse(ira, sa, normalize=False)
    out = [conv.process(np.ascontiguousarray(x[:, :AT * B]).copy())]
    conv.update_impulse(irb, sb, normalize=False, fade_blocks=2, curve="linear")
    out.append(conv.process(np.ascontiguousarray(x[:, AT * B:]).copy()))
    conv.close()
    want = np.concatenate(out, axis=1)
    got = np.fromfile(files[1], dtype=np.float32).reshape(C, NB * B)
    assert got.any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "impulse: C++ and Python paths differ"
