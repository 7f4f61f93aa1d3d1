"""Live filter updates through the C++ header API (include/neo/convolution.hpp:
hip_matrix_convolver::update_filter, update_impulse, fade_info, fade_curve):
tests/cpp/test_matrix_fade.cpp compiles against libneo_hip.so and the oracle; its host part runs
without a GPU; on the device its 2 x 2, B = 32, P = 5 run (filter A, 7 blocks, an update over 3
blocks, 13 blocks more) must give the bits of the same calls through neo.MatrixConvolver."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "bin")
I, O, B, P, NB, AT, FADE = 2, 2, 32, 5, 20, 7, 3  # as tests/cpp/test_matrix_fade.cpp


def build():
    """flags as tests/cpp/Makefile"""
    os.makedirs(BIN, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "liboracle.so"])
    out, src = os.path.join(BIN, "test_matrix_fade"), os.path.join(CPP, "test_matrix_fade.cpp")
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


def test_matrix_fade_cpp_builds_and_host_checks():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_matrix_fade_cpp_on_gpu(neo_gpu, oracle, tmp_path):
    neo = neo_gpu
    files = [str(tmp_path / "upols.f32"), str(tmp_path / "upola.f32")]
    r = subprocess.run([build()] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "matrix fade C++ tests passed" in r.stdout, r.stdout + r.stderr
    routes = [(0, 0), (0, 1), (1, 0), (1, 1)]

    def parts(seed):
        ir = np.stack([oracle.noise(seed + k, B * P) for k in range(len(routes))])
        return oracle.uniform_partition(oracle.normalize_impulse(ir), B)

    pa, pb = parts(4100), parts(4200)
    x = np.stack([oracle.noise(4300 + i, B * NB) for i in range(I)])
    for method, path in zip(("upols", "upola"), files):
        conv = neo.MatrixConvolver(I, O, B, P, method=method)
        conv.filter(pa, routes)
        head = conv.process(x[:, :AT * B])
        conv.update_filter(pb, fade_blocks=FADE, curve="cosine")
        want = np.concatenate([head, conv.process(x[:, AT * B:])], axis=1)
        conv.close()
        got = np.fromfile(path, dtype=np.float32).reshape(O, NB * B)
        assert got.any()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{method}: C++ and Python paths differ"
