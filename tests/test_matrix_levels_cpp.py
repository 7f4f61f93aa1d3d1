"""Window levels through the C++ header API (include/neo/convolution.hpp: hip_matrix_convolver::levels,
levels_info): tests/cpp/test_matrix_levels.cpp compiles against libneo_hip.so and the oracle; its host
part runs without a GPU, its 2 x 2 and 3 x 5 cases with levels(true) against the block step on the device."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "bin")


def build():
    """flags as tests/cpp/Makefile"""
    os.makedirs(BIN, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "liboracle.so"])
    out, src = os.path.join(BIN, "test_matrix_levels"), os.path.join(CPP, "test_matrix_levels.cpp")
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


def test_matrix_levels_cpp_builds_and_host_checks():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_matrix_levels_cpp_on_gpu():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "matrix levels C++ tests passed" in r.stdout, r.stdout + r.stderr
