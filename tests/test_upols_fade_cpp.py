"""Live filter updates of the dense convolvers through the C++ header API
(include/neo/convolution.hpp: upols_multichannel / upols_multidevice update_filter, update_impulse,
fade_info): tests/cpp/upols_fade_main.cpp compiles against libneo_hip.so and the oracle; its host
part runs without a GPU; on the device it checks the C++ calls against the C ones bit for bit
(and the sharded class against the unsharded one), and its 3-channel, B = 32, P = 5 run (filter A, 7
blocks, an update over 3 blocks, 6 blocks, an update over 2 blocks from an impulse normalised on the
host, 8 blocks more) must give
the bits of the same calls through neo.UpolsConvolver."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "bin")
C, B, P, NB, AT1, AT2, FADE1, FADE2 = 3, 32, 5, 24, 7, 16, 3, 2  # as tests/cpp/upols_fade_main.cpp


def build():
    """flags as tests/cpp/Makefile"""
    os.makedirs(BIN, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "liboracle.so"])
    out, src = os.path.join(BIN, "upols_fade_main"), os.path.join(CPP, "upols_fade_main.cpp")
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


def test_upols_fade_cpp_builds_and_host_checks():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_upols_fade_cpp_on_gpu(neo_gpu, oracle, tmp_path):
    neo = neo_gpu
    files = [str(tmp_path / "upols.f32"), str(tmp_path / "upola.f32")]
    r = subprocess.run([build()] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "upols fade C++ tests passed" in r.stdout, r.stdout + r.stderr

    def impulse(seed):
        return np.stack([oracle.noise(seed + c, B * P) for c in range(C)])

    def parts(seed):
        return oracle.uniform_partition(oracle.normalize_impulse(impulse(seed)), B)

    pa, pb, irc = parts(5100), parts(5200), oracle.normalize_impulse(impulse(5300))
    x = np.stack([oracle.noise(5400 + c, B * NB) for c in range(C)])
    for method, path in zip(("upols", "upola"), files):
        conv = neo.UpolsConvolver(C, B, P, method=method)
        conv.filter(pa)
        y = [conv.process(np.ascontiguousarray(x[:, :AT1 * B]).copy())]
        conv.update_filter(pb, fade_blocks=FADE1, curve="cosine")
        y.append(conv.process(np.ascontiguousarray(x[:, AT1 * B:AT2 * B]).copy()))
        conv.update_impulse(irc, normalize=False, fade_blocks=FADE2, curve="linear")
        y.append(conv.process(np.ascontiguousarray(x[:, AT2 * B:]).copy()))
        conv.close()
        want = np.concatenate(y, axis=1)
        got = np.fromfile(path, dtype=np.float32).reshape(C, NB * B)
        assert got.any()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{method}: C++ and Python paths differ"
