"""Offline windows through the C++ header API (include/neo/convolution.hpp:
upols_multichannel64::offline / offline_info, dense_convolve on double arrays with the switch):
tests/cpp/test_f64_offline.cpp compiles against libneo_hip.so; its host part runs without a GPU, the
3-channel case of tests/golden/upols_f64_offline_case.bin (float64 numpy truth,
tools/make_upols_f64_offline_golden.py) on the device, overlap-save and overlap-add, in calls that hold
a window, a batched pass and a remainder, at 1e-12."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "upols_f64_offline_case.bin")


def run():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "f64_offline.mk", "bin/test_f64_offline"])
    return subprocess.run([os.path.join(CPP, "bin", "test_f64_offline"), GOLDEN], capture_output=True, text=True, timeout=300)


def test_f64_offline_cpp_builds_and_host_checks():
    r = run()
    assert r.returncode == 0, r.stdout + r.stderr


def test_golden_fixture_is_the_numpy_truth():
    """The committed fixture equals what its generator's statement of the algorithm gives now, agrees
    with np.convolve within 1e-13, and holds a window, a batched pass of 16 blocks and a remainder."""
    import numpy as np

    import upols_f64_truth as T

    assert os.path.getsize(GOLDEN) < 1 << 20
    raw = open(GOLDEN, "rb").read()
    C, B, P, nb, L = (int(v) for v in np.frombuffer(raw, "<i8", 5))
    assert (C, B, P, nb) == (3, 16, 129, 128 + 16 + 3)
    body = np.frombuffer(raw, "<f8", offset=40)
    n = nb * B
    assert body.size == C * (L + 3 * n)
    ir, x = body[:C * L].reshape(C, L), body[C * L:C * (L + n)].reshape(C, n)
    for i, method in enumerate(("upols", "upola")):
        y = body[C * (L + n * (1 + i)):C * (L + n * (2 + i))].reshape(C, n)
        assert T.peak_err(y, T.blockwise(x, T.partition(ir, B), method)) <= 1e-15
        assert T.peak_err(y, T.whole(x, ir)) <= T.TRUTH_AGREE


@pytest.mark.gpu
def test_f64_offline_cpp_on_gpu():
    r = run()
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "f64 offline C++ tests passed" in r.stdout, r.stdout + r.stderr
