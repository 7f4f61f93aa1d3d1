"""Live filter updates of the dense UPOLS / UPOLA convolvers, the part that needs no GPU: null
handles, the new symbols, the spill check of the fade step and the fade split rule as a sanitized
stand-alone program ("Live filter updates of dense handles")."""
import ctypes
import inspect
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
NEW_SYMBOLS = ("neo_hip_upols_update_filter", "neo_hip_upols_update_impulse", "neo_hip_upols_fade_info",
               "neo_hip_upols_multi_update_filter", "neo_hip_upols_multi_update_impulse")


def test_null_handle_is_einval():
    import neo

    lib = neo._native.load()
    buf = np.zeros(8, np.complex64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    E = neo._native.NEO_HIP_EINVAL
    assert lib.neo_hip_upols_update_filter(None, p, 0, 1, 0, None) == E
    assert lib.neo_hip_upols_update_impulse(None, p, 8, 1, 0, 1, 0, None) == E
    r = ctypes.c_int()
    assert lib.neo_hip_upols_fade_info(None, ctypes.byref(r), None, None) == E
    assert lib.neo_hip_upols_multi_update_filter(None, p, 1, 0) == E
    assert lib.neo_hip_upols_multi_update_impulse(None, p, 8, 1, 1, 0) == E


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
    assert lib.neo_hip_version() == neo._native.ABI_VERSION >= 1300
    assert int(re.search(r"#define NEO_HIP_VERSION (\d+)", hdr).group(1)) >= 1300
    assert "0.13.0" in hdr and hdr.count("STREAM CONTRACT") >= 2
    assert neo.fade_gains is neo.matrix_fade_gains and "fade_gains" in neo.__all__ and "fade_gains" in neo.convolution.__all__
    for cls in (neo.UpolsConvolver, neo.UpolsMultiConvolver):
        sig = inspect.signature(cls.update_filter).parameters
        assert list(sig)[1:] == ["partitions", "fade_blocks", "curve", "stream"]
        assert sig["fade_blocks"].default == 1 and sig["curve"].default == "linear" and sig["stream"].default == 0
        sig = inspect.signature(cls.update_impulse).parameters
        assert list(sig)[1:] == ["impulse_response", "normalize", "fade_blocks", "curve", "stream"]
        assert sig["normalize"].default is True and sig["fade_blocks"].default == 1 and sig["curve"].default == "linear"
        assert sig["stream"].default == 0
        assert hasattr(cls, "fade_info")
    cpp = open(os.path.join(REPO, "include", "neo", "convolution.hpp")).read()
    for name in ("neo_hip_upols_update_filter", "neo_hip_upols_update_impulse", "neo_hip_upols_fade_info",
                 "neo_hip_upols_multi_update_filter", "neo_hip_upols_multi_update_impulse"):
        assert name in cpp, name
    assert cpp.index("enum class fade_curve") < cpp.index("struct upols_multichannel")


def _kernels():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import spill_check
    finally:
        sys.path.pop(0)
    return spill_check.kernels(os.path.join(REPO, "neo-dsp_amd", "lib", "libneo_hip.so"))


def test_fade_step_does_not_spill():
    """Every instantiation of k_upols_fade_step (9 block sizes x {overlap-save, overlap-add}; two
    accumulator sets, pinned to 4 waves per SIMD) in the built library: no spilled VGPR or SGPR, no
    scratch, at most 128 VGPRs (tools/spill_check.py; no GPU)."""
    steps = {n: v for n, v in _kernels().items() if "k_upols_fade_step" in n}
    assert len(steps) == 18, sorted(steps)
    sizes = sorted({int(re.search(r"k_upols_fade_stepILi(\d+)E", n).group(1)) for n in steps})
    assert sizes == [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
    bad = {n: v for n, v in steps.items() if v["vgpr_spill"] or v["sgpr_spill"] or v["scratch"]}
    assert not bad, bad
    assert all(v["vgpr"] <= 128 for v in steps.values()), steps


def _fade_plans(cases):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    os.makedirs(os.path.join(CPP, "bin"), exist_ok=True)
    out = os.path.join(CPP, "bin", "upols_fade_plan_main")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", out,
                           os.path.join(CPP, "upols_fade_plan_main.cpp")])
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
    r = subprocess.run([out], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(res) == len(cases)
    return res


def test_fade_split_rule():
    """upols_fade_split (upols_plan.hpp), sanitized: the fade step cuts the partitions exactly where
    the handle's plain step does, whether that step is one launch or two; no split is empty; the
    slabs are [C][S][2][B] and the bank the handle's own [C][ring][B]; the largest shapes do not
    overflow."""
    cases = [(C, B, P, fused, wgs)
             for C in (1, 2, 3, 16, 256, 1024)
             for B in (16, 64, 512, 1024, 4096)
             for P in (1, 3, 9, 37, 70, 255, 938, 4001)
             for fused, wgs in ((-1, 0), (0, 0), (1, 0), (0, 64), (1, 7), (-1, 100000))]
    cases += [(4096, 4096, 60000, -1, 0), (1, 4096, 65000, 0, 1 << 30), (0, 64, 8, -1, 0), (2, 48, 8, -1, 0), (2, 64, 0, -1, 0)]
    res = _fade_plans(cases)
    assert [("refused" in r) for r in res[-3:]] == [True, True, True]
    seen_s = set()
    for (C, B, P, fused, wgs), r in zip(cases[:-3], res[:-3]):
        assert "refused" not in r, ((C, B, P, fused, wgs), r)
        assert (r["S"], r["rows"]) == (r["plain_S"], r["plain_rows"]), r
        assert 1 <= r["S"] <= 64 and r["S"] * r["rows"] >= P > (r["S"] - 1) * r["rows"], ((C, B, P), r)
        assert r["slab_bytes"] == C * r["S"] * 2 * B * 8 and r["bank_bytes"] == C * r["ring"] * B * 8, r
        if fused >= 0:
            assert r["plain_fused"] == fused
        seen_s.add(r["S"])
    assert {1, 2, 64} <= seen_s
