"""The host-only shape planner (neo-dsp_amd/csrc/upols_plan.hpp) as a program: tests/cpp/upols_plan_main.cpp
built with the address and undefined-behaviour sanitizers, run directly, one case per input line."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

CPP = os.path.join(os.path.dirname(__file__), "cpp")
_built = None


def planner():
    global _built
    if _built is None:
        if not shutil.which("g++"):
            pytest.skip("no g++")
        os.makedirs(os.path.join(CPP, "bin"), exist_ok=True)
        out = os.path.join(CPP, "bin", "upols_plan_main")
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", out,
                               os.path.join(CPP, "upols_plan_main.cpp")])
        _built = out
    return _built


def plan_shapes(cases):
    """cases: (kind, borrowed, channels, block, partitions, opts) with opts the 11 neo_hip_upols_opts
    ints or None -> one dict per case: the plan's fields, or {"refused": why}."""
    lines = []
    for kind, borrowed, C, B, P, opts in cases:
        o = list(opts) if opts is not None else []
        assert len(o) in (0, 11)
        lines.append(" ".join(str(v) for v in [kind, int(borrowed), C, B, P, len(o)] + o))
    r = subprocess.run([planner()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(cases), (len(out), len(cases), r.stderr[-2000:])
    return out
