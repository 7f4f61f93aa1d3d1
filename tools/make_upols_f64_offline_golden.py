#!/usr/bin/env python3
"""Writes tests/golden/upols_f64_offline_case.bin, the float64 fixture of tests/cpp/test_f64_offline.cpp:
tests/golden/upols_f64_case.bin's layout with enough blocks for a window, a batched pass and a
remainder (147 = 128 + 16 + 3) and a filter of two segments, the last of one partition (129), and its
numpy truth (tests/upols_f64_truth.py). Little-endian: int64 C, B, P, nb, L; then float64 ir [C][L],
x [C][nb B], y_upols [C][nb B], y_upola [C][nb B] (the filter is uniform_partition of ir, not
normalized)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import upols_f64_truth as T  # noqa: E402

C, B, P, nb = 3, 16, 129, 147
rng = np.random.default_rng(641728)
ir = rng.standard_normal((C, P * B - 3))
x = rng.standard_normal((C, nb * B))
H = T.partition(ir, B)
ys = [T.blockwise(x, H, m) for m in ("upols", "upola")]
assert all(T.peak_err(y, T.whole(x, ir)) < 1e-13 for y in ys)
out = os.path.join(REPO, "tests", "golden", "upols_f64_offline_case.bin")
with open(out, "wb") as f:
    f.write(np.array([C, B, P, nb, ir.shape[1]], dtype="<i8").tobytes())
    for a in (ir, x, *ys):
        f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
print(out, os.path.getsize(out), "bytes")
