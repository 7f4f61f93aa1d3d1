"""A handle follows its plan: what the C-ABI getters of six small handles report
(neo_hip_upols_info, batch_info, get_offline, get_ahead, sparse_batch_info) against what the
host-only planner (csrc/upols_plan.hpp, built and run as tests/cpp/upols_plan_main.cpp) gives for
the same shapes. The planner itself is pinned to the recorded handles by tests/test_upols_plan.py.

  dense  2 x 64 x 70     levels on (Toeplitz only), no offline windows
  dense  1 x 256 x 300   levels with the far band, offline windows, three segments
  dense  4 x 16 x 1100   the cap of 64 splits
  v2     2 x 64 x 8      no levels, no offline windows
  sparse 2 x 64 x 70     cut like its dense twin
  sparse 1 x 256 x 40"""
import ctypes

import pytest

from upols_plan_common import plan_shapes

pytestmark = pytest.mark.gpu

HANDLES = [("dense", 2, 64, 70), ("dense", 1, 256, 300), ("dense", 4, 16, 1100), ("v2", 2, 64, 8), ("sparse", 2, 64, 70),
           ("sparse", 1, 256, 40)]


def getters(neo, kind, C, B, P):
    if kind == "sparse":
        conv = neo.SparseUpolsConvolver(C, B, P)
    else:
        conv = neo.UpolsConvolver(C, B, P, method="upola_v2" if kind == "v2" else "upols")
    lib = neo._native.load()
    v = [ctypes.c_int() for _ in range(4)]
    neo._native.check(lib.neo_hip_upols_info(conv._h, *[ctypes.byref(x) for x in v]))
    out = {"info": tuple(x.value for x in v), "batch_info": conv.batch_info(), "offline": conv.offline_info(),
           "ahead": conv.ahead_info()}
    if kind == "sparse":
        out["sparse_batch_info"] = conv.sparse_batch_info()
    return out


def test_handles_follow_their_plan(neo_gpu):
    plans = plan_shapes([(k, 0, C, B, P, None) for k, C, B, P in HANDLES])
    got = {}
    for (kind, C, B, P), p in zip(HANDLES, plans):
        assert "refused" not in p, (kind, C, B, P, p)
        g = got[(kind, C, B, P)] = getters(neo_gpu, kind, C, B, P)
        assert g["info"] == (C, B, P, p["S"]), (kind, C, B, P, g, p)
        assert g["batch_info"] == ((p["batch_blocks"], p["Sb"]) if p["batch"] else (1, p["S"])), (kind, C, B, P, g, p)
        assert g["offline"] == (bool(p["off"]), p["off_nseg"]), (kind, C, B, P, g, p)
        assert g["ahead"] == (bool(p["ahead"]), 0, p["window"], p["levels"] + (1 if p["nseg"] else 0)), (kind, C, B, P, g, p)
        if kind == "sparse":
            s = g["sparse_batch_info"]
            assert (s["blocks_per_pass"], s["splits"], s["window_tiles"]) == (p["batch_blocks"], p["Sb"], 0), (s, p)
    # the plans are the ones meant: the cap of 64 splits, levels and offline windows where they start
    by = {h: p for h, p in zip(HANDLES, plans)}
    # (capped at 64 splits, 1100 partitions go 18 to a split, so 62 splits; uncapped 69 of 16)
    assert by[("dense", 4, 16, 1100)]["rows"] == -(-1100 // 64) and by[("dense", 1, 256, 300)]["off_nseg"] == 3
    assert [by[h]["ahead"] for h in HANDLES] == [1, 1, 1, 0, 0, 0] and [by[h]["off"] for h in HANDLES] == [0, 1, 1, 0, 0, 0]
    # a sparse handle and its dense twin cut the partitions alike
    assert got[("sparse", 2, 64, 70)]["info"] == got[("dense", 2, 64, 70)]["info"]
    assert got[("sparse", 2, 64, 70)]["sparse_batch_info"]["splits"] == got[("dense", 2, 64, 70)]["batch_info"][1]
