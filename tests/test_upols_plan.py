"""The shape plan of the UPOLS handles (neo-dsp_amd/csrc/upols_plan.hpp: make_upols_shape), without
a GPU: against the values the create functions computed before the header existed, recorded on an
MI355X from inside those functions (tests/golden/upols_shape_plans.json; never regenerated from
the header), and against the structural facts every plan must satisfy."""
from __future__ import annotations

import json
import os

import pytest

from upols_plan_common import plan_shapes

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "upols_shape_plans.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    cases = [tuple(c[:6]) for c in g["cases"]]
    want = [None if c[6] is None else dict(zip(g["plan_fields"], c[6])) for c in g["cases"]]
    return g, cases, want, plan_shapes(cases)


def test_grid_covers_every_edge(golden):
    """The recorded grid holds both sides of every edge of the rules (so equality below means
    something): the fused rule's 4 Mi, both cache budgets, the three min_rows, explicit split targets,
    the caps at 64 splits, the batched bin groups and blocks per pass, the level and offline cut-offs,
    the grown rings, v2 and borrowed handles, the 2 GiB edge, refusals of every kind."""
    g, cases, want, _ = golden
    assert len(cases) == 614 and sum(w is None for w in want) == 68
    ok = [(c, w) for c, w in zip(cases, want) if w is not None]
    auto = [(c, w) for c, w in ok if c[5] is None]
    assert {w["fused"] for c, w in auto if c[2] * c[3] * c[4] == 4 << 20} == {0}
    assert {w["fused"] for c, w in auto if c[2:5] in ((64, 256, 255), (16, 1024, 255), (1, 4096, 1023), (2, 64, 32767))} == {1}
    for budget, f in ((216 << 20, "pc"), (168 << 20, "pcb")):
        below = [w for c, w in ok if c[0] == "dense" and w[f] == c[4] and 8 * c[2] * c[3] * (c[4] + 1) > budget]
        above = [w for c, w in ok if c[0] == "dense" and w[f] < c[4]]
        assert len(below) >= 3 and len(above) >= 3, (f, len(below), len(above))
    assert {w["S"] for c, w in ok} >= {1, 2, 3, 4, 64} and {w["Sb"] for c, w in ok} >= {1, 2, 64}
    assert any(w["S"] == 64 and c[4] > 64 * w["rows"] - w["rows"] for c, w in ok)
    assert {w["bNB"] for c, w in ok} == {1, 2} and {w["batch_blocks"] for c, w in ok} == {2, 4, 8, 16, 32}
    assert {c[4] for c in cases} >= {63, 64, 127, 128, 129, 256, 257} and {c[3] for c in cases} >= {16, 256, 512, 1024, 2048, 4096}
    assert {w["ahead"] for c, w in ok} == {0, 1} and {w["off"] for c, w in ok} == {0, 1} and {w["bufload"] for c, w in ok} == {0, 1}
    assert any(w["ring"] == c[4] + 256 for c, w in ok if c[5] and c[5][5] == 2)  # far_level 2: P + 2 * 128 rows
    assert any(w["stag"] for c, w in ok) and {w["sg"] for c, w in ok} >= {1, 2, 4, 8}
    assert sum(c[1] for c in cases) >= 12 and {c[0] for c in cases} == {"dense", "v2", "sparse"}
    assert {w["ring"] * c[3] < 1 << 28 for c, w in ok if c[3] == 4096 and c[4] > 60000} == {True, False}
    refused_sparse = [c for c, w in zip(cases, want) if w is None and c[0] == "sparse" and c[5] is None and c[2] > 0 and c[4] > 0
                      and c[3] in (16, 1024, 4096)]
    assert len(refused_sparse) >= 3 and all((c[4] + 31) * c[3] >= 1 << 28 for c in refused_sparse)


def test_plan_reproduces_recorded_handles(golden):
    """Entry for entry: every recorded field equal, every recorded refusal refused (and nothing else)."""
    _, cases, want, got = golden
    bad = []
    for c, w, r in zip(cases, want, got):
        if w is None:
            if "refused" not in r:
                bad.append((c, "accepted, the create call refused it"))
        elif "refused" in r:
            bad.append((c, "refused: " + r["refused"]))
        elif {k: r.get(k) for k in w} != w:
            bad.append((c, {k: (w[k], r.get(k)) for k in w if w[k] != r.get(k)}))
    assert not bad, (len(bad), bad[:10])


def test_plan_structure(golden):
    """Every accepted plan: the splits cover the partitions with no empty split (plain and batched),
    batched splits hold whole chunks of 32 rows, the ring holds a batch, the layout is [C][ring][B];
    a sparse handle and the dense one of the same shape and options cut the partitions alike."""
    _, cases, _, got = golden
    dense = {}
    n = 0
    for c, r in zip(cases, got):
        if "refused" in r:
            continue
        kind, borrowed, C, B, P, opts = c
        n += 1
        assert r["S"] >= 1 and r["S"] * r["rows"] >= P > (r["S"] - 1) * r["rows"], (c, r)
        assert r["Sb"] >= 1 and r["Sb"] * r["rows_b"] >= P > (r["Sb"] - 1) * r["rows_b"], (c, r)
        assert r["rows_b"] % 32 == 0 and r["S"] <= 64 and r["Sb"] <= 64, (c, r)
        assert r["ring"] >= P + 31, (c, r)
        assert r["cstride"] == r["ring"] * B and r["pstride"] == B, (c, r)
        assert 0 <= r["pc"] <= P and 0 <= r["pcb"] <= P, (c, r)
        if kind == "sparse":
            assert (r["batch"], r["ring"], r["ahead"], r["off"], r["off_nseg"], r["levels"], r["nseg"], r["pc"], r["pcb"]) == \
                (0, P + 31, 0, 0, 0, 0, 0, 0, 0), (c, r)
        if kind == "dense" and not borrowed and (opts is None or opts[2:] == [0, 0, -1, -1, 0, 0, 0, 0, 0]):
            dense[(C, B, P, None if opts is None else (opts[0], opts[1]))] = r
    assert n == 546
    twins = 0
    for c, r in zip(cases, got):
        if c[0] != "sparse" or "refused" in r:
            continue
        d = dense.get((c[2], c[3], c[4], None if c[5] is None else (c[5][0], c[5][1])))
        if d is None:
            continue
        twins += 1
        assert all(r[k] == d[k] for k in ("fused", "S", "rows", "Sb", "rows_b")), (c, r, d)
    assert twins >= 130, twins
