"""A group's state changes in the middle of a frame (upols_group.hip, split()): while members
still have their call of a one-launch frame to make, a member is called a second time, takes a new
filter, is reset, joins or leaves. Every member's outputs must stay its own sequential convolver's
(the group's contract, test_group_gpu.py), under every registration: plain and frame_stable roll the
members the leader stepped ahead back one block; under in_place their inputs are gone -- a frame's
blocks are consumed at its first call, and a state change in mid-frame takes effect after them.

Each case plays a script (group_script.py) on a UpolsGroup and on the CPU reference model
(oracle.Upols per member, checked against float64 truth in test_group_model.py): whole frames until
the group runs one launch per frame, the break frame with the trigger after 2 of its calls, whole
frames after it. Measure: per member, max error over all frames / that member's reference peak;
bar 1e-5 (test_group_gpu.py, BASELINE.json)."""
import numpy as np
import pytest

import group_script as gs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def step_group_checked(neo_gpu):
    """the "steps" shape really runs step groups of 4 in the shared handle"""
    C, B, P, _ = gs.SHAPES["steps"]
    probe = neo_gpu.UpolsConvolver(C, B, P)
    g = probe.step_group()
    probe.close()
    return g


@pytest.mark.parametrize("case", gs.CASES, ids=gs.case_id)
def test_group_midframe(neo_gpu, oracle, case, request):
    if case.shape == "steps":
        assert request.getfixturevalue("step_group_checked") == 4
    script, (f, k) = gs.build(oracle, case)
    ref = gs.model(oracle, script)
    g = neo_gpu.UpolsGroup(script.block, gs.SHAPES[case.shape][2], method=case.method)
    r = gs.run(g, script, snap_at=(f, k))
    final = g.stats()
    g.close()
    worst = gs.worst_error(r.outputs(script), ref)
    print(f"{gs.case_id(case)}: worst member error / peak {worst:.3e}")

    # the break hit a one-launch frame, switched the mode once and re-ran no block
    before = r.stats[(f, k - 1)]
    after = r.stats[(f, k)]
    assert r.frame_stats[f]["coalesced"] and before["coalesced"], (r.frame_stats[f], before)
    assert before["frame_steps"] == r.frame_stats[f]["frame_steps"] + 1, before
    assert not after["coalesced"], after
    assert after["switches"] == before["switches"] + 1, (before, after)
    assert r.frame_stats[f + 1]["switches"] == before["switches"] + 1, r.frame_stats[f + 1]
    assert after["redos"] == before["redos"] == r.frame_stats[f + 1]["redos"], (before, after, r.frame_stats[f + 1])

    events = script.frames[f]
    if case.mode == "in_place":
        # a member that had its call of the frame still to make: that call leaves its block as the
        # leader's step wrote it
        early = {ev[1] for ev in events[:k + 1] if ev[0] == "call"}
        joined = set(range(script.members, script.members_total()))
        late = [(j, ev[1]) for j, ev in enumerate(events) if j > k and ev[0] == "call" and ev[1] not in early | joined]
        assert len(late) >= 2
        for j, m in late:
            assert np.array_equal(r.calls[(f, j)], r.snap[m]), (j, m)

    if case.trigger == "leave":
        # the others are in step and keep their buffers: call_independent wants two good complete
        # frames, so at the latest after the third whole frame following the break it is one launch
        # per frame again
        assert r.frame_stats[f + 4]["coalesced"], [s["coalesced"] for s in r.frame_stats]
        assert final["coalesced"] and final["switches"] == before["switches"] + 2, final
        # sooner, in fact: the frame under observation goes on across the split, and under in_place
        # the remaining members' calls of the break frame (nothing left to do) count as their calls
        # of it, so the break frame is the first good frame and the next whole frame the second
        assert r.frame_stats[f + 2]["coalesced"], [s["coalesced"] for s in r.frame_stats]

    assert worst <= 1e-5, worst


def test_group_midframe_in_place_foreign_buffer(neo_gpu, oracle):
    """The in-place promise broken after a split in mid-frame: a member whose frame block the
    leader's step consumed is called on ANOTHER buffer. Its frame block keeps the output of the
    block it held, and the block it brings is stepped as a new one (one block more than the other
    members from then on); every member still equals its own sequential convolver."""
    C, B, P, _ = gs.SHAPES["small"]
    parts, _ = gs.filters(oracle, "small")
    rng = np.random.default_rng(77)
    g = neo_gpu.UpolsGroup(B, P)
    frame = np.zeros((C, B), np.float32)
    g.register(frame, in_place=True)
    ids = [g.join() for _ in range(C)]
    ref = [oracle.Upols(parts[c]) for c in range(C)]
    for c in range(C):
        g.filter(ids[c], parts[c])
    got, expect = [], []

    def whole_frame():
        x = rng.random((C, B), dtype=np.float32) - np.float32(0.5)
        frame[:] = x
        for c in range(C):
            g(ids[c], frame[c])
        got.append(frame.copy())
        expect.append(np.stack([ref[c](x[c]) for c in range(C)]))

    for _ in range(4):
        whole_frame()
    assert g.stats()["coalesced"]
    x = rng.random((C, B), dtype=np.float32) - np.float32(0.5)
    frame[:] = x
    g(ids[0], frame[0])
    g(ids[1], frame[1])
    g.reset(ids[0])  # the one-launch mode ends; members 2.. hold their outputs already
    assert not g.stats()["coalesced"]
    y = np.stack([ref[c](x[c]) for c in range(C)])
    ref[0] = oracle.Upols(parts[0])
    odd = rng.random(B, dtype=np.float32) - np.float32(0.5)
    y_odd = ref[2](odd)
    g(ids[2], odd)
    for c in range(3, C):
        g(ids[c], frame[c])
    got += [frame.copy(), odd[None].copy()]
    expect += [y, y_odd[None]]
    for _ in range(4):
        whole_frame()
    g.close()
    # per member: max error over the run / its reference peak (member 2's extra block is its own row)
    err = np.max([np.abs(a - b).max(axis=1) for a, b in zip(got, expect) if len(b) == C], axis=0)
    peak = np.max([np.abs(b).max(axis=1) for b in expect if len(b) == C], axis=0)
    err[2] = max(err[2], float(np.abs(got[5] - expect[5]).max()))
    worst = float((err / peak).max())
    print(f"in_place foreign buffer: worst member error / peak {worst:.3e}")
    assert worst <= 1e-5, worst
