"""The reference model of the scripted group tests (group_script.model: one oracle.Upols per
member) against float64 truth, on every script test_group_midframe_gpu.py plays: for each member the
linear convolution, in float64, of its input since its last filter or reset with its normalised
impulse response. The truth takes the in-place rule in its other form -- a filter or reset of a
member made between the frame's first call and that member's own call of the frame is MOVED behind
that call -- while the model computes the pending members' outputs at the frame's first call, so
the two agree only if the model's bookkeeping is the documented one. Bar: the project's 1e-5 on the
per-member max error over the run / the per-member peak of the truth (the oracle itself is recorded
at <= 4.9e-7 against such truth, tests/golden/manifest.json). No GPU."""
import numpy as np
import pytest

import group_script as gs


def _effective(script, events, members):
    """the frame's events in the order they take effect; members: those there when the frame began"""
    if script.mode != "in_place":
        return list(events)
    calls = [k for k, ev in enumerate(events) if ev[0] == "call"]
    out, held = [], {}
    for k, ev in enumerate(events):
        late = calls and k > calls[0] and ev[0] in ("filter", "reset") and ev[1] in members
        if late and any(e[0] == "call" and e[1] == ev[1] for e in events[k:]) and \
                not any(e[0] == "call" and e[1] == ev[1] for e in events[:k]):
            held.setdefault(ev[1], []).append(ev)  # its block was consumed at the frame's first call
            continue
        out.append(ev)
        if ev[0] == "call":
            out += held.pop(ev[1], [])
    assert not held
    return out


def _truth(script):
    """member -> float64 samples of every block its calls return, in order"""
    seg = {}  # member -> [impulse, [blocks since the last filter or reset]]
    out = {}

    def flush(m):
        ir, blocks = seg[m]
        if blocks:
            x = np.concatenate(blocks).astype(np.float64)
            n = 1 << int(np.ceil(np.log2(len(x) + len(ir))))
            y = np.fft.irfft(np.fft.rfft(x, n) * np.fft.rfft(ir.astype(np.float64), n), n)[:len(x)]
            out.setdefault(m, []).append(y)
        seg[m] = [ir, []]

    for events in script.frames:
        for ev in _effective(script, events, set(seg)):
            if ev[0] == "call":
                seg[ev[1]][1].append(ev[2])
            elif ev[0] == "filter":
                if ev[1] in seg:
                    flush(ev[1])
                seg[ev[1]] = [script.impulse_of(ev[2]), []]
            elif ev[0] == "reset":
                flush(ev[1])
            elif ev[0] == "leave":
                flush(ev[1])
                del seg[ev[1]]
    for m in list(seg):
        flush(m)
    return {m: [np.concatenate(v)] for m, v in out.items()}


@pytest.mark.parametrize("case", gs.CASES, ids=gs.case_id)
def test_model_matches_float64_truth(oracle, case):
    script, _ = gs.build(oracle, case)
    ref = gs.model(oracle, script)
    truth = _truth(script)
    assert set(ref) == set(truth)
    worst = gs.worst_error(ref, truth)
    print(f"{gs.case_id(case)}: model vs float64 truth {worst:.3e}")
    assert worst <= 1e-5, worst


def test_in_place_blocks_are_consumed_at_the_first_call(oracle):
    """The in-place rule spelled out on one script: a pending member's filter change in mid-frame
    leaves its output of that frame the OLD filter's (its block was consumed), the new filter starts
    from zero state with its next frame; the same script under a plain registration gives the new
    filter's output at once."""
    case = gs.Case("small", "upols", "in_place", "filter", "pending", 4)
    script, (f, _) = gs.build(oracle, case)
    t = gs.TARGETS["pending"]
    blocks = {fr: gs.first_calls(ev)[t] for fr, ev in enumerate(script.frames)}
    old, new = script.frames[0][t][2], script.frames[f][2][2]
    assert script.frames[0][t][:2] == ("filter", t) and script.frames[f][2][:2] == ("filter", t)
    a = oracle.Upols(old)
    expect = [a(blocks[fr]) for fr in range(f + 1)]
    b = oracle.Upols(new)
    expect += [b(blocks[fr]) for fr in range(f + 1, len(script.frames))]
    got = gs.model(oracle, script)[t]
    assert all(np.array_equal(x, y) for x, y in zip(got, expect)) and len(got) == len(expect)
    plain = gs.Script(script.members, script.block, "upols", "plain", script.frames, script.impulses)
    b = oracle.Upols(new)
    expect = expect[:f] + [b(blocks[fr]) for fr in range(f, len(script.frames))]
    got = gs.model(oracle, plain)[t]
    assert all(np.array_equal(x, y) for x, y in zip(got, expect)) and len(got) == len(expect)
