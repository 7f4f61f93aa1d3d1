"""Scripted runs of a convolver group (neo_hip_upols_group_*, neo.UpolsGroup) and their CPU
reference. A plain module: test_group_model.py (no GPU) and test_group_midframe_gpu.py import it.

A Script is a list of frames; a frame is an ordered list of events
    ("call", member, block)    the member's call on a block [B] float32 (the input it holds)
    ("filter", member, parts)  a new filter [P][B+1] (restarts the member's state)
    ("reset", member)
    ("join",)                  a new member; it takes the next index
    ("leave", member)
plus the registration mode ("plain": one registered buffer per member; "frame_stable" / "in_place":
one registered [C][B] array with that promise, member c always on row c) and the method. Members
are numbered 0 .. members - 1 from the start. As the plugin does, the owner fills every member's
buffer with the block of its first call of the frame BEFORE the frame's first call; the block of a
second call of a member in the same frame goes into its buffer right before that call.

run(group, script)    plays the script on a UpolsGroup and records what every call returned.
model(oracle, script) plays it on one oracle.Upols per member (replaced on filter, rebuilt from the
                      same filter on reset): the reference; it never touches the library under test.

Plain and frame_stable: events apply in script order. in_place: a frame's blocks are consumed at its
first call, and a state change in mid-frame takes effect after them -- at the frame's first call
every member that has its call of the frame still to make consumes its frame block; a filter or
reset of such a member later in the frame acts on the state AFTER that block, and the member's
remaining call of the frame, on its frame block, is a no-op that returns the output computed then.
(That is what a group in the one-launch mode does; on a handle per member the blocks are consumed
call by call, which gives the same outputs for every frame without a state change in its middle.
The scripts therefore break only frames the group runs in one launch, and the tests assert that.)"""
from collections import namedtuple

import numpy as np

MODES = ("plain", "frame_stable", "in_place")


class Script:
    def __init__(self, members, block, method, mode, frames, impulses):
        assert mode in MODES and method in ("upols", "upola")
        self.members, self.block, self.method, self.mode = members, block, method, mode
        self.frames = frames
        self.impulses = impulses  # [(parts, normalised impulse response)]: what each filter came from

    def impulse_of(self, parts):
        for p, ir in self.impulses:
            if p is parts:
                return ir
        raise KeyError("filter without an impulse response")

    def members_total(self):
        return self.members + sum(ev[0] == "join" for fr in self.frames for ev in fr)


def first_calls(events):
    """member -> block of its first call in the frame"""
    first = {}
    for ev in events:
        if ev[0] == "call" and ev[1] not in first:
            first[ev[1]] = ev[2]
    return first


class Run:
    """What run() saw: calls[(frame, event)] = the block that call returned, stats[(frame, event)] =
    group.stats() after that event, frame_stats[frame] = before its first event (one more entry:
    after the last frame), snap = a copy of every member's buffer after the event at `snap_at`."""

    def __init__(self):
        self.calls, self.stats, self.frame_stats, self.snap = {}, {}, [], None

    def outputs(self, script):
        out = {}
        for f, events in enumerate(script.frames):
            for k, ev in enumerate(events):
                if ev[0] == "call":
                    out.setdefault(ev[1], []).append(self.calls[(f, k)])
        return out


def run(group, script, snap_at=None):
    B, n = script.block, script.members_total()
    if script.mode == "plain":
        bufs = [np.zeros(B, np.float32) for _ in range(n)]
        for b in bufs:
            group.register(b)
    else:
        frame = np.zeros((n, B), np.float32)
        group.register(frame, frame_stable=True, in_place=script.mode == "in_place")
        bufs = [frame[c] for c in range(n)]
    ids = [group.join() for _ in range(script.members)]
    r = Run()
    for f, events in enumerate(script.frames):
        r.frame_stats.append(group.stats())
        for m, blk in first_calls(events).items():  # the owner fills the frame, then loops over the members
            bufs[m][:] = blk
        called = set()
        for k, ev in enumerate(events):
            if ev[0] == "call":
                m = ev[1]
                if m in called:
                    bufs[m][:] = ev[2]
                called.add(m)
                group(ids[m], bufs[m])
                r.calls[(f, k)] = bufs[m].copy()
            elif ev[0] == "filter":
                group.filter(ids[ev[1]], ev[2])
            elif ev[0] == "reset":
                group.reset(ids[ev[1]])
            elif ev[0] == "join":
                ids.append(group.join())
            elif ev[0] == "leave":
                group.leave(ids[ev[1]])
            else:
                raise ValueError(ev[0])
            r.stats[(f, k)] = group.stats()
            if snap_at == (f, k):
                r.snap = np.stack(bufs)
    r.frame_stats.append(group.stats())
    return r


def model(oracle, script):
    """member -> the list of blocks its calls return, from oracle.Upols alone"""
    ola = script.method == "upola"
    conv, filt, out = {}, {}, {}
    for events in script.frames:
        consumed = None  # in_place: member -> output of its frame block, computed at the frame's first call
        for ev in events:
            if ev[0] == "call":
                m, blk = ev[1], ev[2]
                if script.mode == "in_place" and consumed is None:
                    consumed = {c: conv[c](b) for c, b in first_calls(events).items() if c in conv}
                if consumed and m in consumed:
                    y = consumed.pop(m)  # its call of the frame: the block holds its output already
                else:
                    y = conv[m](blk)
                out.setdefault(m, []).append(y)
            elif ev[0] == "filter":
                filt[ev[1]] = ev[2]
                conv[ev[1]] = oracle.Upols(ev[2], ola=ola)
            elif ev[0] == "reset":
                conv[ev[1]] = oracle.Upols(filt[ev[1]], ola=ola)
            elif ev[0] == "join":
                pass  # the new member's filter event brings its convolver
            elif ev[0] == "leave":
                del conv[ev[1]]
                if consumed:
                    consumed.pop(ev[1], None)
            else:
                raise ValueError(ev[0])
    return out


def worst_error(got, ref):
    """max over the members of (max error over the run) / (the member's reference peak)"""
    worst = 0.0
    for m, blocks in ref.items():
        r = np.concatenate(blocks).astype(np.float64)
        g = np.concatenate(got[m]).astype(np.float64)
        assert g.shape == r.shape, m
        worst = max(worst, float(np.abs(g - r).max()) / float(np.abs(r).max()))
    return worst


# ---------------------------------------------------------------------------------------------
# The scripts of the mid-frame tests: whole frames until the group runs one launch per frame, the
# break frame (the trigger after 2 of its calls, so members on both sides of it exist), whole frames
# after it (a stale ring row or previous block shows there, not only in the break frame).
Case = namedtuple("Case", "shape method mode trigger target at")
SHAPES = {  # members, block, partitions, whole frames after the break
    "small": (6, 128, 150, 4),  # no step groups
    "steps": (64, 512, 100, 4),  # step groups of 4 (2048 16-column units)
    "far": (4, 128, 300, 12),  # the far level contributes (P > 256); its re-primed window needs frames
}
TARGETS = {"pending": 3, "committed": 1, "leader": 0}  # after calls of members 0 and 1


def _matrix(shape, method, modes, at):
    out = []
    for mode in modes:
        out += [Case(shape, method, mode, t, None, at) for t in ("second_leader", "second_committed", "join")]
        out += [Case(shape, method, mode, t, who, at) for t in ("filter", "reset", "leave") for who in TARGETS]
    return out


CASES = (
    _matrix("small", "upols", MODES, 4)
    + _matrix("small", "upola", ("plain", "in_place"), 4)
    + [Case("steps", "upols", mode, trig, who, at) for mode in ("plain", "in_place")
       for trig, who in (("filter", "pending"), ("second_leader", None)) for at in (4, 5, 6, 7)]
    + [Case("far", "upols", "in_place", "reset", "pending", 4)]
)


def case_id(c):
    return "-".join(str(x) for x in c if x is not None)


_filters = {}


def filters(oracle, shape):
    """(C + 2 filters [P][B + 1], their normalised impulses [C + 2][L]) of a shape, made once: a
    filter per member and two spare ones (a filter change, a joining member)"""
    if shape not in _filters:
        C, B, P, _ = SHAPES[shape]
        seed = 3000 + 100 * sorted(SHAPES).index(shape)
        ir = oracle.normalize_impulse(np.stack([oracle.noise(seed + c, B * P) for c in range(C + 2)]))
        _filters[shape] = (list(oracle.uniform_partition(ir, B)), ir)
    return _filters[shape]


def build(oracle, case):
    """the case's Script and the (frame, event) of its trigger"""
    C, B, P, after = SHAPES[case.shape]
    parts, ir = filters(oracle, case.shape)
    assert parts[0].shape == (P, B + 1)
    rng = np.random.default_rng(7 + CASES.index(case))
    live = list(range(C))

    def blk():
        return rng.random(B, dtype=np.float32) - np.float32(0.5)

    frames = []
    for f in range(case.at):
        pre = [("filter", c, parts[c]) for c in live] if f == 0 else []
        frames.append(pre + [("call", c, blk()) for c in live])
    t = TARGETS.get(case.target)
    brk = [("call", 0, blk()), ("call", 1, blk())]
    rest = live[2:]
    if case.trigger == "second_leader":
        brk.append(("call", 0, blk()))
    elif case.trigger == "second_committed":
        brk.append(("call", 1, blk()))
    elif case.trigger == "filter":
        brk.append(("filter", t, parts[C]))
    elif case.trigger == "reset":
        brk.append(("reset", t))
    elif case.trigger == "join":
        brk += [("join",), ("filter", C, parts[C + 1])]
        rest = rest + [C]
        live = live + [C]
    elif case.trigger == "leave":
        brk.append(("leave", t))
        rest = [c for c in rest if c != t]
        live = [c for c in live if c != t]
    else:
        raise ValueError(case.trigger)
    frames.append(brk + [("call", c, blk()) for c in rest])
    for _ in range(after):
        frames.append([("call", c, blk()) for c in live])
    impulses = [(parts[c], ir[c]) for c in range(C + 2)]
    return Script(C, B, case.method, case.mode, frames, impulses), (case.at, 2)
