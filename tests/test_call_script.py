"""The call scripts of tests/call_script.py without a GPU: their float64 model against the oracle
(float32 families) and against np.convolve (double family), and the coverage conditions that the
committed seed lists must meet. The conditions are asserted from the scripts alone (call_script.walk);
a seed list that stops meeting one fails here, before a GPU sees it.

Oracle check: every float32 script is played on oracle.Upols instances, one per bank and channel
(per route for the matrix family), rebuilt at every filter and reset event and fed the whole stretch
since; the two banks are mixed in float64 with the model's gains. Bar: 1e-5 of the per-epoch,
per-channel peak (call_script.script_error). The oracle computes in float32, the model in float64:
the bar is the project's float32 bar. Double scripts: np.convolve of every epoch's input with the
bank's impulse response, 1e-13 (upols_f64_truth.TRUTH_AGREE)."""
import numpy as np
import pytest

import call_script as cs

SHAPE_IDS = [(fam, k) for fam in cs.FAMILIES for k in range(len(cs.SHAPES[fam]))]
ALL = cs.all_scripts()
FLOAT32 = [p for p in ALL if p[0] != "f64"]
DOUBLE = [p for p in ALL if p[0] == "f64"]


def sid(p):
    return cs.shape_name(*p[:2]) + (f"-seed{p[2]}" if len(p) > 2 else "")


def scripts_of(fam, k):
    return [cs.script(fam, k, seed) for seed in cs.SEEDS[(fam, k)]]


# ------------------------------------------------------------------------------ model vs oracle
def oracle_play(oracle, s, m):
    """[outputs][n] float64: the script on oracle.Upols instances, mixed with the model's gains"""
    B, ola = s.B, s.method == "upola"
    H = [np.asarray(h * k, dtype=np.complex64) for h, k in zip(s.filters(), s.masks())] if s.family == "sparse" else s.filters()
    x = s.signal()
    rows = [(o, i) for o, i in s.routes] if s.family == "matrix" else [(c, c) for c in range(s.inputs)]
    y = np.zeros((s.outputs, s.nblocks * B))
    for a, b in m.epochs:
        used = {}  # filter -> blocks of the epoch its instance is fed
        for t in range(a, b):
            for f in m.walk.blocks[t][1:3]:
                if f is not None:
                    used[f] = t + 1 - a
        bank = {}
        for f, n in used.items():
            out = np.zeros((s.outputs, n * B))
            for r, (o, i) in enumerate(rows):
                out[o] += oracle.Upols(H[f][r], ola=ola).run(x[i, a * B:(a + n) * B]).astype(np.float64)
            bank[f] = out
        for t in range(a, b):
            _, fa, fb, k, F, curve = m.walk.blocks[t]
            q = slice((t - a) * B, (t - a + 1) * B)
            ya = bank[fa][:, q]
            if fb is not None:
                ya = ya + cs.gains(B, F, k, curve) * (bank[fb][:, q] - ya)
            y[:, t * B:(t + 1) * B] = ya
    return y


@pytest.mark.parametrize("fam,k,seed", FLOAT32, ids=[sid(p) for p in FLOAT32])
def test_model_agrees_with_the_oracle(oracle, fam, k, seed):
    s = cs.script(fam, k, seed)
    m = cs.model(s)
    assert m.remaining == cs.walk(s).remaining and len(m.remaining) == len(s.events)
    err = cs.script_error(oracle_play(oracle, s, m), m)
    print(f"{s.name}: {s.nblocks} blocks, {len(m.epochs)} epochs, oracle against model {err:.3g}")
    assert err <= 1e-5, (s.name, err)


@pytest.mark.parametrize("fam,k,seed", DOUBLE, ids=[sid(p) for p in DOUBLE])
def test_double_model_agrees_with_np_convolve(fam, k, seed):
    s = cs.script(fam, k, seed)
    m = cs.model(s)
    assert not any(m.remaining)
    irs = cs._filters(s.family, s.dims)[1]
    x, B = s.signal(), s.B
    y = np.zeros_like(m.y)
    for a, b in m.epochs:
        f = m.walk.blocks[a][1]
        assert all(blk[1] == f and blk[2] is None for blk in m.walk.blocks[a:b])
        for c in range(s.inputs):
            y[c, a * B:b * B] = np.convolve(x[c, a * B:b * B], irs[f][c])[:(b - a) * B]
    err = cs.script_error(y, m)
    print(f"{s.name}: np.convolve against model {err:.3g}")
    assert err <= 1e-13, (s.name, err)


def test_sparse_masks_thin_the_filters_and_differ():
    for k in range(len(cs.SHAPES["sparse"])):
        s = scripts_of("sparse", k)[0]
        kept = [float(m.mean()) for m in s.masks()]
        assert all(0.02 < d < 0.98 for d in kept), kept  # neither everything nor nothing is kept
        assert kept[1] < kept[0] and kept[1] < kept[2]   # -20 dB keeps less than -40 dB


# -------------------------------------------------------------------------- coverage conditions
class Facts:
    """What the conditions read, from the walks of a shape's scripts."""

    def __init__(self, fam, k):
        self.cap = cs.capabilities(fam, k)
        self.P = cs.SHAPES[fam][k]["dims"][-1]
        self.fades, self.calls, self.clears, self.toggles, self.refused = [], [], [], [], 0
        for s in scripts_of(fam, k):
            w = cs.walk(s)
            modes = dict(self.cap["modes"])
            fade_of = {f["event"]: f for f in w.fades}
            for e, ev in enumerate(s.events):
                at = w.at[e]
                if ev[0] in cs.MODE_EVENTS:
                    assert ev[0] in modes, (s.name, ev)
                    if modes[ev[0]] != ev[1]:
                        self.toggles.append((ev[0], ev[1], at["since"]))
                    modes[ev[0]] = ev[1]
                elif ev[0] == "update":
                    assert at["left"] == 0, (s.name, e)  # only legal sequences
                    nxt = next(x for x in s.events[e + 1:] if x[0] in ("blocks", "filter", "reset"))
                    f = fade_of[e]
                    f["levels"] = bool(self.cap["levels"]) and modes[self.cap["levels"]]
                    f["how"] = nxt[2] if nxt[0] == "blocks" else None
                    f["script"] = s.name
                    self.fades.append(f)
                elif ev[0] == "refused_update":
                    assert at["left"] > 0, (s.name, e)
                    self.refused += 1
                elif ev[0] in ("filter", "reset"):
                    self.clears.append((ev[0], at["left"], at["since"]))
                elif ev[0] == "blocks" and ev[2] == "call":
                    # (a dense handle's offline windows take batching as well)
                    offline = modes.get("offline", False) and (fam != "dense" or modes["batch"])
                    self.calls.append(dict(n=ev[1], block=at["block"], left=at["left"], offline=offline, script=s.name))


@pytest.mark.parametrize("fam,k", SHAPE_IDS, ids=[sid(p) for p in SHAPE_IDS])
def test_seed_list_has_four_seeds_and_every_script_is_in_budget(fam, k):
    seeds = cs.SEEDS[(fam, k)]
    assert len(seeds) == 4 and {seed % 4 for seed in seeds} == {0, 1, 2, 3}  # one seed per scene set of make_script
    for s in scripts_of(fam, k):
        B, small = s.B, fam == "sparse" and s.B == 512
        assert B <= 128 or small
        assert s.nblocks <= (200 if small else 1100), (s.name, s.nblocks)
        events, blocks = s.prefix()
        assert 1 <= blocks < s.nblocks, (s.name, "the prefix before the first mode event must hold blocks, and not all")
        for ev in s.events:
            assert fam != "f64" or ev[0] not in ("update", "refused_update", "ahead", "levels")
            assert ev[0] != "ahead" or fam == "dense"
            assert ev[0] != "levels" or fam == "matrix"


LEVELS = [p for p in SHAPE_IDS if cs.capabilities(*p)["levels"]]
FADING = [p for p in SHAPE_IDS if cs.capabilities(*p)["fades"]]


@pytest.mark.parametrize("fam,k", LEVELS, ids=[sid(p) for p in LEVELS])
def test_fades_of_shapes_with_streaming_levels(fam, k):
    """counted: fades that start with the levels on and run one block per call"""
    F = Facts(fam, k)
    live = [f for f in F.fades if f["levels"] and f["how"] == "step"]
    phases = {f["since"] % 32 for f in live}
    assert len(phases) >= 8, sorted(phases)
    assert any(f["end"] is not None and (f["since"] + f["F"]) % 32 == 0 for f in live), "no fade ends on a multiple of 32"
    assert any(f["F"] > 32 and f["end"] is not None for f in live), "no fade longer than a window"
    assert any((f["since"] + f["F"] - 1) // 128 > f["since"] // 128 and f["since"] % 128 and f["end"] is not None
               for f in live), "no fade spans a multiple of 128"
    assert any(f["since"] < F.P for f in live), "no update before block P"
    soon = [(a, b) for a, b in zip(F.fades, F.fades[1:])
            if a["script"] == b["script"] and a["end"] is not None and b in live and 0 <= b["start"] - a["end"] <= 2
            and b["since"] - a["since"] == b["start"] - a["start"]]
    assert soon, "no update within 2 blocks of a fade's last block"


@pytest.mark.parametrize("fam,k", FADING, ids=[sid(p) for p in FADING])
def test_fades_of_every_fading_shape(fam, k):
    F = Facts(fam, k)
    assert any(c["script"] == f["script"] and c["block"] == f["start"] and f["end"] is not None and f["end"] < c["block"] + c["n"]
               for c in F.calls for f in F.fades), "no call spans a fade's start and its end"
    if F.cap["offline"]:  # dense from 128 partitions, matrix
        assert any(c["offline"] and c["left"] > 0 and c["n"] >= c["left"] + 128 for c in F.calls), \
            "no offline call begins with fade blocks left"
    assert any(kind == "reset" and left > 0 for kind, left, _ in F.clears), "no reset with fade blocks left"
    assert any(kind == "filter" and left > 0 for kind, left, _ in F.clears), "no filter with fade blocks left"
    assert F.refused >= 1, "no refused update"
    assert any(kind == "reset" and 0 < since < F.P for kind, _, since in F.clears), "no reset before P blocks have run"


@pytest.mark.parametrize("fam,k", SHAPE_IDS, ids=[sid(p) for p in SHAPE_IDS])
def test_mode_toggles_and_call_lengths(fam, k):
    F = Facts(fam, k)
    for name in F.cap["modes"]:
        for on in (False, True):
            assert any(n == name and o == on and since >= F.P for n, o, since in F.toggles), \
                f"{name} -> {on} never comes with the ring wrapped"
    lengths = [c["n"] for c in F.calls]
    assert any(2 <= n < 8 for n in lengths), "no call of fewer than T blocks"
    assert any(n >= 32 and 1 <= n % 32 <= 7 and n < 128 for n in lengths), "no call of a multiple of T plus a rest"
    if not (fam == "sparse" and cs.SHAPES[fam][k]["dims"][1] == 512):  # 150 blocks in all there (and no offline windows)
        off = [c["n"] for c in F.calls if c["offline"] and not c["left"]] if F.cap["offline"] else lengths
        assert 128 in off and 256 in off, sorted(off)
        assert any(256 + 128 < n < 512 for n in off), "no call of 256 + 128 + a rest"
    if fam == "f64":  # a reset before the ring has filled once: the double family has no fades, the condition stands alone
        assert any(0 < since < F.P for _, _, since in F.clears)


def test_walk_states_the_rules():
    """filter cancels a fade, reset completes it, a mode switch keeps it, a refused update changes nothing"""
    ev = [("blocks", 3, "step"), ("update", 1, 4, "linear"), ("blocks", 1, "step"), ("batch", False), ("refused_update", 2),
          ("blocks", 1, "call"), ("reset",), ("blocks", 2, "step"), ("update", 2, 2, "cosine"), ("blocks", 1, "step"),
          ("filter", 0), ("blocks", 2, "step"), ("update", 1, 2, "linear"), ("blocks", 5, "call")]
    w = cs.walk(cs.Script("dense", 5, "upols", (2, 32, 37), {}, ev, name="rules"))
    assert w.remaining == [0, 4, 3, 3, 3, 2, 0, 0, 2, 1, 0, 0, 2, 0]
    assert w.epochs == [(0, 5), (5, 8), (8, 15)]
    assert [b[1:3] for b in w.blocks] == [(0, None)] * 3 + [(0, 1)] * 2 + [(1, None)] * 2 + [(1, 2)] + [(0, None)] * 2 + \
        [(0, 1)] * 2 + [(1, None)] * 3
    assert [b[3] for b in w.blocks[3:5]] == [0, 1] and w.fades[0]["end"] is None and w.fades[2]["end"] == 12
    g = cs.gains(32, 4, 1, "cosine")
    assert g[0] == pytest.approx(0.5 - 0.5 * np.cos(np.pi * 0.25)) and cs.gains(32, 4, 0, "linear")[0] == 0.0
