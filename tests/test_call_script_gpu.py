"""The seeded call scripts of tests/call_script.py on the device: every way a handle of the four
families runs a block, joined by the state one route hands to the next (the delay-line ring and its
wrap, the previous block or the overlap-add tail, the partly summed level windows and their priming,
the second filter bank and the fade counter).

Reference: call_script.model, numpy float64 (tests/test_call_script.py pins it to the oracle and to
np.convolve without a GPU). Error: the maximum over channels and epochs (stretches between
state-clearing events) of max|y - truth| over that channel's truth peak in that epoch; epochs
shorter than 4 blocks take the whole run's peak. Bars: the project's, 1e-5 for the float32 families,
1e-12 for the double family.

Per script: values; fade_info()["remaining_blocks"] after every event against the model's; every
refused update raises NeoHipError (and the rest of the run meets the bar); a second fresh handle
gives the same bits; a third handle that plays only the events before the first mode-changing event
gives the bits of those blocks (nothing later reaches back).

Worst measured errors (MI355X), per family over its shapes and seeds:
    dense   2.98e-07  (28 scripts; every one between 2.0e-07 and 3.0e-07)
    sparse  3.07e-07  (32 scripts)
    matrix  3.09e-07  (16 scripts)
    f64     9.34e-16  (16 scripts)
Each script takes about 0.2 s (three handles of up to about 1000 blocks and the model)."""
import numpy as np
import pytest

import call_script as cs

pytestmark = pytest.mark.gpu
TOL = {"dense": 1e-5, "sparse": 1e-5, "matrix": 1e-5, "f64": 1e-12}

CASES = cs.all_scripts()
IDS = [f"{cs.shape_name(fam, k)}-seed{seed}" for fam, k, seed in CASES]


def check(neo, torch, s):
    m = cs.model(s)
    y, remaining, refused = cs.run(neo, torch, s)
    err = cs.script_error(y, m)
    print(f"{s.name}: {s.nblocks} blocks, {len(s.events)} events, {len(m.epochs)} epochs, {len(m.walk.fades)} fades: "
          f"err {err:.3g}")
    assert np.isfinite(y).all(), s.name
    assert err <= TOL[s.family], (s.name, err)
    assert remaining == m.remaining, (s.name, [(e, s.events[e], a, b) for e, (a, b) in
                                              enumerate(zip(remaining, m.remaining)) if a != b][:5])
    assert refused == sum(ev[0] == "refused_update" for ev in s.events), s.name
    y2, remaining2, _ = cs.run(neo, torch, s)
    assert remaining2 == remaining
    assert np.array_equal(y2.view(np.uint8), y.view(np.uint8)), f"{s.name}: a second fresh handle gives other bits"
    events, blocks = s.prefix()
    y3, _, _ = cs.run(neo, torch, s, events=events)
    assert y3.shape[1] == blocks * s.B
    assert np.array_equal(y3.view(np.uint8), np.ascontiguousarray(y[:, :blocks * s.B]).view(np.uint8)), \
        f"{s.name}: the {blocks} blocks before the first mode event differ when nothing follows them"
    return err


@pytest.mark.parametrize("case", CASES + sorted(cs.REGRESSIONS), ids=IDS + sorted(cs.REGRESSIONS))
def test_script(neo_gpu, case):
    """a committed seed's script, or a named regression case (call_script.REGRESSIONS)"""
    import torch

    check(neo_gpu, torch, cs.REGRESSIONS[case] if isinstance(case, str) else cs.script(*case))
