"""The LDS-tile Toeplitz walk with 8 outputs per lane (toep_lds_role / t32_walk in
csrc/upols_levels.hip), at the smallest shapes where its geometry changes:

  C = 2,  B = 64,  P = 65, 97        fewer than 256 units: two window parts per unit (2 output
                                     octets x 8 band groups); P = 97 is an odd band of 33
                                     partitions (the FDL columns' 16-byte alignment shift),
                                     P = 65 a band of one (the single-partition tail alone)
  C = 64, B = 64,  P = 100, 256, 300 exactly 256 units: one part (4 octets x 4 band groups), a
                                     short band, the full 192-wide band, and the far level
  C = 3,  B = 256, P = 130           bin 0 (packed DC / Nyquist) in one unit of sixteen
  C = 4,  B = 256, P = 300           the shapes part_plan is tested at, step groups of 4 and
                                     one launch per step

Every shape streams 200 single-block steps (more than 3 windows of every level after priming,
and past one far window where P > 256) and is checked three ways: against the oracle's
dense_convolve, against the same handle's plain step (set_ahead(False)), both at the project's
bar of 1e-5 peak-normalised, and two identical runs bit for bit."""
import numpy as np
import pytest

from conftest import peak_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
STEPS = 200

SHAPES = [
    (2, 64, 65, {}),
    (2, 64, 97, {}),
    (64, 64, 100, {}),
    (64, 64, 256, {}),
    (64, 64, 300, {}),
    (3, 256, 130, {}),
    (4, 256, 300, {"step_group": 4}),
    (4, 256, 300, {"step_group": 1}),
]
_ref = {}  # (C, B, P) -> (filter partitions, signal, oracle output): computed once, never written to


def _case(oracle, C, B, P):
    key = (C, B, P)
    if key not in _ref:
        L = B * (P - 1) + B // 2 + 1
        ir = np.stack([oracle.noise(7000 + 13 * P + c, L) for c in range(C)])
        parts = oracle.uniform_partition(oracle.normalize_impulse(ir), B)
        assert parts.shape[1] == P
        sig = np.stack([oracle.noise(7500 + 17 * P + c, B * STEPS) for c in range(C)])
        ref = oracle.dense_convolve(sig, parts)
        for a in (parts, sig, ref):
            a.setflags(write=False)
        _ref[key] = (parts, sig, ref)
    return _ref[key]


def _stream(conv, sig, torch):
    t = torch.from_numpy(sig.copy()).cuda()
    conv.process_blocks(t)  # set_batch(False): one single-block step per block
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("C,B,P,opts", SHAPES)
def test_walk_against_oracle_plain_step_and_itself(neo_gpu, oracle, C, B, P, opts):
    torch = pytest.importorskip("torch")
    parts, sig, ref = _case(oracle, C, B, P)
    conv = neo_gpu.UpolsConvolver(C, B, P, options=opts)
    conv.filter(parts)
    conv.set_batch(False)
    assert conv.ahead_info()[0], "streaming levels off"
    if "step_group" in opts:
        assert conv.step_group() == opts["step_group"]
    first = _stream(conv, sig, torch)
    conv.reset()
    second = _stream(conv, sig, torch)
    conv.reset()
    conv.set_ahead(False)
    plain = _stream(conv, sig, torch)
    conv.close()
    # the largest error of any sample of any of the 200 blocks, over the reference's peak
    e_oracle, e_plain = peak_err(first, ref), peak_err(first, plain)
    print(f"C={C} B={B} P={P} {opts}: oracle {e_oracle:.3e} plain step {e_plain:.3e}")
    assert e_oracle < TOL
    assert e_plain < TOL
    assert np.array_equal(first, second), "two identical runs differ"
