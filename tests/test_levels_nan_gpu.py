"""A bad input block leaves the dense handle's streaming levels.

One block of one channel is NaN. Channels never meet, so the other channels must equal the clean run
bit for bit. The poisoned channel is NaN for as long as the filter reaches, blocks [at, at + P): every
partition of the noise filter is nonzero. After that the exact sum has no NaN term left, but the
levels keep state of their own, and how long that may hold the NaN is derived here from the plan:

  * the block role (partitions < 8) and the Toeplitz levels (windows of 4 .. 32 blocks, and the
    128-block level of far_level = 0) multiply the FDL row t - p by partition p of their band only.
    toep_role also multiplies by the zero it reads for a filter row past its band's end, but such
    a row stands for a partition below 256 < P, and the 128-block level's tile takes the rows of
    its band [256, P) alone: their slabs are clean from block at + P on.
  * the far level transforms along the block axis: the window that starts at block s multiplies the
    spectrum of segment j < nseg by the transform of the 256 FDL rows [s - F - 128 (j + 1),
    s - F - 128 (j - 1)) (F the level's first partition: 256 aligned, plan_levels_stag's farA
    staggered; stored in the row-pair ring, in phase 1's partial sums, or recomputed -- the same
    rows), and a NaN row poisons all 256 points of its pair and through them the window's 128
    blocks, whatever the filter holds there. Row `at` is in a pair of window s up to
    s <= at + F + 128 nseg, so the last poisoned block is before at + F + 128 nseg + 128. Both
    plans have F + 128 nseg < P + 128 (nseg is the least number of segments that covers [F, P)),
    which gives at + P + 256. A class's window phase (staggered) moves s, not this bound.

So from block at + P + 256 on the channel is finite and equal to the clean run bit for bit: the
same launches on the same values. A NaN that stays longer is state that was not rewritten."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C, B, P, AT = 3, 64, 450, 21
NB = AT + P + 256 + 70
BAD_CHANNEL = 1
FORMS = [{"step_group": 1}, {"step_group": 4, "windows": 1}, {"step_group": 4, "windows": 2},
         {"step_group": 4, "far_level": 0}, {"step_group": 4, "far_level": 2}]


def stream(neo, torch, opts, parts, sig):
    conv = neo.UpolsConvolver(C, B, P, options=opts)
    assert conv.step_group() == opts["step_group"] and conv.windows() == opts.get("windows", 1)
    assert conv.ahead_info()[0], "streaming levels off"
    conv.filter(parts)
    conv.set_batch(False)
    t = torch.from_numpy(sig).cuda()
    conv.process_blocks(t)
    conv.join_background(None)
    torch.cuda.synchronize()
    out = t.cpu().numpy()
    conv.close()
    return out


@pytest.fixture(scope="module")
def case(oracle):
    ir = np.stack([oracle.noise(3100 + c, B * P) for c in range(C)])
    parts = oracle.uniform_partition(oracle.normalize_impulse(ir), B)
    sig = np.stack([oracle.noise(3150 + c, B * NB) for c in range(C)])
    bad = np.array(sig)
    bad[BAD_CHANNEL, AT * B:(AT + 1) * B] = np.nan
    return parts, sig, bad


@pytest.mark.parametrize("opts", FORMS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_nan_block_leaves_the_levels(neo_gpu, oracle, case, opts):
    torch = pytest.importorskip("torch")
    parts, sig, bad = case
    clean = stream(neo_gpu, torch, opts, parts, sig)
    assert np.isfinite(clean).all()
    y = stream(neo_gpu, torch, opts, parts, bad)
    others = [c for c in range(C) if c != BAD_CHANNEL]
    assert np.array_equal(y[others].view(np.uint32), clean[others].view(np.uint32)), "a channel beside the NaN block"
    yb, cb = y[BAD_CHANNEL], clean[BAD_CHANNEL]
    assert np.array_equal(yb[:AT * B].view(np.uint32), cb[:AT * B].view(np.uint32)), "before the NaN block"
    assert np.isnan(yb[AT * B:(AT + P) * B]).all(), "the filter's reach"
    end = (AT + P + 256) * B
    last = np.nonzero(~np.isfinite(yb))[0].max() // B
    print(f"nan block {AT}, P {P}, {opts}: the last block that is not finite is {last} (bound {AT + P + 256})")
    assert np.isfinite(yb[end:]).all(), f"not finite at block {last}"
    assert np.array_equal(yb[end:].view(np.uint32), cb[end:].view(np.uint32)), "clean again"
