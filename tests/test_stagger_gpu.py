"""Staggered level windows (neo_hip_upols_opts.windows = 2) on the GPU: forced at small shapes,
every run compared with the plain step (one pass over the whole filter per block, options levels =
0) of a second handle that is fed the same calls. Each run streams 2 P + 3 * 128 blocks one block
per launch, which crosses every class's first regular window and the ring's wrap, and on its way
-- in mid-window, off the step groups' grid -- switches the paced modes on and off, leaves the
levels for a few plain steps (the background stream joins, the classes prime again), resets, and
loads another filter."""
import numpy as np
import pytest

from conftest import peak_err

pytestmark = pytest.mark.gpu

TOL = 1e-5


def problem(oracle, C, B, P, nb, seed):
    irs = [np.stack([oracle.noise(seed + 7 * k + c, B * P) for c in range(C)]) for k in range(2)]
    parts = [oracle.uniform_partition(oracle.normalize_impulse(ir), B) for ir in irs]
    sig = np.stack([oracle.noise(seed + 50 + c, B * nb) for c in range(C)])
    return parts, sig


def drive(torch, conv, parts, sig, B, P, levels, strided=False):
    """the same calls for both handles; the level-only ones (paced, set_ahead) where `levels`"""
    C, n = sig.shape
    nb = n // B
    conv.filter(parts[0])
    conv.set_batch(False)
    if strided:  # separate input and output buffers with row strides of their own
        ld_in, ld_out = n + 3 * B, n + 5 * B
        x = torch.zeros((C, ld_in), dtype=torch.float32, device="cuda")
        x[:, :n] = torch.from_numpy(sig).cuda()
        y = torch.full((C, ld_out), 7.0, dtype=torch.float32, device="cuda")
    else:
        x = y = torch.from_numpy(sig).cuda()
        ld_in = ld_out = n
    torch.cuda.synchronize()
    pos = [0]

    def go(k):
        k = min(k, nb - pos[0])
        if k > 0:
            o = 4 * B * pos[0]
            conv.process_samples_ptr(x.data_ptr() + o, ld_in, y.data_ptr() + o, ld_out, k * B, True)
            pos[0] += k

    go(P // 3 + 37)          # mid-window, off the group grid
    if levels:
        conv.set_paced(1)
    go(45)
    if levels:
        conv.set_paced(2)
    go(46)
    if levels:
        conv.set_paced(0)
    go(129)
    if levels:
        conv.set_ahead(False)  # a plain-step excursion
    go(5)
    if levels:
        conv.set_ahead(True)
    go(P // 2 + 131)
    conv.reset()
    go(150 + 3)
    conv.filter(parts[1])    # resets the state too
    go(nb)
    torch.cuda.synchronize()
    assert pos[0] == nb
    return y[:, :n].cpu().numpy()


def compare(neo_gpu, oracle, torch, C, B, P, opts, strided=False, method="upols"):
    nb = 2 * P + 3 * 128
    parts, sig = problem(oracle, C, B, P, nb, 2600 + P + B)
    conv = neo_gpu.UpolsConvolver(C, B, P, method=method, options=dict(opts, windows=2))
    assert conv.windows() == 2 and conv.step_group() == opts["step_group"]
    out = drive(torch, conv, parts, sig, B, P, True, strided)
    conv.close()
    plain = neo_gpu.UpolsConvolver(C, B, P, method=method, options={"levels": 0})
    ref = drive(torch, plain, parts, sig, B, P, False)
    plain.close()
    return peak_err(out, ref)


@pytest.mark.parametrize("C,B,P,G,K", [
    (2, 64, 450, 4, 0),    # 2 channels: most of the 32 far classes are empty
    (16, 64, 938, 4, 0),   # the headline's partitions
    (4, 256, 300, 4, 0),   # one far segment
    (3, 64, 700, 2, 0),    # G = 2: the 8-, 16- and 32-block levels staggered
    (3, 64, 1100, 8, 0),   # G = 8: the 32-block level and the far level
    (5, 64, 700, 4, 2),    # far window groups
    (5, 32, 1100, 4, 3)])
def test_staggered_windows_vs_plain_step(neo_gpu, oracle, C, B, P, G, K):
    torch = pytest.importorskip("torch")
    opts = {"step_group": G, "far_group": K}
    assert compare(neo_gpu, oracle, torch, C, B, P, opts) <= TOL


def test_staggered_windows_strided_io_ola(neo_gpu, oracle):
    torch = pytest.importorskip("torch")
    assert compare(neo_gpu, oracle, torch, 3, 64, 450, {"step_group": 4}, strided=True, method="upola") <= TOL


# (G, P, far_group, levels' windows, last level's band, far level's first partition, nseg): the plan's
# band edges at C = 3, B = 64 (neo.convolution.stagger_plan). G = 4: a = [8, 16, 32, 48], F in [144, 240];
# G = 2: a = [8, 16, 24, 40], F in [136, 232]; G = 8: a = [8, 16, 32, 64], F in [160, 256]
BAND_EDGES = [
    (4, 33, 0, [4, 8, 16], (32, 33), 33, 0),          # the T = 16 band of one partition
    (4, 48, 0, [4, 8, 16], (32, 48), 48, 0),          # the T = 16 band full, no T = 32 level
    (4, 49, 0, [4, 8, 16, 32], (48, 49), 49, 0),      # the T = 32 band of one partition, no far level
    (4, 144, 0, [4, 8, 16, 32], (48, 144), 144, 0),   # the last P without a far level
    (4, 145, 0, [4, 8, 16, 32], (48, 144), 144, 1),   # the far level appears: one partition in its segment
    (4, 337, 0, [4, 8, 16, 32], (48, 209), 209, 1),   # the longest filter of one segment ...
    (4, 338, 0, [4, 8, 16, 32], (48, 144), 144, 2),   # ... and two: F falls back to 144
    (4, 368, 4, [4, 8, 16, 32], (48, 240), 240, 1),   # F = 240: the T = 32 level's full 192-row tile
    (2, 17, 0, [4, 8], (16, 17), 17, 0),              # the T = 8 band of one partition (staggered at G = 2)
    (2, 25, 0, [4, 8, 16], (24, 25), 25, 0),
    (2, 41, 0, [4, 8, 16, 32], (40, 41), 41, 0),
    (2, 137, 0, [4, 8, 16, 32], (40, 136), 136, 1),
    (2, 329, 0, [4, 8, 16, 32], (40, 201), 201, 1),
    (2, 360, 4, [4, 8, 16, 32], (40, 232), 232, 1),   # the full tile at G = 2
    (8, 65, 0, [4, 8, 16, 32], (64, 65), 65, 0),
    (8, 161, 0, [4, 8, 16, 32], (64, 160), 160, 1),
    (8, 353, 0, [4, 8, 16, 32], (64, 225), 225, 1),
    (8, 384, 4, [4, 8, 16, 32], (64, 256), 256, 1)]   # the full tile at G = 8


@pytest.mark.parametrize("G,P,K,T,band,F,nseg", BAND_EDGES)
def test_staggered_band_edges(neo_gpu, oracle, G, P, K, T, band, F, nseg):
    """The edges of the staggered plan's bands: a level or the far level with one partition, the
    longest band of the T = 32 level's LDS tile, the step from one far segment to two. Each case
    first asserts the band it is named for, so a change of the plan cannot turn it into another."""
    torch = pytest.importorskip("torch")
    C, B = 3, 64
    plan = neo_gpu.convolution.stagger_plan(C, B, P, G, K)
    assert plan["T"] == T and (plan["a"][-1], plan["b"][-1]) == band and plan["staggered"][-1]
    assert (plan["far_a"], plan["nseg"]) == (F, nseg)
    assert nseg == 0 or P - F - 128 * (nseg - 1) >= 1  # partitions of the last segment
    # levels = 1: below 64 partitions a handle runs the plain step unless asked
    assert compare(neo_gpu, oracle, torch, C, B, P, {"step_group": G, "far_group": K, "levels": 1}) <= TOL


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("B", [16, 128, 512, 1024])
def test_staggered_block_sizes(neo_gpu, oracle, B, method):
    """The block kernel's staggered build is an instantiation of its own per block size and method:
    the sizes that the other cases here do not force."""
    torch = pytest.importorskip("torch")
    assert compare(neo_gpu, oracle, torch, 3, B, 170, {"step_group": 4}, method=method) <= TOL


def test_automatic_choice(neo_gpu, oracle):
    """windows = 0: staggered where the step group is automatic and the shape has 65536 16-column
    units or more, aligned below and with an explicit step group; the handle reports the plain
    step's form (1) while its levels are off. The streaming of the automatic handle at full size is
    test_upols_gpu.py's."""
    C, P = 2048, 70  # no far level, the 32-block level's band is [48, 70)
    for B, opts, want in ((256, {}, 1), (512, {}, 2), (512, {"step_group": 4}, 1), (512, {"windows": 1}, 1)):
        conv = neo_gpu.UpolsConvolver(C, B, P, options=opts)
        assert conv.step_group() == 4 and conv.windows() == want, (B, opts)
        if want == 2:
            conv.set_ahead(False)
            assert conv.windows() == 1
            conv.set_ahead(True)
            assert conv.windows() == 2
        conv.close()
    conv = neo_gpu.UpolsConvolver(2, 64, 300, options={"step_group": 4, "windows": 2, "levels": 0})
    assert conv.windows() == 1
    conv.close()


def test_staggered_refuses_latency_mode_and_bad_forms(neo_gpu):
    conv = neo_gpu.UpolsConvolver(2, 64, 300, options={"step_group": 4, "windows": 2})
    with pytest.raises(Exception, match="staggered"):
        conv.set_persistent(True)
    conv.close()
    for bad in ({"step_group": 1, "windows": 2}, {"step_group": 4, "far_level": 2, "windows": 2}):
        with pytest.raises(Exception, match="staggered"):
            neo_gpu.UpolsConvolver(2, 64, 300, options=bad)
    # explicit step groups at a small shape stay aligned; windows = 1 forces it anywhere
    conv = neo_gpu.UpolsConvolver(2, 64, 300, options={"step_group": 4})
    assert conv.windows() == 1
    conv.close()
