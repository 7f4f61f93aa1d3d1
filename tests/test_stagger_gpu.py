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
