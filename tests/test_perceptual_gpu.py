"""The perceptual sparsity predicate on the device (csrc/perceptual.hip: k_perc_max, k_perc_mask,
k_perc_hist) and the sparse handles' perceptual setup calls.

Every value test runs on the DEVICE'S OWN partitions, neo.uniform_partition(neo.normalize_impulse(ir))
downloaded: the definition is applied to those spectra, by the host definition
(neo.perceptual_mask_host, csrc/perceptual_plan.hpp) and by the float64 numpy restatement of
tests/perceptual_common.py, not to a separately computed FFT (weak bins of a GPU and a CPU
transform differ by far more than the band). A device result may differ from the float64
restatement only inside the band (perceptual_common: DELTA, DELTA_HIST), which holds at most 0.1 %
of a case's bins. Convolver outputs are compared bit for bit where the same kernels run on the same
tiles, and against oracle.dense_convolve on the masked filter at the project's 1e-5 bar."""
import ctypes

import numpy as np
import pytest

import perceptual_common as pc
from conftest import peak_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
_cache = {}


def problem(neo, C, B, P):
    """ir [C][B P], the device's partitions of the normalized ir [C][P][B+1] and a signal, made once."""
    key = ("problem", C, B, P)
    if key not in _cache:
        ir = pc.impulse(C, B, P)
        parts = neo.uniform_partition(neo.normalize_impulse(ir.copy()), B)
        rng = np.random.default_rng(8000 + B + P)
        sig = rng.standard_normal((C, B * pc.BLOCKS[(C, B, P)])).astype(np.float32)
        for a in (ir, parts, sig):
            a.setflags(write=False)
        _cache[key] = (ir, parts, sig)
    return _cache[key]


def sparsity_of(neo, B):
    """the rule the convolver tests run with: A-weighting at a 40 dB dynamic range; the first two
    columns always kept where a row has more than two tiles (they would keep tile 0 of every row)"""
    return neo.PerceptualSparsity(pc.SAMPLE_RATE, -40.0, 2 if B > 32 else 0, "a")


def run(conv, sig):
    out = sig.copy()
    conv.process(out)
    return out


def mask_route(neo, C, B, P, method, fused):
    """filter(parts, perceptual_mask(parts, ...)): outputs and sparse_info, made once per case"""
    key = ("mask-route", C, B, P, method, fused)
    if key not in _cache:
        _, parts, sig = problem(neo, C, B, P)
        sp = sparsity_of(neo, B)
        conv = neo.SparseUpolsConvolver(C, B, P, method=method, options={"fused": fused})
        conv.filter(parts, neo.perceptual_mask(parts, sp))
        _cache[key] = (run(conv, sig), conv.sparse_info())
        conv.close()
    return _cache[key]


@pytest.mark.parametrize("C,B,P", pc.SHAPES)
def test_device_mask(neo_gpu, C, B, P):
    import torch

    neo = neo_gpu
    _, parts, _ = problem(neo, C, B, P)
    dparts = torch.from_numpy(parts.copy()).cuda()
    for weighting in pc.WEIGHTINGS:
        for low in pc.low_bins(B):
            lv, exact = pc.levels64(parts, pc.weights64(B, pc.SAMPLE_RATE, low, weighting))
            for theta in pc.THRESHOLDS:
                sp = neo.PerceptualSparsity(pc.SAMPLE_RATE, theta, low, weighting)
                what = f"{(C, B, P)} {weighting} low={low} theta={theta}"
                got = neo.perceptual_mask(parts, sp)
                assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and got.shape == parts.shape
                assert set(np.unique(got.view(np.uint8))) <= {0, 1}
                nband = pc.check_mask(got, lv, exact, theta, what + " device")
                host = neo.perceptual_mask_host(parts, sp)
                pc.check_mask(host, lv, exact, theta, what + " host")
                assert int((got != host).sum()) <= nband, what
                tgot = neo.perceptual_mask(dparts, sp)
                assert tgot.is_cuda and tgot.dtype == torch.bool and tuple(tgot.shape) == parts.shape
                assert np.array_equal(tgot.cpu().numpy().view(np.uint8), got.view(np.uint8)), what
                if theta == -80.0 and weighting == "none":
                    assert got.all()
    # a row that starts on every byte offset of a 32-bit word was covered: rows are B + 1 bytes


@pytest.mark.parametrize("C,B,P", pc.SHAPES)
def test_device_histogram(neo_gpu, C, B, P):
    import torch

    neo = neo_gpu
    _, parts, _ = problem(neo, C, B, P)
    dparts = torch.from_numpy(parts.copy()).cuda()
    for weighting in pc.WEIGHTINGS:
        for low in pc.low_bins(B):
            what = f"{(C, B, P)} {weighting} low={low}"
            sp = neo.PerceptualSparsity(pc.SAMPLE_RATE, -40.0, low, weighting)
            lv, exact = pc.levels64(parts, pc.weights64(B, pc.SAMPLE_RATE, low, weighting))
            tl, texact = pc.tile_levels64(lv, exact)
            h = neo.perceptual_histogram(parts, sp)
            assert h["bins"].shape == h["tiles"].shape == (C, 144)
            pc.check_hist(h["bins"], lv, exact, P * (B + 1), lv.size, what + " bins")
            pc.check_hist(h["tiles"], tl, texact, P * (B // 16), lv.size, what + " tiles")
            # against the host definition: the two may differ by band members only
            hh = neo.perceptual_histogram_host(parts, sp)
            for name, levels, ex in (("bins", lv, exact), ("tiles", tl, texact)):
                lower, upper, _ = pc.hist_bounds(levels, ex)
                assert np.all(np.abs(h[name] - hh[name]) <= upper - lower), (what, name)
            ht = neo.perceptual_histogram(dparts, sp)
            assert np.array_equal(ht["bins"], h["bins"]) and np.array_equal(ht["tiles"], h["tiles"]), what
    # the cumulative counts are the tiles a handle keeps at an integer threshold
    sp = sparsity_of(neo, B)
    lv, exact = pc.levels64(parts, pc.weights64(B, sp.sample_rate, sp.low_bins_to_keep, sp.weighting))
    tl, texact = pc.tile_levels64(lv, exact)
    tiles = neo.perceptual_histogram(parts, sp)["tiles"]
    conv = neo.SparseUpolsConvolver(C, B, P)
    for theta in (-20.0, -40.0, -60.0):
        conv.filter(parts, neo.PerceptualSparsity(sp.sample_rate, theta, sp.low_bins_to_keep, sp.weighting))
        kept = conv.sparse_info()["kept_tiles"]
        near = int(((np.abs(tl - theta) <= pc.DELTA) & ~texact).sum())
        print(f"{(C, B, P)} theta={theta}: kept tiles {kept}, histogram {int(tiles[:, :int(-theta)].sum())}, near {near}")
        assert abs(int(tiles[:, :int(-theta)].sum()) - kept) <= near
        assert abs(kept - int((tl > theta).sum())) <= near
    conv.close()


@pytest.mark.parametrize("C,B,P", pc.SHAPES)
def test_filter_with_sparsity_equals_filter_with_its_mask(neo_gpu, C, B, P):
    import torch

    neo = neo_gpu
    _, parts, sig = problem(neo, C, B, P)
    sp = sparsity_of(neo, B)
    for method in ("upols", "upola"):
        for fused in (0, 1):
            want, info = mask_route(neo, C, B, P, method, fused)
            conv = neo.SparseUpolsConvolver(C, B, P, method=method, options={"fused": fused})
            conv.filter(parts, sp)
            assert conv.sparse_info() == info, (method, fused)
            got = run(conv, sig)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (method, fused)
            assert 0 < info["kept_tiles"] < C * P * (B // 16) and np.abs(got).max() > 0
            if fused == 0:  # a device filter takes the same route with nothing copied in
                conv.filter(torch.from_numpy(parts.copy()).cuda(), sp)
                assert conv.sparse_info() == info
                assert np.array_equal(run(conv, sig).view(np.uint32), want.view(np.uint32)), (method, "device filter")
            conv.close()


@pytest.mark.parametrize("C,B,P", pc.SHAPES)
def test_set_impulse_with_sparsity(neo_gpu, oracle, C, B, P):
    import torch

    neo = neo_gpu
    ir, parts, sig = problem(neo, C, B, P)
    sp = sparsity_of(neo, B)
    mask = neo.perceptual_mask(parts, sp)
    for method in ("upols", "upola"):
        ref = oracle.dense_convolve(sig, (parts * mask).astype(np.complex64), method=method)
        for fused in (0, 1):
            want, info = mask_route(neo, C, B, P, method, fused)
            conv = neo.SparseUpolsConvolver(C, B, P, method=method, options={"fused": fused})
            conv.set_impulse(ir, sp)
            assert conv.sparse_info() == info, (method, fused)
            got = run(conv, sig)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (method, fused)
            err = peak_err(got, ref)
            print(f"{(C, B, P)} {method} fused={fused}: peak err {err:.3g}, tiles {info['kept_tiles']}")
            assert err <= TOL, (method, fused, err)
            if fused == 1:  # a device impulse response
                conv.set_impulse(torch.from_numpy(ir.copy()).cuda(), sp)
                assert conv.sparse_info() == info
                assert np.array_equal(run(conv, sig).view(np.uint32), want.view(np.uint32)), (method, "device ir")
            conv.close()
        a = neo.sparse_convolve(sig, ir, B, sp, method=method)
        b = neo.sparse_convolve(sig, ir, B, mask, method=method)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), method
    # normalize=False partitions the impulse response as it is
    conv = neo.SparseUpolsConvolver(C, B, P)
    conv.set_impulse(ir, sp, normalize=False)
    raw = neo.uniform_partition(ir, B)
    other = neo.SparseUpolsConvolver(C, B, P)
    other.filter(raw, neo.perceptual_mask(raw, sp))
    assert conv.sparse_info() == other.sparse_info()
    assert np.array_equal(run(conv, sig).view(np.uint32), run(other, sig).view(np.uint32))
    conv.close()
    other.close()


def test_dense_handle_and_refused_calls(neo_gpu):
    neo = neo_gpu
    C, B, P = 3, 128, 9
    ir, parts, sig = problem(neo, C, B, P)
    lib = neo._native.load()
    E = neo._native.NEO_HIP_EINVAL
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = sparsity_of(neo, B)._c()
    dense = neo.UpolsConvolver(C, B, P)
    assert lib.neo_hip_upols_set_filter_perceptual(dense._h, vp(parts), ctypes.byref(good), 0) == E
    assert b"not a sparse handle" in lib.neo_hip_last_error()
    assert lib.neo_hip_upols_set_impulse_perceptual(dense._h, vp(ir), ir.shape[1], 1, ctypes.byref(good), 0) == E
    assert b"not a sparse handle" in lib.neo_hip_last_error()
    dense.close()
    # a refused call in the middle of a stream of blocks changes nothing
    sp = sparsity_of(neo, B)
    conv = neo.SparseUpolsConvolver(C, B, P)
    conv.set_impulse(ir, sp)
    want = run(conv, sig)
    conv.set_impulse(ir, sp)
    info = conv.sparse_info()
    half = (sig.shape[1] // B // 2) * B
    first = np.ascontiguousarray(sig[:, :half])
    conv.process(first)
    bad_low = neo.PerceptualSparsity(pc.SAMPLE_RATE, -40.0, B + 1, "a")
    with pytest.raises(neo._native.NeoHipError, match="low_bins_to_keep"):
        conv.set_impulse(ir, bad_low)
    with pytest.raises(neo._native.NeoHipError, match="low_bins_to_keep"):
        conv.filter(parts, bad_low)
    with pytest.raises(neo._native.NeoHipError, match="partitions"):
        conv.set_impulse(ir[:, : B * (P - 1)], sp)
    with pytest.raises(neo._native.NeoHipError, match="sparse"):
        conv.set_impulse(ir)  # the base-class form stays refused
    with pytest.raises(neo._native.NeoHipError, match="threshold_db"):
        conv.filter(parts, neo.PerceptualSparsity(pc.SAMPLE_RATE, float("nan"), 0, "a"))
    assert conv.sparse_info() == info
    second = np.ascontiguousarray(sig[:, half:])
    conv.process(second)
    conv.close()
    assert np.array_equal(np.concatenate([first, second], axis=1).view(np.uint32), want.view(np.uint32))


def test_setup_beside_running_work(neo_gpu):
    """A handle stepping on a stream of its own while a second sparse handle is set up from an
    impulse response (on that handle's stream): both give what they give alone."""
    import torch

    neo = neo_gpu
    C, B, P = 2, 512, 70
    ir, parts, sig = problem(neo, C, B, P)
    sp = sparsity_of(neo, B)
    want_b, info = mask_route(neo, C, B, P, "upols", 1)
    solo = neo.SparseUpolsConvolver(C, B, P, options={"fused": 0})
    solo.filter(parts, neo.PerceptualSparsity(pc.SAMPLE_RATE, -60.0, 0, "none"))
    want_a = run(solo, sig)
    solo.close()
    a = neo.SparseUpolsConvolver(C, B, P, options={"fused": 0})
    a.filter(parts, neo.PerceptualSparsity(pc.SAMPLE_RATE, -60.0, 0, "none"))
    b = neo.SparseUpolsConvolver(C, B, P, options={"fused": 1})
    stream = torch.cuda.Stream()
    x = torch.from_numpy(sig.copy()).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        a.process_blocks(x, stream=stream.cuda_stream)  # queued: 120 single-block steps
    b.set_impulse(ir, sp)  # beside them
    got_b = run(b, sig)
    stream.synchronize()
    got_a = x.cpu().numpy()
    assert b.sparse_info() == info
    a.close()
    b.close()
    assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32))
    assert np.array_equal(got_b.view(np.uint32), want_b.view(np.uint32))


def test_cpp_perceptual_on_gpu():
    """tests/cpp/test_perceptual.cpp on the device: sparse_upola_convolver::filter(matrix,
    perceptual_sparsity) against the callable form on the host definition, B = 128 and 1024."""
    import subprocess

    from test_perceptual import build_cpp_test

    r = subprocess.run([build_cpp_test()], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "perceptual C++ tests passed" in r.stdout
