"""Crossfaded live filter updates of the dense UPOLS / UPOLA convolvers on the GPU
(neo_hip_upols_update_filter / _update_impulse). The handle has filter A and has
processed blocks 0 .. k-1; the update brings filter B and a fade of F blocks. With y_A, y_B the
outputs of two convolvers with A and B fed the whole input: blocks before k are y_A, sample n of
blocks k .. k+F-1 is y_A + g[n] (y_B - y_A), blocks from k+F on are y_B.

Reference: the float64 mix of two oracle.dense_convolve outputs with neo.matrix_fade_gains; bar
peak_err <= 1e-5, the peak taken over the whole signal (it holds pure y_A and pure y_B stretches, so
a cancellation inside the fade cannot shrink the denominator)."""
import ctypes

import numpy as np
import pytest

from conftest import peak_err
from test_io_contract_gpu import IN_FILL, OUT_FILL, _arena, assert_same_bits, check_regions

pytestmark = pytest.mark.gpu
TOL = 1e-5
EINVAL = 1  # NEO_HIP_EINVAL

_cache = {}


def problem(oracle, C, B, P, nb, method="upols", banks=2):
    """filters [banks][C][P][B+1], the signal [C][nb B] and the oracle's outputs per filter (float64)"""
    key = (C, B, P, nb, banks)
    if key not in _cache:
        parts = []
        for k in range(banks):
            ir = np.stack([oracle.noise(9100 + 101 * k + 13 * c + B + P, B * P) for c in range(C)])
            parts.append(oracle.uniform_partition(oracle.normalize_impulse(ir), B))
        sig = np.stack([oracle.noise(9700 + 13 * c + B + P, B * nb) for c in range(C)])
        sig.setflags(write=False)
        _cache[key] = (parts, sig)
    parts, sig = _cache[key]
    m = "upola" if method == "upola" else "upols"
    if key + (m,) not in _cache:
        _cache[key + (m,)] = [oracle.dense_convolve(sig, p, method=m).astype(np.float64) for p in parts]
    return parts, sig, _cache[key + (m,)]


def mix(neo, ya, yb, B, k, F, curve):
    """blocks < k: y_A; the F blocks from k: y_A + g (y_B - y_A); then y_B"""
    ref = ya.copy()
    g = neo.matrix_fade_gains(B, F, curve).astype(np.float64)
    s = slice(k * B, (k + F) * B)
    ref[:, s] = ya[:, s] + g * (yb[:, s] - ya[:, s])
    ref[:, (k + F) * B:] = yb[:, (k + F) * B:]
    return ref


def run(neo, torch, sig, B, make, updates=(), stream=0):
    """One block per process_device call, in place; updates: {block: callable(conv)} run before that
    block. Returns the output [C][n] and the handle (open)."""
    conv = make()
    t = torch.from_numpy(np.array(sig, dtype=np.float32)).cuda()
    n = t.shape[1]
    updates = dict(updates)
    for b in range(n // B):
        if b in updates:
            updates[b](conv)
        p = t.data_ptr() + 4 * b * B
        conv.process_device(p, n, p, n, stream)
    torch.cuda.synchronize()
    return t.cpu().numpy(), conv


def maker(neo, C, B, P, parts, method, options):
    def make():
        conv = neo.UpolsConvolver(C, B, P, method=method, options=options)
        conv.filter(parts)
        return conv
    return make


# ---------------------------------------------------------------- 1. plain-step handles
PLAIN = [(1, 16, 3, 20, 7), (2, 32, 37, 100, 75), (3, 128, 9, 40, 11), (2, 512, 70, 20, 6), (2, 1024, 20, 12, 5),
         (2, 2048, 5, 10, 4), (1, 4096, 3, 8, 3)]


def check_plain(neo, oracle, torch, C, B, P, nb, k, method, options):
    parts, sig, (ya, yb) = problem(oracle, C, B, P, nb, method)
    never, ca = run(neo, torch, sig, B, maker(neo, C, B, P, parts[0], method, options))
    always, cb = run(neo, torch, sig, B, maker(neo, C, B, P, parts[1], method, options))
    ca.close()
    cb.close()
    for F in (1, 3):
        for curve in ("linear", "cosine"):
            got, conv = run(neo, torch, sig, B, maker(neo, C, B, P, parts[0], method, options),
                            {k: lambda c: c.update_filter(parts[1], fade_blocks=F, curve=curve)})
            assert conv.fade_info()["remaining_blocks"] == 0 and conv.fade_info()["bank_bytes"] > 0
            conv.close()
            err = peak_err(got, mix(neo, ya, yb, B, k, F, curve))
            print(f"C={C} B={B} P={P} {method} {options} F={F} {curve}: peak err {err:.3g}")
            assert err <= TOL, (F, curve, err)
            assert_same_bits(got[:, :k * B], never[:, :k * B], "blocks before the update")
            first = k + F + (method == "upola")  # overlap-add: block k + F takes a tail summed in the fade's order
            assert_same_bits(got[:, first * B:], always[:, first * B:], "blocks after the fade")


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("C,B,P,nb,k", PLAIN)
def test_plain_step_handles(neo_gpu, oracle, C, B, P, nb, k, fused, method):
    torch = pytest.importorskip("torch")
    check_plain(neo_gpu, oracle, torch, C, B, P, nb, k, method, {"levels": 0, "fused": fused})


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb,k,wgs", [(2, 32, 37, 100, 75, 24), (2, 512, 70, 20, 6, 128), (1, 4096, 3, 8, 3, 3)])
def test_plain_step_forced_splits(neo_gpu, oracle, C, B, P, nb, k, wgs, method):
    torch = pytest.importorskip("torch")
    opts = {"levels": 0, "fused": 0, "split_workgroups": wgs}
    conv = neo_gpu.UpolsConvolver(C, B, P, method=method, options=opts)
    assert conv.splits > 1
    conv.close()
    check_plain(neo_gpu, oracle, torch, C, B, P, nb, k, method, opts)


# ---------------------------------------------------------------- 2. streaming handles, one block per call
STREAMING = [(2, 64, 70, "upols", {}), (2, 32, 300, "upols", {"far_level": 1}),
             (3, 64, 450, "upols", {"step_group": 4, "windows": 1}),
             (2, 64, 700, "upola", {"step_group": 2, "windows": 2}),
             (2, 64, 420, "upols", {"step_group": 4, "far_level": 2})]


@pytest.mark.parametrize("C,B,P,method,options", STREAMING)
def test_streaming_handles(neo_gpu, oracle, C, B, P, method, options):
    """The update at block 301 (inside every level's window), F = 3, then two far windows more.
    After the fade the levels are primed at another phase than an always-B handle's, so the sums
    differ in order there: no bit comparison after the fade, the oracle's bar alone."""
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    k, F, nb = 301, 3, 301 + 3 + 2 * 128 + 8
    parts, sig, (ya, yb) = problem(oracle, C, B, P, nb, method)
    make = maker(neo, C, B, P, parts[0], method, options)
    never, c0 = run(neo, torch, sig[:, :k * B], B, make)
    assert c0.ahead_info()[0], "streaming levels off"
    c0.close()
    outs = []
    for _ in range(2):
        got, conv = run(neo, torch, sig, B, make, {k: lambda c: c.update_filter(parts[1], fade_blocks=F, curve="cosine")})
        assert conv.ahead_info()[0] and conv.fade_info()["remaining_blocks"] == 0
        conv.close()
        outs.append(got)
    err = peak_err(outs[0], mix(neo, ya, yb, B, k, F, "cosine"))
    print(f"C={C} B={B} P={P} {method} {options}: peak err {err:.3g}")
    assert err <= TOL, err
    assert_same_bits(outs[0][:, :k * B], never, "blocks before the update")
    assert_same_bits(outs[1], outs[0], "a second identical run")


# ---------------------------------------------------------------- 3. mixed calls
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_batched_call_spans_the_fade(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, k, F = 2, 64, 40, 100, 20, 5
    parts, sig, (ya, yb) = problem(oracle, C, B, P, nb, method)
    conv = neo.UpolsConvolver(C, B, P, method=method)
    conv.filter(parts[0])
    assert conv.batch_info()[0] > 1
    t = torch.from_numpy(np.array(sig)).cuda()
    head = t[:, :k * B].contiguous()
    conv.process_blocks(head)
    conv.update_filter(parts[1], fade_blocks=F)
    mid = t[:, k * B:(k + 64) * B].contiguous()
    conv.process_blocks(mid)  # 5 fade steps, then the call's usual passes
    assert conv.fade_info()["remaining_blocks"] == 0
    rest = t[:, (k + 64) * B:].contiguous()
    conv.process_blocks(rest)
    torch.cuda.synchronize()
    got = np.concatenate([x.cpu().numpy() for x in (head, mid, rest)], axis=1)
    conv.close()
    err = peak_err(got, mix(neo, ya, yb, B, k, F, "linear"))
    print(f"batched {method}: peak err {err:.3g}")
    assert err <= TOL, err


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_offline_windows_after_the_fade(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, k, F = 2, 32, 200, 9, 4
    nb = k + 300
    parts, sig, (ya, yb) = problem(oracle, C, B, P, nb, method)
    conv = neo.UpolsConvolver(C, B, P, method=method)
    conv.filter(parts[0])
    assert conv.offline_info()[0]
    t = torch.from_numpy(np.array(sig)).cuda()
    head = t[:, :k * B].contiguous()
    conv.process_blocks(head)
    conv.update_filter(parts[1], fade_blocks=F, curve="cosine")
    rest = t[:, k * B:].contiguous()
    conv.process_blocks(rest)  # 4 fade steps, two offline windows of 128 blocks from B's spectra, the rest
    torch.cuda.synchronize()
    got = np.concatenate([head.cpu().numpy(), rest.cpu().numpy()], axis=1)
    conv.close()
    err = peak_err(got, mix(neo, ya, yb, B, k, F, "cosine"))
    print(f"offline {method}: peak err {err:.3g}")
    assert err <= TOL, err


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_host_buffer_blocks(neo_gpu, oracle, method):
    neo = neo_gpu
    C, B, P, nb, k, F = 2, 32, 37, 100, 75, 3
    parts, sig, (ya, yb) = problem(oracle, C, B, P, nb, method)
    conv = neo.UpolsConvolver(C, B, P, method=method)
    conv.filter(parts[0])
    got = np.empty_like(sig)
    for b in range(nb):
        if b == k:
            conv.update_filter(parts[1], fade_blocks=F)
        blk = np.ascontiguousarray(sig[:, b * B:(b + 1) * B])
        conv(blk)
        got[:, b * B:(b + 1) * B] = blk
    conv.close()
    err = peak_err(got, mix(neo, ya, yb, B, k, F, "linear"))
    print(f"host blocks {method}: peak err {err:.3g}")
    assert err <= TOL, err


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_a_b_c_second_update_allocates_nothing(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb = 2, 64, 12, 60
    k1, F1, k2, F2 = 10, 3, 30, 2
    parts, sig, ys = problem(oracle, C, B, P, nb, method, banks=3)
    seen = {}

    def second(conv):
        assert conv.fade_info()["remaining_blocks"] == 0
        torch.cuda.synchronize()
        seen["bank"], seen["mem"] = conv.fade_info()["bank_bytes"], neo.memory_info()
        conv.update_filter(parts[2], fade_blocks=F2, curve="cosine")
        assert conv.fade_info()["bank_bytes"] == seen["bank"] > 0
        assert neo.memory_info() == seen["mem"], "the second update allocated"

    got, conv = run(neo, torch, sig, B, maker(neo, C, B, P, parts[0], method, {"levels": 0}),
                    {k1: lambda c: c.update_filter(parts[1], fade_blocks=F1), k2: second})
    conv.close()
    ref = mix(neo, mix(neo, ys[0], ys[1], B, k1, F1, "linear"), ys[2], B, k2, F2, "cosine")
    err = peak_err(got, ref)
    print(f"A -> B -> C {method}: peak err {err:.3g}")
    assert err <= TOL, err


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_reset_during_a_fade_leaves_b(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb = 2, 64, 12, 30
    parts, sig, _ = problem(oracle, C, B, P, nb, method)
    opts = {"levels": 0}
    fresh, cb = run(neo, torch, sig, B, maker(neo, C, B, P, parts[1], method, opts))
    cb.close()
    conv = maker(neo, C, B, P, parts[0], method, opts)()
    t = torch.from_numpy(np.array(sig)).cuda()
    conv.process_blocks(t[:, :7 * B].contiguous())
    conv.update_filter(parts[1], fade_blocks=6)
    conv.process_blocks(t[:, 7 * B:9 * B].contiguous())
    assert conv.fade_info()["remaining_blocks"] == 4
    conv.reset()
    assert conv.fade_info()["remaining_blocks"] == 0
    got, _ = run(neo, torch, sig, B, lambda: conv)
    conv.close()
    assert_same_bits(got, fresh, "after a reset during a fade")


def test_set_filter_during_a_fade_cancels_it(neo_gpu, oracle):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb = 2, 64, 12, 30
    parts, sig, _ = problem(oracle, C, B, P, nb, banks=3)
    opts = {"levels": 0}
    fresh, cc = run(neo, torch, sig, B, maker(neo, C, B, P, parts[2], "upols", opts))
    cc.close()
    conv = maker(neo, C, B, P, parts[0], "upols", opts)()
    t = torch.from_numpy(np.array(sig)).cuda()
    conv.process_blocks(t[:, :7 * B].contiguous())
    conv.update_filter(parts[1], fade_blocks=6)
    conv.process_blocks(t[:, 7 * B:9 * B].contiguous())
    conv.filter(parts[2])
    assert conv.fade_info()["remaining_blocks"] == 0 and conv.fade_info()["fade_blocks"] == 0
    got, _ = run(neo, torch, sig, B, lambda: conv)
    conv.close()
    assert_same_bits(got, fresh, "after a set_filter during a fade")


def test_update_during_a_fade_is_refused_and_changes_nothing(neo_gpu, oracle):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, k, F = 2, 64, 12, 30, 9, 5
    parts, sig, _ = problem(oracle, C, B, P, nb, banks=3)
    make = maker(neo, C, B, P, parts[0], "upols", {"levels": 0})
    want, c0 = run(neo, torch, sig, B, make, {k: lambda c: c.update_filter(parts[1], fade_blocks=F)})
    c0.close()

    def refused(conv):
        assert conv.fade_info()["remaining_blocks"] == F - 2
        with pytest.raises(neo._native.NeoHipError) as e:
            conv.update_filter(parts[2], fade_blocks=2)
        assert e.value.code == EINVAL and "fade" in str(e.value)
        assert conv.fade_info() == {"remaining_blocks": F - 2, "fade_blocks": F, "bank_bytes": conv.fade_info()["bank_bytes"]}

    got, c1 = run(neo, torch, sig, B, make, {k: lambda c: c.update_filter(parts[1], fade_blocks=F), k + 2: refused})
    c1.close()
    assert_same_bits(got, want, "a refused update changed the output")


# ---------------------------------------------------------------- 4. refusals
def test_refusals(neo_gpu, oracle):
    """Every refusal of the update calls that a caller can reach. (A group's members are handles the
    group owns: neo_hip_upols_group_* has no update call and hands out no member handle, so that
    refusal has no public path; null handles: tests/test_upols_fade.py.)"""
    neo = neo_gpu
    lib = neo._native.load()
    C, B, P = 2, 64, 70
    parts, _, _ = problem(oracle, C, B, P, 8)
    ir = np.stack([oracle.noise(77 + c, B * P) for c in range(C)])
    H = np.ascontiguousarray(parts[1])
    hp = H.ctypes.data_as(ctypes.c_void_p)

    def einval(conv, fn, word=None):
        before = conv.fade_info()
        with pytest.raises(neo._native.NeoHipError) as e:
            fn()
        assert e.value.code == EINVAL, e.value
        assert word is None or word in str(e.value), e.value
        assert conv.fade_info() == before

    conv = neo.UpolsConvolver(C, B, P)
    einval(conv, lambda: conv.update_filter(parts[1]), "no filter")  # no filter set yet
    einval(conv, lambda: conv.update_impulse(ir), "no filter")
    conv.filter(parts[0])
    assert lib.neo_hip_upols_update_filter(conv._h, None, 0, 1, 0, None) == EINVAL  # a null argument
    assert lib.neo_hip_upols_update_impulse(conv._h, None, B * P, 1, 0, 1, 0, None) == EINVAL
    for F in (0, -3, (1 << 20) + 1):
        einval(conv, lambda: conv.update_filter(parts[1], fade_blocks=F), "fade_blocks")
    for curve in (2, -1):
        einval(conv, lambda: conv.update_filter(parts[1], curve=curve), "curve")
    with pytest.raises(ValueError):
        conv.update_filter(parts[1], curve="cubic")
    einval(conv, lambda: conv.update_impulse(ir[:, :B * (P - 1)]), "partitions")  # another P
    assert lib.neo_hip_upols_update_impulse(conv._h, ir.ctypes.data_as(ctypes.c_void_p), 0, 1, 0, 1, 0, None) == EINVAL
    assert conv.fade_info() == {"remaining_blocks": 0, "fade_blocks": 0, "bank_bytes": 0}  # nothing was allocated
    conv.set_persistent(True)  # latency mode on
    einval(conv, lambda: conv.update_filter(parts[1]), "latency")
    conv.set_persistent(False)
    conv.update_filter(parts[1], fade_blocks=4)
    einval(conv, lambda: conv.update_filter(parts[0]), "fade")  # a fade has blocks left
    einval(conv, lambda: conv.update_impulse(ir), "fade")
    with pytest.raises(neo._native.NeoHipError) as e:  # and the latency mode stays off meanwhile
        conv.set_persistent(True)
    assert e.value.code == EINVAL and "fade" in str(e.value)
    assert not conv.persistent_info()["enabled"]
    for call in (lambda: conv.set_batch(False), lambda: conv.set_offline(False), lambda: conv.set_ahead(False),
                 lambda: conv.set_paced(0)):
        call()
        assert conv.fade_info()["remaining_blocks"] == 4  # the mode switches keep the fade
    conv.close()

    v2 = neo.UpolsConvolver(C, B, P, method="upola_v2")
    v2.filter(parts[0])
    einval(v2, lambda: v2.update_filter(parts[1]), "v2")
    v2.close()

    sp = neo.SparseUpolsConvolver(C, B, P)
    sp.filter(parts[0], np.ones(parts[0].shape, np.uint8))
    with pytest.raises(neo._native.NeoHipError) as e:
        sp.update_filter(parts[1])
    assert e.value.code == EINVAL and "sparse" in str(e.value)
    with pytest.raises(neo._native.NeoHipError):
        sp.update_impulse(ir)
    sp.close()


# ---------------------------------------------------------------- 5. I/O contract
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_io_contract_through_a_fade(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, k, F = 2, 64, 12, 24, 7, 3
    parts, sig, (ya, yb) = problem(oracle, C, B, P, nb, method)
    n = nb * B
    make = maker(neo, C, B, P, parts[0], method, {"levels": 0})

    def drive(ip, li, op, lo):
        conv = make()
        for b in range(nb):
            if b == k:
                conv.update_filter(parts[1], fade_blocks=F, curve="cosine")
            conv.process_device(ip + 4 * b * B, li, op + 4 * b * B, lo, 0)
        torch.cuda.synchronize()
        conv.close()

    t = torch.from_numpy(np.array(sig)).cuda()
    drive(t.data_ptr(), n, t.data_ptr(), n)
    A = t.cpu().numpy()
    err = peak_err(A, mix(neo, ya, yb, B, k, F, "cosine"))
    assert err <= TOL, err
    ld_in, ld_out = n + 36, n + 4
    ia = _arena(torch, C, ld_in, IN_FILL)
    ia.view(torch.float32)[1:C + 1, :n] = torch.from_numpy(np.array(sig)).cuda()
    oa = _arena(torch, C, ld_out, OUT_FILL)
    before = ia.cpu().numpy()
    drive(ia.data_ptr() + 4 * ld_in, ld_in, oa.data_ptr() + 4 * ld_out, ld_out)
    payload = check_regions(oa.cpu().numpy(), C, n, OUT_FILL, before, ia.cpu().numpy())
    assert_same_bits(payload, A, "separate padded buffers")
    pa = _arena(torch, C, ld_out, IN_FILL)
    pa.view(torch.float32)[1:C + 1, :n] = torch.from_numpy(np.array(sig)).cuda()
    drive(pa.data_ptr() + 4 * ld_out, ld_out, pa.data_ptr() + 4 * ld_out, ld_out)
    assert_same_bits(check_regions(pa.cpu().numpy(), C, n, IN_FILL), A, "in place, padded")


# ---------------------------------------------------------------- 6. CUDA tensors on a non-default stream
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_cuda_tensors_on_a_side_stream(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, k, F = 2, 64, 12, 24, 7, 3
    parts, sig, (ya, yb) = problem(oracle, C, B, P, nb, method)
    irb = np.stack([oracle.noise(9100 + 101 + 13 * c + B + P, B * P) for c in range(C)])  # filter B's impulse
    side = torch.cuda.Stream()
    outs = []
    for form in ("filter", "impulse"):
        conv = neo.UpolsConvolver(C, B, P, method=method, options={"levels": 0})
        conv.filter(parts[0])
        with torch.cuda.stream(side):
            t = torch.from_numpy(np.array(sig)).cuda()
            n = t.shape[1]
            for b in range(nb):
                if b == k and form == "filter":
                    conv.update_filter(torch.from_numpy(parts[1]).cuda(), fade_blocks=F)
                elif b == k:
                    conv.update_impulse(torch.from_numpy(irb).cuda(), fade_blocks=F)
                p = t.data_ptr() + 4 * b * B
                conv.process_device(p, n, p, n, side.cuda_stream)
            side.synchronize()
        outs.append(t.cpu().numpy())
        conv.close()
        err = peak_err(outs[-1], mix(neo, ya, yb, B, k, F, "linear"))
        print(f"side stream, {form}, {method}: peak err {err:.3g}")
        assert err <= TOL, (form, err)


# ---------------------------------------------------------------- 7. multi-device
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_multi_device_equals_unsharded(neo_gpu, oracle, method):
    neo = neo_gpu
    C, B, P, nb, k, F = 3, 64, 12, 24, 7, 3
    parts, sig, (ya, yb) = problem(oracle, C, B, P, nb, method)
    ir = np.stack([oracle.noise(31 + c, B * P) * (c + 1) for c in range(C)])
    outs = []
    for multi in (False, True):
        conv = (neo.UpolsMultiConvolver(C, B, P, [0, 0], method=method, options={"levels": 0}) if multi
                else neo.UpolsConvolver(C, B, P, method=method, options={"levels": 0}))
        conv.filter(parts[0])
        y = [conv.process(np.ascontiguousarray(sig[:, :k * B]).copy())]
        conv.update_filter(parts[1], fade_blocks=F, curve="cosine")
        assert conv.fade_info()["remaining_blocks"] == F
        y.append(conv.process(np.ascontiguousarray(sig[:, k * B:(k + 9) * B]).copy()))
        conv.update_impulse(ir, fade_blocks=2)  # one normalisation factor over all channels
        y.append(conv.process(np.ascontiguousarray(sig[:, (k + 9) * B:]).copy()))
        assert conv.fade_info()["remaining_blocks"] == 0
        outs.append(np.concatenate(y, axis=1))
        conv.close()
    err = peak_err(outs[0][:, :(k + 9) * B], mix(neo, ya, yb, B, k, F, "cosine")[:, :(k + 9) * B])
    assert err <= TOL, err
    assert_same_bits(outs[1], outs[0], "sharded and unsharded")
