"""Crossfaded live filter updates of the sparse UPOLS / UPOLA convolvers on the GPU
(neo_hip_upols_update_filter_sparse / _perceptual / _update_impulse_perceptual; DESIGN 5.7, "Live
filter updates"). The handle has sparse filter A (partitions under a mask) and has processed blocks
0 .. k-1; the update brings filter B (partitions under another mask) and a fade of F blocks. With
y_A, y_B the outputs of two sparse convolvers that had A and B from block 0: blocks before k are y_A,
sample n of blocks k .. k+F-1 is y_A + g[n] (y_B - y_A), blocks from k+F on are y_B.

Reference: the float64 mix (neo.fade_gains) of oracle.dense_convolve(sig, parts_a * mask_a) and
oracle.dense_convolve(sig, parts_b * mask_b); bar peak_err <= 1e-5, the peak over the whole signal."""
import ctypes

import numpy as np
import pytest

from conftest import peak_err
from test_io_contract_gpu import IN_FILL, OUT_FILL, _arena, _host_arena, assert_same_bits, check_regions
from test_upols_fade_gpu import mix, run

pytestmark = pytest.mark.gpu
TOL = 1e-5
EINVAL = 1  # NEO_HIP_EINVAL

#         C  B     P   blocks k     the smallest shape at which ...
SHAPES = [(2, 16, 7, 60, 41),     # one tile per row; the ring of P + 31 = 38 rows has wrapped before the update
          (1, 32, 37, 100, 75),   # two tiles, per-lane bitmap loads, wrap
          (3, 128, 9, 40, 11),    # first wave-uniform rows
          (2, 512, 70, 24, 6),    # exactly one bitmap word, P >= 64
          (1, 1024, 20, 12, 5),   # two words, two float4 per lane
          (2, 2048, 5, 10, 4),    # chunked rows
          (1, 4096, 3, 8, 3)]     # chunked rows
PAIRS = ["nested-up", "nested-down", "disjoint", "decaying-to-bernoulli", "full-to-empty", "empty-to-full", "same-mask"]
_cache = {}


def filters(oracle, C, B, P, banks=2):
    """independent filters [banks][C][P][B+1]"""
    key = ("filters", C, B, P, banks)
    if key not in _cache:
        out = []
        for j in range(banks):
            ir = np.stack([oracle.noise(7100 + 101 * j + 13 * c + B + P, B * P) for c in range(C)])
            p = oracle.uniform_partition(oracle.normalize_impulse(ir), B)
            p.setflags(write=False)
            out.append(p)
        _cache[key] = out
    return _cache[key]


def signal(oracle, C, B, P, nb):
    key = ("signal", C, B, P, nb)
    if key not in _cache:
        sig = np.stack([oracle.noise(7700 + 13 * c + B + P, B * nb) for c in range(C)])
        sig.setflags(write=False)
        _cache[key] = sig
    return _cache[key]


def mask_pair(name, C, B, P):
    """(mask A, mask B) [C][P][B+1] bool"""
    rng = np.random.default_rng(5000 + B + P)
    shape = (C, P, B + 1)
    u = rng.random(shape)
    if name == "nested-up":  # the threshold knob, opening: 0.1 within 0.5
        return u < 0.1, u < 0.5
    if name == "nested-down":
        return u < 0.5, u < 0.1
    if name == "disjoint":
        return u < 0.3, u >= 0.7
    if name == "decaying-to-bernoulli":  # the decaying mask of tests/test_sparse_gpu.py
        lim = np.floor(B * 0.5 ** (np.arange(P) / 8.0)).astype(int)
        return np.broadcast_to(np.arange(B + 1)[None, :] <= lim[:, None], shape).copy(), u < 0.3
    if name == "full-to-empty":  # the empty bank has no tile and no allocation
        return np.ones(shape, bool), np.zeros(shape, bool)
    if name == "empty-to-full":
        return np.zeros(shape, bool), np.ones(shape, bool)
    if name == "same-mask":  # other values under the same mask
        return u < 0.3, u < 0.3
    raise KeyError(name)


def masked(parts, mask):
    return (parts * mask).astype(np.complex64)


def reference(oracle, sig, parts, mask, method, key):
    key = ("ref", method) + key
    if key not in _cache:
        y = oracle.dense_convolve(sig, masked(parts, mask), method=method).astype(np.float64)
        y.setflags(write=False)
        _cache[key] = y
    return _cache[key]


def sparse_maker(neo, C, B, P, parts, mask, method, options=None, batch=False):
    def make():
        conv = neo.SparseUpolsConvolver(C, B, P, method=method, options=options)
        conv.filter(parts, mask)
        if batch:
            conv.set_batch(True)
        return conv
    return make


def canon(x):
    return x + np.float32(0.0)  # -0 -> +0


# ---------------------------------------------------------------- 1, 2. every shape, pair, method
def check_pair(neo, oracle, torch, C, B, P, nb, k, method, pair, options, dense_options=None):
    pa, pb = filters(oracle, C, B, P)
    ma, mb = mask_pair(pair, C, B, P)
    sig = signal(oracle, C, B, P, nb)
    ya = reference(oracle, sig, pa, ma, method, (C, B, P, nb, pair, "a"))
    yb = reference(oracle, sig, pb, mb, method, (C, B, P, nb, pair, "b"))
    never, ca = run(neo, torch, sig, B, sparse_maker(neo, C, B, P, pa, ma, method, options))
    always, cb = run(neo, torch, sig, B, sparse_maker(neo, C, B, P, pb, mb, method, options))
    info_b = cb.sparse_info()
    ca.close()
    cb.close()
    for F in (1, 3):
        for curve in ("linear", "cosine"):
            upd = {k: lambda c: c.update_filter(pb, mb, fade_blocks=F, curve=curve)}
            got, conv = run(neo, torch, sig, B, sparse_maker(neo, C, B, P, pa, ma, method, options), upd)
            assert conv.fade_info()["remaining_blocks"] == 0 and conv.fade_info()["bank_bytes"] > 0
            assert conv.sparse_info() == info_b
            conv.close()
            err = peak_err(got, mix(neo, ya, yb, B, k, F, curve))
            print(f"C={C} B={B} P={P} {method} {pair} {options} F={F} {curve}: peak err {err:.3g}")
            assert err <= TOL, (F, curve, err)
            assert_same_bits(got[:, :k * B], never[:, :k * B], "blocks before the update")
            first = k + F + (method == "upola")  # overlap-add: block k + F takes a tail summed in the fade's order
            assert_same_bits(got[:, first * B:], always[:, first * B:], "blocks after the fade")
            if dense_options is not None:  # the dense handle's fade on the zeroed filters: the same order of sums
                def dense():
                    d = neo.UpolsConvolver(C, B, P, method=method, options=dense_options)
                    d.filter(masked(pa, ma))
                    return d
                want, dc = run(neo, torch, sig, B, dense, {k: lambda c: c.update_filter(masked(pb, mb), fade_blocks=F, curve=curve)})
                sp = neo.SparseUpolsConvolver(C, B, P, method=method, options=options)
                assert sp.splits == dc.splits, (sp.splits, dc.splits)
                sp.close()
                dc.close()
                s = slice(k * B, (k + F) * B)
                assert_same_bits(canon(got[:, s]), canon(want[:, s]), "fade blocks against the dense fade on the zeroed filters")


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb,k", SHAPES)
def test_every_shape_and_mask_pair(neo_gpu, oracle, C, B, P, nb, k, method, pair):
    torch = pytest.importorskip("torch")
    for fused in (0, 1):
        check_pair(neo_gpu, oracle, torch, C, B, P, nb, k, method, pair, {"fused": fused})


@pytest.mark.parametrize("pair", ["nested-up", "full-to-empty"])
@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb,k,wgs", [(2, 16, 7, 60, 41, 1), (1, 32, 37, 100, 75, 1), (3, 128, 9, 40, 11, 1),
                                            (2, 512, 70, 24, 6, 1), (1, 1024, 20, 12, 5, 1), (2, 2048, 5, 10, 4, 1),
                                            (1, 4096, 3, 8, 3, 1),
                                            (1, 32, 37, 100, 75, 12), (2, 512, 70, 24, 6, 128), (1, 1024, 20, 12, 5, 4),
                                            (1, 4096, 3, 8, 3, 3)])
def test_fade_blocks_equal_the_dense_fade_on_zeroed_filters(neo_gpu, oracle, C, B, P, nb, k, wgs, method, pair):
    """split_workgroups = 1: one split; a forced value: more than one, the same in both handles"""
    torch = pytest.importorskip("torch")
    opts = {"fused": 0, "split_workgroups": wgs}
    sp = neo_gpu.SparseUpolsConvolver(C, B, P, method=method, options=opts)
    assert (sp.splits > 1) == (wgs > 1), sp.splits
    sp.close()
    check_pair(neo_gpu, oracle, torch, C, B, P, nb, k, method, pair, opts, dict(opts, levels=0))


# ---------------------------------------------------------------- 3. impulse responses and the threshold knob
def _impulses(oracle, C, B, P):
    """decaying noise: its partitions fall through the thresholds one after the other"""
    n = B * P
    env = np.exp(-6.0 * np.arange(n) / n).astype(np.float32)
    return [np.stack([oracle.noise(8100 + 17 * j + c + B, n) * env for c in range(C)]) for j in range(2)]


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb,k", [(2, 64, 12, 30, 9), (1, 1024, 6, 14, 5)])
def test_update_impulse_equals_update_filter_with_the_perceptual_mask(neo_gpu, oracle, C, B, P, nb, k, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    ir_a, ir_b = _impulses(oracle, C, B, P)
    sa, sb = neo.PerceptualSparsity(48000.0, -30.0, 1), neo.PerceptualSparsity(48000.0, -45.0, 2)
    sig = signal(oracle, C, B, P, nb)
    Pb = neo.uniform_partition(neo.normalize_impulse(ir_b.copy()), B)
    mb = neo.perceptual_mask(Pb, sb)
    assert 0 < int(mb.sum()) < mb.size

    def make():
        conv = neo.SparseUpolsConvolver(C, B, P, method=method)
        conv.set_impulse(ir_a.copy(), sa)
        return conv

    outs, infos = [], []
    for upd in (lambda c: c.update_impulse(ir_b.copy(), sb, fade_blocks=3, curve="cosine"),
                lambda c: c.update_filter(Pb, mb, fade_blocks=3, curve="cosine"),
                lambda c: c.update_filter(Pb, sb, fade_blocks=3, curve="cosine"),
                lambda c: c.update_impulse(torch.from_numpy(ir_b.copy()).cuda(), sb, fade_blocks=3, curve="cosine")):
        got, conv = run(neo, torch, sig, B, make, {k: upd})
        outs.append(got)
        infos.append(conv.sparse_info())
        conv.close()
    for got, info in zip(outs[1:], infos[1:]):
        assert info == infos[0]
        assert_same_bits(got, outs[0], "update_impulse against update_filter with the perceptual mask")


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_threshold_change_on_the_same_impulse(neo_gpu, oracle, method):
    """the threshold knob: the same impulse response under two threshold_db values, F = 3"""
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, k, F = 2, 128, 10, 30, 12, 3
    ir = _impulses(oracle, C, B, P)[0]
    # the device's own partitions and masks: a bin within rounding of a threshold may fall on either side
    # of it in another transform's spectra, and the reference must thin what the handle thins
    parts = neo.uniform_partition(neo.normalize_impulse(ir.copy()), B)
    sa, sb = neo.PerceptualSparsity(48000.0, -25.0), neo.PerceptualSparsity(48000.0, -50.0)
    ma, mb = neo.perceptual_mask(parts, sa), neo.perceptual_mask(parts, sb)
    assert 0 < int(ma.sum()) < int(mb.sum()) < mb.size, (int(ma.sum()), int(mb.sum()), mb.size)
    sig = signal(oracle, C, B, P, nb)
    ya = oracle.dense_convolve(sig, masked(parts, ma), method=method).astype(np.float64)
    yb = oracle.dense_convolve(sig, masked(parts, mb), method=method).astype(np.float64)

    def make():
        conv = neo.SparseUpolsConvolver(C, B, P, method=method)
        conv.set_impulse(ir.copy(), sa)
        return conv

    got, conv = run(neo, torch, sig, B, make, {k: lambda c: c.update_impulse(ir.copy(), sb, fade_blocks=F)})
    kept = conv.sparse_info()["kept_bins"]
    conv.close()
    err = peak_err(got, mix(neo, ya, yb, B, k, F, "linear"))
    print(f"threshold knob {method}: kept {int(ma.sum())} -> {kept}, peak err {err:.3g}")
    assert err <= TOL, err


# ---------------------------------------------------------------- 4. batched passes
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_batched_call_spans_the_fade(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, k, F = 2, 64, 70, 140, 20, 5
    pa, pb = filters(oracle, C, B, P)
    ma, mb = mask_pair("nested-down", C, B, P)
    sig = signal(oracle, C, B, P, nb)
    ya = reference(oracle, sig, pa, ma, method, (C, B, P, nb, "batched", "a"))
    yb = reference(oracle, sig, pb, mb, method, (C, B, P, nb, "batched", "b"))
    def drive(conv, update):
        """head [0, k) | (the update) | mid [k, k + 64): F fade steps, then the call's batched passes | rest.
        The always-B handle takes mid as two calls cut at the fade's end, so both run the same passes after it."""
        t = torch.from_numpy(np.array(sig)).cuda()
        cuts = [0, k, k + 64, nb] if update else [0, k, k + F, k + 64, nb]
        pieces = [t[:, a * B:b * B].contiguous() for a, b in zip(cuts[:-1], cuts[1:])]
        for i, x in enumerate(pieces):
            if update and i == 1:
                conv.update_filter(pb, mb, fade_blocks=F)
                assert conv.fade_info()["remaining_blocks"] == F
            conv.process_blocks(x)
            if update and i == 1:
                assert conv.fade_info()["remaining_blocks"] == 0
        torch.cuda.synchronize()
        return np.concatenate([x.cpu().numpy() for x in pieces], axis=1)

    conv = sparse_maker(neo, C, B, P, pa, ma, method, batch=True)()
    T = conv.sparse_batch_info()["blocks_per_pass"]
    assert T > 1
    got = drive(conv, True)
    wt = conv.sparse_batch_info()["window_tiles"]
    conv.close()
    cb = sparse_maker(neo, C, B, P, pb, mb, method, batch=True)()
    always = drive(cb, False)
    assert wt == cb.sparse_batch_info()["window_tiles"]
    assert wt == neo.sparse_window_plan(neo.sparse_plan(mb, B)["tile_mask"], B, T)["window_tiles"]  # B's
    cb.close()
    err = peak_err(got, mix(neo, ya, yb, B, k, F, "linear"))
    print(f"batched {method}: T = {T}, peak err {err:.3g}")
    assert err <= TOL, err
    first = k + F + (method == "upola")
    assert_same_bits(got[:, first * B:], always[:, first * B:], "batched passes after the fade")


# ---------------------------------------------------------------- 5. A -> B -> C
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_a_b_c_keeps_the_fixed_size_buffers(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb = 2, 64, 12, 60
    k1, F1, k2, F2 = 10, 3, 30, 2
    parts = filters(oracle, C, B, P, banks=3)
    rng = np.random.default_rng(77)
    ms = [rng.random((C, P, B + 1)) < d for d in (0.5, 0.1, 0.3)]
    sig = signal(oracle, C, B, P, nb)
    ys = [oracle.dense_convolve(sig, masked(p, m), method=method).astype(np.float64) for p, m in zip(parts, ms)]
    tiles = [neo.sparse_plan(m, B)["kept_tiles"] for m in ms]
    tables = C * (2 * P * 1 + P + 1) * 4 + (C + 3) * 8  # bitmaps, window bitmaps, offsets, bases
    seen = {}

    def first(conv):
        assert conv.fade_info()["bank_bytes"] == 0 and conv.sparse_info()["kept_tiles"] == tiles[0]
        conv.update_filter(parts[1], ms[1], fade_blocks=F1)
        assert conv.fade_info() == {"remaining_blocks": F1, "fade_blocks": F1, "bank_bytes": tables + 128 * tiles[1]}
        assert conv.sparse_info()["kept_tiles"] == tiles[1]  # the bank being faded to

    def second(conv):
        assert conv.fade_info() == {"remaining_blocks": 0, "fade_blocks": 0, "bank_bytes": tables + 128 * tiles[0]}  # A, retired
        assert conv.sparse_info()["kept_tiles"] == tiles[1]
        torch.cuda.synchronize()
        seen["mem"] = neo.memory_info()
        conv.update_filter(parts[2], ms[2], fade_blocks=F2, curve="cosine")
        assert conv.fade_info()["bank_bytes"] == tables + 128 * tiles[2]  # the same tables, C's tiles
        assert conv.sparse_info()["kept_tiles"] == tiles[2]
        print(f"memory_info before / after the second update: {seen['mem']} / {neo.memory_info()}")

    got, conv = run(neo, torch, sig, B, sparse_maker(neo, C, B, P, parts[0], ms[0], method), {k1: first, k2: second})
    assert conv.sparse_info()["kept_tiles"] == tiles[2] and conv.fade_info()["bank_bytes"] == tables + 128 * tiles[1]
    conv.close()
    ref = mix(neo, mix(neo, ys[0], ys[1], B, k1, F1, "linear"), ys[2], B, k2, F2, "cosine")
    err = peak_err(got, ref)
    print(f"A -> B -> C {method}: peak err {err:.3g}")
    assert err <= TOL, err


# ---------------------------------------------------------------- 6. state rules
def _state_problem(oracle):
    C, B, P, nb = 2, 64, 12, 30
    parts = filters(oracle, C, B, P, banks=3)
    rng = np.random.default_rng(78)
    ms = [rng.random((C, P, B + 1)) < d for d in (0.4, 0.2, 0.6)]
    return C, B, P, nb, parts, ms, signal(oracle, C, B, P, nb)


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_reset_during_a_fade_leaves_b(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, parts, ms, sig = _state_problem(oracle)
    fresh, cb = run(neo, torch, sig, B, sparse_maker(neo, C, B, P, parts[1], ms[1], method))
    info_b = cb.sparse_info()
    cb.close()
    conv = sparse_maker(neo, C, B, P, parts[0], ms[0], method)()
    t = torch.from_numpy(np.array(sig)).cuda()
    conv.process_blocks(t[:, :7 * B].contiguous())
    conv.update_filter(parts[1], ms[1], fade_blocks=6)
    conv.set_batch(True)  # keeps the fade
    conv.process_blocks(t[:, 7 * B:9 * B].contiguous())
    conv.set_batch(False)
    assert conv.fade_info()["remaining_blocks"] == 4
    conv.reset()
    assert conv.fade_info()["remaining_blocks"] == 0 and conv.sparse_info() == info_b
    got, _ = run(neo, torch, sig, B, lambda: conv)
    conv.close()
    assert_same_bits(got, fresh, "after a reset during a fade")


def test_filter_during_a_fade_cancels_it(neo_gpu, oracle):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, parts, ms, sig = _state_problem(oracle)
    fresh, cc = run(neo, torch, sig, B, sparse_maker(neo, C, B, P, parts[2], ms[2], "upols"))
    cc.close()
    conv = sparse_maker(neo, C, B, P, parts[0], ms[0], "upols")()
    t = torch.from_numpy(np.array(sig)).cuda()
    conv.process_blocks(t[:, :7 * B].contiguous())
    conv.update_filter(parts[1], ms[1], fade_blocks=6)
    conv.process_blocks(t[:, 7 * B:9 * B].contiguous())
    conv.filter(parts[2], ms[2])
    assert conv.fade_info()["remaining_blocks"] == 0 and conv.fade_info()["fade_blocks"] == 0
    got, _ = run(neo, torch, sig, B, lambda: conv)
    conv.close()
    assert_same_bits(got, fresh, "after a filter() during a fade")


def test_update_during_a_fade_is_refused_and_changes_nothing(neo_gpu, oracle):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, parts, ms, sig = _state_problem(oracle)
    k, F = 9, 5
    make = sparse_maker(neo, C, B, P, parts[0], ms[0], "upols")
    want, c0 = run(neo, torch, sig, B, make, {k: lambda c: c.update_filter(parts[1], ms[1], fade_blocks=F)})
    c0.close()

    def refused(conv):
        before = (conv.fade_info(), conv.sparse_info())
        assert before[0]["remaining_blocks"] == F - 2
        with pytest.raises(neo._native.NeoHipError) as e:
            conv.update_filter(parts[2], ms[2], fade_blocks=2)
        assert e.value.code == EINVAL and "fade" in str(e.value)
        assert (conv.fade_info(), conv.sparse_info()) == before

    got, c1 = run(neo, torch, sig, B, make, {k: lambda c: c.update_filter(parts[1], ms[1], fade_blocks=F), k + 2: refused})
    c1.close()
    assert_same_bits(got, want, "a refused update changed the output")


# ---------------------------------------------------------------- 7. refusals
def test_refusals(neo_gpu, oracle):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    lib = neo._native.load()
    C, B, P, nb, parts, ms, sig = _state_problem(oracle)
    ir = np.stack([oracle.noise(79 + c, B * P) for c in range(C)])
    sp = neo.PerceptualSparsity(48000.0, -40.0)
    H = np.ascontiguousarray(parts[1])
    M = np.ascontiguousarray(ms[1], dtype=np.uint8)
    hp, mp = H.ctypes.data_as(ctypes.c_void_p), M.ctypes.data_as(ctypes.c_void_p)
    pp = sp._c()

    def einval(conv, fn, word=None):
        before = conv.fade_info(), (conv.sparse_info() if isinstance(conv, neo.SparseUpolsConvolver) else None)
        try:
            rc = fn()
        except neo._native.NeoHipError as e:
            assert e.code == EINVAL, e
            assert word is None or word in str(e), e
        else:
            assert rc == EINVAL, rc
        assert (conv.fade_info(), (conv.sparse_info() if isinstance(conv, neo.SparseUpolsConvolver) else None)) == before

    conv = neo.SparseUpolsConvolver(C, B, P)
    einval(conv, lambda: conv.update_filter(parts[1], ms[1]), "no filter")
    einval(conv, lambda: conv.update_filter(parts[1], sp), "no filter")
    einval(conv, lambda: conv.update_impulse(ir, sp), "no filter")
    conv.filter(parts[0], ms[0])
    blk = torch.from_numpy(np.array(sig)).cuda()
    n = blk.shape[1]

    def step(b):
        p = blk.data_ptr() + 4 * b * B
        conv.process_device(p, n, p, n, 0)

    for b in range(3):
        step(b)
    calls = [
        (lambda: lib.neo_hip_upols_update_filter_sparse(conv._h, None, mp, 0, 1, 0, None), None),  # null pointers
        (lambda: lib.neo_hip_upols_update_filter_sparse(conv._h, hp, None, 0, 1, 0, None), None),
        (lambda: lib.neo_hip_upols_update_filter_perceptual(conv._h, None, ctypes.byref(pp), 0, 1, 0, None), None),
        (lambda: lib.neo_hip_upols_update_filter_perceptual(conv._h, hp, None, 0, 1, 0, None), None),
        (lambda: lib.neo_hip_upols_update_impulse_perceptual(conv._h, None, B * P, 1, ctypes.byref(pp), 0, 1, 0, None), None),
        (lambda: lib.neo_hip_upols_update_impulse_perceptual(conv._h, ir.ctypes.data_as(ctypes.c_void_p), 0, 1,
                                                             ctypes.byref(pp), 0, 1, 0, None), None),
    ]
    calls += [(lambda F=F: conv.update_filter(parts[1], ms[1], fade_blocks=F), "fade_blocks") for F in (0, -3, (1 << 20) + 1)]
    calls += [(lambda F=F: conv.update_impulse(ir, sp, fade_blocks=F), "fade_blocks") for F in (0, (1 << 20) + 1)]
    calls += [(lambda cv=cv: conv.update_filter(parts[1], sp, curve=cv), "curve") for cv in (2, -1)]
    calls += [(lambda: conv.update_impulse(ir[:, :B * (P - 1)], sp), "partitions")]  # another P
    for fn, word in calls:
        einval(conv, fn, word)
    with pytest.raises(ValueError):
        conv.update_filter(parts[1], ms[1], curve="cubic")
    assert conv.fade_info() == {"remaining_blocks": 0, "fade_blocks": 0, "bank_bytes": 0}  # nothing was allocated
    step(3)  # the next block's bits are those of a handle that saw no refused call
    clean = sparse_maker(neo, C, B, P, parts[0], ms[0], "upols")()
    ref, _ = run(neo, torch, sig[:, :4 * B], B, lambda: clean)
    clean.close()
    torch.cuda.synchronize()
    assert_same_bits(blk[:, :4 * B].cpu().numpy(), ref, "blocks around the refused calls")
    conv.close()

    dense = neo.UpolsConvolver(C, B, P, options={"levels": 0})  # a dense handle given to the new calls
    dense.filter(parts[0])
    einval(dense, lambda: lib.neo_hip_upols_update_filter_sparse(dense._h, hp, mp, 0, 1, 0, None))
    einval(dense, lambda: lib.neo_hip_upols_update_filter_perceptual(dense._h, hp, ctypes.byref(pp), 0, 1, 0, None))
    einval(dense, lambda: lib.neo_hip_upols_update_impulse_perceptual(dense._h, ir.ctypes.data_as(ctypes.c_void_p), B * P, 1,
                                                                      ctypes.byref(pp), 0, 1, 0, None))
    assert b"sparse" in lib.neo_hip_last_error()
    dense.close()


# ---------------------------------------------------------------- 8. I/O contract
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_io_contract_through_a_fade(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, parts, ms, sig = _state_problem(oracle)
    nb, k, F = 24, 7, 3
    sig = sig[:, :nb * B]
    n = nb * B
    ya = oracle.dense_convolve(sig, masked(parts[0], ms[0]), method=method).astype(np.float64)
    yb = oracle.dense_convolve(sig, masked(parts[1], ms[1]), method=method).astype(np.float64)
    make = sparse_maker(neo, C, B, P, parts[0], ms[0], method)

    def drive(ip, li, op, lo, device=True):
        conv = make()
        for b in range(nb):
            if b == k:
                conv.update_filter(parts[1], ms[1], fade_blocks=F, curve="cosine")
            if device:
                conv.process_device(ip + 4 * b * B, li, op + 4 * b * B, lo, 0)
            else:
                conv.process_samples_ptr(ip + 4 * b * B, li, op + 4 * b * B, lo, B, False)
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
    # host buffers: separate strided arenas, then in place
    hi, ho = _host_arena(C, ld_in, IN_FILL, sig), _host_arena(C, ld_out, OUT_FILL)
    hb = hi.copy()
    drive(hi.ctypes.data + 4 * ld_in, ld_in, ho.ctypes.data + 4 * ld_out, ld_out, device=False)
    assert_same_bits(check_regions(ho, C, n, OUT_FILL, hb, hi), A, "host memory, separate padded buffers")
    hp = _host_arena(C, ld_out, IN_FILL, sig)
    drive(hp.ctypes.data + 4 * ld_out, ld_out, hp.ctypes.data + 4 * ld_out, ld_out, device=False)
    assert_same_bits(check_regions(hp, C, n, IN_FILL), A, "host memory, in place, padded")


# ---------------------------------------------------------------- 9, 10. a side stream; two runs
@pytest.mark.parametrize("method", ["upols", "upola"])
def test_cuda_tensors_on_a_side_stream_and_equal_runs(neo_gpu, oracle, method):
    torch = pytest.importorskip("torch")
    neo = neo_gpu
    C, B, P, nb, parts, ms, sig = _state_problem(oracle)
    k, F = 7, 3
    ya = oracle.dense_convolve(sig, masked(parts[0], ms[0]), method=method).astype(np.float64)
    yb = oracle.dense_convolve(sig, masked(parts[1], ms[1]), method=method).astype(np.float64)
    side = torch.cuda.Stream()
    outs = []
    for form in ("array mask", "tensor mask", "tensor mask"):
        conv = sparse_maker(neo, C, B, P, parts[0], ms[0], method)()
        with torch.cuda.stream(side):
            t = torch.from_numpy(np.array(sig)).cuda()
            n = t.shape[1]
            for b in range(nb):
                if b == k:
                    m = torch.from_numpy(ms[1]).cuda() if form == "tensor mask" else ms[1]
                    conv.update_filter(torch.from_numpy(np.array(parts[1])).cuda(), m, fade_blocks=F)
                p = t.data_ptr() + 4 * b * B
                conv.process_device(p, n, p, n, side.cuda_stream)
            side.synchronize()
        outs.append(t.cpu().numpy())
        conv.close()
        err = peak_err(outs[-1], mix(neo, ya, yb, B, k, F, "linear"))
        print(f"side stream, {form}, {method}: peak err {err:.3g}")
        assert err <= TOL, (form, err)
    assert_same_bits(outs[1], outs[0], "a tensor mask against an array mask")
    assert_same_bits(outs[2], outs[1], "a second identical run")
