"""Sparse UPOLS / UPOLA convolvers on the device (neo_hip_upols_create_sparse, k_upols_sparse_step).

The reference for every value test is the unchanged oracle on the MASKED DENSE filter,
oracle.dense_convolve(sig, parts * mask): the reference's CSR multiply_add adds exactly the kept
terms and adding x * 0 to a float sum changes nothing, so that is the reference's sparse result.
Tolerance: the project's bar, 1e-5 peak-normalized (conftest.peak_err).

Shapes: the smallest at which each mechanism can fail -- one tile per row (B = 16), two tiles and a
wrapping ring of P + 31 rows (B = 32, 80 blocks), exactly one bitmap word with P >= 64 (B = 512),
two words and two float4 per lane (B = 1024), eight words (B = 4096)."""
import ctypes

import numpy as np
import pytest

from conftest import peak_err

pytestmark = pytest.mark.gpu
TOL = 1e-5

#        C  B     P   blocks
SHAPES = [(2, 16, 7, 60), (1, 32, 37, 80), (3, 128, 9, 50), (2, 512, 70, 120), (1, 1024, 20, 60), (1, 4096, 3, 40)]
_cache = {}


def problem(oracle, C, B, P, nb):
    """Filter [C][P][B+1] and signal [C][nb B] of a shape, made once."""
    key = ("problem", C, B, P, nb)
    if key not in _cache:
        ir = np.stack([oracle.noise(900 + 7 * c + B, B * P) for c in range(C)])
        parts = oracle.uniform_partition(oracle.normalize_impulse(ir), B)
        sig = np.stack([oracle.noise(1900 + 7 * c + B, B * nb) for c in range(C)])
        parts.setflags(write=False)
        sig.setflags(write=False)
        _cache[key] = (parts, sig)
    return _cache[key]


def masks(C, B, P):
    rng = np.random.default_rng(4000 + B + P)
    shape = (C, P, B + 1)
    k = np.arange(B + 1)
    out = {f"bernoulli-{d}": rng.random(shape) < d for d in (0.5, 0.1, 0.01)}
    lim = np.floor(B * 0.5 ** (np.arange(P) / 8.0)).astype(int)
    out["decaying"] = np.broadcast_to(k[None, :] <= lim[:, None], shape).copy()  # DC always, Nyquist for p = 0 only
    m = rng.random(shape) < 0.3
    m[:, 1::3] = False
    m[:, P - 1] = False
    out["empty-rows"] = m
    return out


def reference(oracle, C, B, P, nb, name, mask, method):
    key = ("ref", C, B, P, nb, name, method)
    if key not in _cache:
        parts, sig = problem(oracle, C, B, P, nb)
        ref = oracle.dense_convolve(sig, (parts * mask).astype(np.complex64), method=method)
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def run_sparse(neo, C, B, P, parts, mask, sig, method, options=None):
    conv = neo.SparseUpolsConvolver(C, B, P, method=method, options=options)
    conv.filter(parts, mask)
    out = sig.copy()
    conv.process(out)
    info = conv.sparse_info()
    conv.close()
    return out, info


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb", SHAPES)
def test_sparse_matches_oracle_on_masked_filter(neo_gpu, oracle, C, B, P, nb, method):
    parts, sig = problem(oracle, C, B, P, nb)
    for name, mask in masks(C, B, P).items():
        ref = reference(oracle, C, B, P, nb, name, mask, method)
        plan = neo_gpu.sparse_plan(mask, B)
        for fused in (0, 1):
            out, info = run_sparse(neo_gpu, C, B, P, parts, mask, sig, method, {"fused": fused})
            err = peak_err(out, ref)
            print(f"{(C, B, P)} {method} {name} fused={fused}: peak err {err:.3g}, tiles {info['kept_tiles']}")
            assert err <= TOL, (name, fused, err)
            # the device setup computes the host plan's format
            assert info["kept_tiles"] == plan["kept_tiles"] and info["kept_bins"] == plan["kept_bins"] == int(mask.sum())
            nw = max(1, B // 512)
            assert info["filter_bytes"] == plan["kept_tiles"] * 128 + 4 * C * (P * nw + P + 1)


@pytest.mark.parametrize("C,B,P,nb", [(2, 512, 70, 120), (1, 1024, 20, 60), (2, 16, 7, 60)])
def test_sparse_equals_dense_plain_step_bit_for_bit(neo_gpu, oracle, C, B, P, nb):
    """One split per channel, the same fused choice, levels off: the sparse step runs the dense
    plain step's mac2 expressions in its order with the dropped terms left out, and a 0 * x term
    leaves a float sum unchanged -- equal bit for bit once -0 is canonicalised."""
    parts, sig = problem(oracle, C, B, P, nb)
    for name, mask in masks(C, B, P).items():
        if name not in ("bernoulli-0.5", "bernoulli-0.01", "decaying"):
            continue
        masked = np.ascontiguousarray(parts * mask, dtype=np.complex64)
        for method in ("upols", "upola"):
            for fused in (0, 1):
                opts = {"fused": fused, "split_workgroups": 1}
                sp = neo_gpu.SparseUpolsConvolver(C, B, P, method=method, options=opts)
                de = neo_gpu.UpolsConvolver(C, B, P, method=method, options=dict(opts, levels=0))
                assert sp.splits == 1 and de.splits == 1
                sp.filter(parts, mask)
                de.filter(masked)
                de.set_batch(False)  # the plain step, one block per pass
                a, b = sig.copy(), sig.copy()
                sp.process(a)
                de.process(b)
                sp.close()
                de.close()
                assert np.array_equal(a + 0.0, b + 0.0), (name, method, fused, float(np.abs(a - b).max()))


def test_all_true_is_dense_and_all_false_is_zero(neo_gpu, oracle):
    C, B, P, nb = 2, 512, 70, 120
    parts, sig = problem(oracle, C, B, P, nb)
    for method in ("upols", "upola"):
        key = ("dense-ref", method)
        if key not in _cache:
            _cache[key] = oracle.dense_convolve(sig, parts, method=method)
        out, info = run_sparse(neo_gpu, C, B, P, parts, np.ones(parts.shape, bool), sig, method)
        assert peak_err(out, _cache[key]) <= TOL
        assert info["kept_tiles"] == C * P * (B // 16) and info["kept_bins"] == C * P * (B + 1)
        out, info = run_sparse(neo_gpu, C, B, P, parts, np.zeros(parts.shape, bool), sig, method)
        assert info["kept_tiles"] == 0 and info["kept_bins"] == 0
        assert not out.any()


@pytest.mark.parametrize("B", [128, 256, 512, 1024])
def test_reference_identity_test_both_aliases(neo_gpu, oracle, B):
    """uniform_partitioned_convolver_test.cpp:35-75: identity impulse of 3 partitions, an
    always-true predicate, 20 noise blocks; output equals input to 1e-5."""
    filt = np.zeros((3, B + 1), np.complex64)
    filt[0] = 1.0
    signal = oracle.noise(B, B * 20)
    for cls in (neo_gpu.sparse_upols_convolver, neo_gpu.sparse_upola_convolver):
        conv = cls()
        conv.filter(filt, lambda row, col, value: True)
        out = signal.copy()
        for i in range(0, out.size, B):
            conv(out[i:i + B])
        assert np.abs(out - signal).max() <= 1e-5, cls.__name__


def test_filter_twice_resets_state(neo_gpu, oracle):
    C, B, P, nb = 3, 128, 9, 50
    parts, sig = problem(oracle, C, B, P, nb)
    m = masks(C, B, P)
    conv = neo_gpu.SparseUpolsConvolver(C, B, P)
    conv.filter(parts, m["bernoulli-0.5"])
    junk = sig[:, : 7 * B].copy()
    conv.process(junk)
    conv.filter(parts, m["decaying"])
    assert conv.sparse_info()["kept_tiles"] == neo_gpu.sparse_plan(m["decaying"], B)["kept_tiles"]
    a = sig.copy()
    conv.process(a)
    conv.close()
    b, _ = run_sparse(neo_gpu, C, B, P, parts, m["decaying"], sig, "upols")
    assert np.array_equal(a, b)
    assert peak_err(a, reference(oracle, C, B, P, nb, "decaying", m["decaying"], "upols")) <= TOL


def test_refused_setters_leave_the_handle_usable(neo_gpu, oracle):
    C, B, P, nb = 3, 128, 9, 50
    parts, sig = problem(oracle, C, B, P, nb)
    mask = masks(C, B, P)["bernoulli-0.5"]
    lib = neo_gpu._native.load()
    E = neo_gpu._native.NEO_HIP_EINVAL
    conv = neo_gpu.SparseUpolsConvolver(C, B, P)
    conv.filter(parts, mask)
    half = (nb // 2) * B
    out = sig.copy()
    conv.process(out[:, :half].copy())  # state advances; the refusals below must not disturb it
    conv.reset()
    first = np.ascontiguousarray(out[:, :half])
    conv.process(first)
    h = conv._h
    ir = np.zeros((C, B * P), np.float32)
    for rc, word in ((lib.neo_hip_upols_set_filter(h, parts.ctypes.data_as(ctypes.c_void_p), 0), b"sparse"),
                     (lib.neo_hip_upols_set_impulse(h, ir.ctypes.data_as(ctypes.c_void_p), B * P, 1, 0), b"sparse"),
                     (lib.neo_hip_upols_set_ahead(h, 1), b"sparse"),
                     (lib.neo_hip_upols_set_offline(h, 1), b"sparse"),
                     (lib.neo_hip_upols_set_persistent(h, 1, 50.0), b"sparse"),
                     (lib.neo_hip_upols_set_paced(h, 1), b"sparse"),
                     (lib.neo_hip_upols_set_paced(h, 2), b"sparse")):
        assert rc == E
        assert word in lib.neo_hip_last_error()
    dense = neo_gpu.UpolsConvolver(1, B, 2)
    m1 = np.ones((1, 2, B + 1), np.uint8)
    f1 = np.zeros((1, 2, B + 1), np.complex64)
    assert lib.neo_hip_upols_set_filter_sparse(dense._h, f1.ctypes.data_as(ctypes.c_void_p),
                                               m1.ctypes.data_as(ctypes.c_void_p), 0) == E
    assert lib.neo_hip_upols_sparse_info(dense._h, None, None, None) == E
    dense.close()
    # the getters report off; turning things off is accepted
    assert conv.ahead_info()[0] == 0 and conv.offline_info()[0] == 0 and conv.batch_info()[0] == 1
    assert not conv.persistent_info()["enabled"]
    conv.set_ahead(False)
    conv.set_offline(False)
    conv.set_persistent(False)
    conv.set_paced(0)
    second = np.ascontiguousarray(out[:, half:])
    conv.process(second)
    conv.close()
    ref = reference(oracle, C, B, P, nb, "bernoulli-0.5", mask, "upols")
    assert peak_err(np.concatenate([first, second], axis=1), ref) <= TOL


def test_process_blocks_equals_single_calls(neo_gpu, oracle):
    import torch

    C, B, P, nb = 2, 512, 70, 120
    parts, sig = problem(oracle, C, B, P, nb)
    mask = masks(C, B, P)["bernoulli-0.1"]
    a = neo_gpu.SparseUpolsConvolver(C, B, P)
    b = neo_gpu.SparseUpolsConvolver(C, B, P)
    a.filter(torch.from_numpy(parts.copy()).cuda(), torch.from_numpy(mask).cuda())  # device filter and mask
    b.filter(parts, mask)
    x = torch.from_numpy(sig[:, : 5 * B].copy()).cuda()
    ya = a.process_blocks(x.clone())
    yb = x.clone()
    for t in range(5):
        blk = yb[:, t * B:(t + 1) * B].contiguous()
        b(blk)
        yb[:, t * B:(t + 1) * B] = blk
    torch.cuda.synchronize()
    a.close()
    b.close()
    assert torch.equal(ya, yb)
    ref = reference(oracle, C, B, P, nb, "bernoulli-0.1", mask, "upols")[:, : 5 * B]
    assert peak_err(ya.cpu().numpy(), ref) <= TOL


def test_sparse_convolve_follows_the_plugin_loop(neo_gpu, oracle):
    C, B, L, N = 2, 256, 2560, 256 * 9 + 77
    ir = np.stack([oracle.noise(60 + c, L) for c in range(C)])
    sig = np.stack([oracle.noise(70 + c, N) for c in range(C)])
    parts = oracle.uniform_partition(oracle.normalize_impulse(ir), B)
    mask = np.abs(parts) > np.median(np.abs(parts))  # a threshold on the bins, as the plugin's
    pad = np.zeros((C, -(-N // B) * B), np.float32)
    pad[:, :N] = sig
    for method in ("upola", "upols"):
        ref = oracle.dense_convolve(pad, (parts * mask).astype(np.complex64), method=method)[:, :N]
        got = neo_gpu.sparse_convolve(sig, ir, B, mask, method=method)
        assert got.shape == (C, N) and peak_err(got, ref) <= TOL
