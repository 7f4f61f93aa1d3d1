"""Batched passes of the sparse convolvers on the device (neo_hip_upols_set_batch on a sparse handle,
k_sparse_batch_mac): T blocks per pass over the kept filter tiles and the FDL tiles of the window
bitmaps.

The reference for every value test is the unchanged oracle on the MASKED DENSE filter,
oracle.dense_convolve(sig, parts * mask), as in tests/test_sparse_gpu.py. Tolerance: the project's
bar, 1e-5 peak-normalized (conftest.peak_err).

Shapes: the smallest at which each mechanism can fail --
  (2, 16, 7, 95)     one tile per row, a row of 16 bins in a 64-lane workgroup, P < T so every chunk
                     runs past P; batches 32, 32, 16, 8, 4, 2, 1
  (1, 32, 37, 120)   the ring of 68 rows wraps twice, P no multiple of T
  (3, 128, 9, 70)    two waves per workgroup
  (2, 512, 70, 140)  one bitmap word, one split
  (1, 256, 200, 270) three batch splits, the last one short and running past P
  (1, 1024, 20, 80)  two bitmap words
  (1, 4096, 3, 50)   eight words, 16 workgroups per row"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import peak_err
from test_sparse_gpu import masks, problem, reference

pytestmark = pytest.mark.gpu
TOL = 1e-5
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BIN = os.path.join(CPP, "bin")

#        C  B     P   blocks
SHAPES = [(2, 16, 7, 95), (1, 32, 37, 120), (3, 128, 9, 70), (2, 512, 70, 140), (1, 256, 200, 270),
          (1, 1024, 20, 80), (1, 4096, 3, 50)]
MIX = (2, 512, 70, 140)


def all_masks(C, B, P):
    """the five families of test_sparse_gpu.masks and the four corner cases"""
    out = dict(masks(C, B, P))
    shape = (C, P, B + 1)
    out["all-true"] = np.ones(shape, bool)
    out["all-false"] = np.zeros(shape, bool)
    m = np.zeros(shape, bool)
    m[:, P - 1, B - 16:B] = True  # the last partition's last tile
    out["last-tile"] = m
    m = np.zeros(shape, bool)
    m[:, 0] = True
    out["partition-0"] = m
    return out


def batched(neo, C, B, P, parts, mask, method, options=None):
    conv = neo.SparseUpolsConvolver(C, B, P, method=method, options=options)
    conv.filter(parts, mask)
    conv.set_batch(True)
    return conv


def run_batched(neo, C, B, P, parts, mask, sig, method):
    conv = batched(neo, C, B, P, parts, mask, method)
    out = sig.copy()
    conv.process(out)
    info = dict(conv.sparse_info(), **conv.sparse_batch_info())
    conv.close()
    return out, info


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb", SHAPES)
def test_batched_matches_oracle_on_masked_filter(neo_gpu, oracle, C, B, P, nb, method):
    parts, sig = problem(oracle, C, B, P, nb)
    for name, mask in all_masks(C, B, P).items():
        ref = reference(oracle, C, B, P, nb, name, mask, method)
        out, info = run_batched(neo_gpu, C, B, P, parts, mask, sig, method)
        plan = neo_gpu.sparse_plan(mask, B)
        T = info["blocks_per_pass"]
        assert T == 32
        want = neo_gpu.sparse_window_plan(plan["tile_mask"], B, T)["window_tiles"]
        assert info["window_tiles"] == want, (name, info["window_tiles"], want)
        assert info["kept_tiles"] == plan["kept_tiles"]
        if name == "all-false":
            assert info["kept_tiles"] == 0 and info["window_tiles"] == 0
            assert not out.any(), name
            continue
        err = peak_err(out, ref)
        print(f"{(C, B, P)} {method} {name}: peak err {err:.3g}, tiles {info['kept_tiles']}, "
              f"window tiles {info['window_tiles']}, splits {info['splits']}")
        assert err <= TOL, (name, err)


def test_default_is_unbatched_and_getters_follow_set_batch(neo_gpu, oracle):
    C, B, P, nb = 1, 256, 200, 270
    parts, _ = problem(oracle, C, B, P, nb)
    conv = neo_gpu.SparseUpolsConvolver(C, B, P)
    conv.filter(parts, masks(C, B, P)["bernoulli-0.1"])
    assert conv.batch_info() == (1, conv.splits)
    sb = conv.sparse_batch_info()
    assert sb["blocks_per_pass"] == 32 and sb["splits"] == 3  # 200 partitions / (2 x 32), whole chunks of 32: 96, 96, 8
    conv.set_batch(True)
    assert conv.batch_info() == (32, 3)
    conv.set_batch(False)
    assert conv.batch_info() == (1, conv.splits)
    lib = neo_gpu._native.load()
    E = neo_gpu._native.NEO_HIP_EINVAL
    conv.set_batch(True)
    for rc in (lib.neo_hip_upols_set_offline(conv._h, 1), lib.neo_hip_upols_set_ahead(conv._h, 1),
               lib.neo_hip_upols_set_persistent(conv._h, 1, 50.0), lib.neo_hip_upols_set_paced(conv._h, 1)):
        assert rc == E and b"sparse" in lib.neo_hip_last_error()
    conv.close()
    dense = neo_gpu.UpolsConvolver(1, B, 2)
    assert lib.neo_hip_upols_sparse_batch_info(dense._h, None, None, None) == E
    dense.close()


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_mixed_modes_on_one_handle(neo_gpu, oracle, method):
    C, B, P, nb = MIX
    parts, sig = problem(oracle, C, B, P, nb)
    name = "bernoulli-0.1"
    mask = masks(C, B, P)[name]
    conv = batched(neo_gpu, C, B, P, parts, mask, method)
    out = sig.copy()
    cuts = [(0, 40, True), (40, 43, False), (43, nb, True)]
    for b0, b1, on in cuts:
        conv.set_batch(on)
        piece = np.ascontiguousarray(out[:, b0 * B:b1 * B])
        conv.process(piece)
        out[:, b0 * B:b1 * B] = piece
    conv.close()
    err = peak_err(out, reference(oracle, C, B, P, nb, name, mask, method))
    print(f"mixed {method}: peak err {err:.3g}")
    assert err <= TOL


def test_reset_filter_change_and_determinism(neo_gpu, oracle):
    C, B, P, nb = MIX
    parts, sig = problem(oracle, C, B, P, nb)
    m = masks(C, B, P)
    for method in ("upols", "upola"):
        fresh, _ = run_batched(neo_gpu, C, B, P, parts, m["decaying"], sig, method)
        again, _ = run_batched(neo_gpu, C, B, P, parts, m["decaying"], sig, method)
        assert np.array_equal(fresh, again), method  # two fresh handles, the same calls
        assert peak_err(fresh, reference(oracle, C, B, P, nb, "decaying", m["decaying"], method)) <= TOL
        # reset in the middle, then the whole signal again
        conv = batched(neo_gpu, C, B, P, parts, m["decaying"], method)
        junk = sig[:, : 45 * B].copy()
        conv.process(junk)
        conv.reset()
        a = sig.copy()
        conv.process(a)
        assert np.array_equal(a, fresh), method
        # another mask after junk blocks: the window bitmaps are rebuilt
        conv.process(sig[:, : 37 * B].copy())
        conv.filter(parts, m["bernoulli-0.01"])
        assert conv.batch_info()[0] == 32  # batching stays on across a filter change
        b = sig.copy()
        conv.process(b)
        info = conv.sparse_batch_info()
        conv.close()
        other, oinfo = run_batched(neo_gpu, C, B, P, parts, m["bernoulli-0.01"], sig, method)
        assert np.array_equal(b, other), method
        assert info["window_tiles"] == oinfo["window_tiles"]
        assert peak_err(b, reference(oracle, C, B, P, nb, "bernoulli-0.01", m["bernoulli-0.01"], method)) <= TOL


@pytest.mark.parametrize("method", ["upols", "upola"])
def test_io_contract_on_the_batched_path(neo_gpu, oracle, method):
    import torch

    C, B, P, nb = MIX
    parts, sig = problem(oracle, C, B, P, nb)
    name = "bernoulli-0.5"
    mask = masks(C, B, P)[name]
    ref = reference(oracle, C, B, P, nb, name, mask, method)
    n = nb * B
    ld_in, ld_out = n + 36, n + 68
    nan = float("nan")
    x = torch.full((C, ld_in), nan, dtype=torch.float32, device="cuda")
    x[:, :n] = torch.from_numpy(sig.copy()).cuda()
    y = torch.full((C, ld_out), nan, dtype=torch.float32, device="cuda")
    x0 = x.clone()
    conv = batched(neo_gpu, C, B, P, parts, mask, method)
    s = torch.cuda.current_stream().cuda_stream
    conv.process_samples_ptr(x.data_ptr(), ld_in, y.data_ptr(), ld_out, n, True, s)
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(x0, nan=-7.0))  # in and its guards
    assert bool(torch.isnan(y[:, n:]).all())  # out's guard columns
    sep = y[:, :n].cpu().numpy()
    err = peak_err(sep, ref)
    print(f"separate I/O {method}: peak err {err:.3g}")
    assert err <= TOL
    # in place gives the same values
    conv.reset()
    z = x0.clone()
    conv.process_samples_ptr(z.data_ptr(), ld_in, z.data_ptr(), ld_in, n, True, s)
    torch.cuda.synchronize()
    assert np.array_equal(z[:, :n].cpu().numpy(), sep)
    assert bool(torch.isnan(z[:, n:]).all())
    # a misaligned pointer is refused and leaves the state as it was
    conv.reset()
    half = 40 * B
    w = x0.clone()
    conv.process_samples_ptr(w.data_ptr(), ld_in, w.data_ptr(), ld_in, half, True, s)
    E = neo_gpu._native.NEO_HIP_EINVAL
    lib = neo_gpu._native.load()
    before = w.clone()
    rc = lib.neo_hip_upols_process_samples(conv._h, ctypes.c_void_p(w.data_ptr() + 4 * half + 4), ld_in,
                                           ctypes.c_void_p(w.data_ptr() + 4 * half + 4), ld_in, n - half, 1,
                                           ctypes.c_void_p(s))
    assert rc == E and b"aligned" in lib.neo_hip_last_error()
    rc = lib.neo_hip_upols_process_samples(conv._h, ctypes.c_void_p(w.data_ptr() + 4 * half), ld_in + 2,
                                           ctypes.c_void_p(w.data_ptr() + 4 * half), ld_in + 2, n - half, 1,
                                           ctypes.c_void_p(s))
    assert rc == E
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(w, nan=-7.0), torch.nan_to_num(before, nan=-7.0))
    conv.process_samples_ptr(w.data_ptr() + 4 * half, ld_in, w.data_ptr() + 4 * half, ld_in, n - half, True, s)
    torch.cuda.synchronize()
    conv.close()
    assert peak_err(w[:, :n].cpu().numpy(), ref) <= TOL


def test_sparse_convolve_batches(neo_gpu, oracle):
    from perceptual_common import SAMPLE_RATE

    C, B, L, N = 2, 256, 2560, 256 * 37 + 77  # 38 blocks: batches of 32, 4 and 2
    ir = np.stack([oracle.noise(60 + c, L) for c in range(C)])
    sig = np.stack([oracle.noise(70 + c, N) for c in range(C)])
    parts = oracle.uniform_partition(oracle.normalize_impulse(ir), B)
    pad = np.zeros((C, -(-N // B) * B), np.float32)
    pad[:, :N] = sig
    sp = neo_gpu.PerceptualSparsity(SAMPLE_RATE, -40.0, 2, "a")
    dev_parts = neo_gpu.uniform_partition(neo_gpu.normalize_impulse(ir), B)
    cases = {"mask": (np.abs(parts) > np.median(np.abs(parts)),) * 2,  # a threshold on the bins, as the plugin's
             "perceptual": (sp, neo_gpu.perceptual_mask(dev_parts, sp))}
    for name, (arg, mask) in cases.items():
        mask = np.asarray(mask) != 0
        assert 0 < mask.sum() < mask.size
        for method in ("upola", "upols"):
            ref = oracle.dense_convolve(pad, (parts * mask).astype(np.complex64), method=method)[:, :N]
            got = neo_gpu.sparse_convolve(sig, ir, B, arg, method=method)
            err = peak_err(got, ref)
            print(f"sparse_convolve {name} {method}: peak err {err:.3g}")
            assert got.shape == (C, N) and err <= TOL, (name, method, err)


def build_cpp_test():
    """tests/cpp/test_sparse_batch.cpp against libneo_hip.so and the oracle (flags as tests/cpp/Makefile)."""
    os.makedirs(BIN, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "liboracle.so"])
    out = os.path.join(BIN, "test_sparse_batch")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(REPO, "include"),
                           "-o", out, os.path.join(CPP, "test_sparse_batch.cpp"),
                           "-L" + os.path.join(REPO, "neo-dsp_amd", "lib"), "-lneo_hip",
                           "-L" + os.path.join(REPO, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(REPO, "neo-dsp_amd", "lib"),
                           "-Wl,-rpath," + os.path.join(REPO, "oracle")])
    return out


def test_cpp_sparse_convolve_on_gpu():
    """The C++ sparse_convolve (both overloads, both methods) and upols_multichannel::batch against
    the oracle on the masked filter (<= 1e-5 peak)."""
    b = build_cpp_test()
    r = subprocess.run([b], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sparse batch C++ tests passed" in r.stdout
