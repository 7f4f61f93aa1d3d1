"""neo.convolution on MI355X: UPOLS convolvers, uniform_partition, normalize_impulse.

Mirrors the reference's C++ convolution API (the reference binds no UPOLS in
Python; extra/python/src/main.cpp:227-234 only lists the `upols` method enum):
  - uniform_partition      src/neo/convolution/uniform_partition.hpp:12-26
  - normalize_impulse      src/neo/convolution/normalize_impulse.hpp:11-33
  - upols_convolver        src/neo/convolution/dense_convolver.hpp:19-20 +
                           uniform_partitioned_convolver.hpp:13-65
  - split_upols_convolver  dense_convolver.hpp:38-42 (same math, SoA on the CPU;
                           one device layout here)
  - upola_convolver        dense_convolver.hpp:23-24 (overlap_add.hpp:76-106 stage)
  - upola_convolver_v2     dense_convolver.hpp:28 (overlap_add_convolver.hpp:20-136,
                           sub-block input)
  - dense_convolve         extra/plugin/src/dsp/DenseConvolution.hpp:39-70
  - UpolsConvolver64       upols_convolver / upola_convolver of complex<double> (dtype=np.float64 on
                           uniform_partition, normalize_impulse, dense_convolve and the two classes)
                           with set_batch(): calls of many blocks in passes of 16 blocks
  - sparse_upols_convolver / sparse_upola_convolver
                           src/neo/convolution/sparse_convolver.hpp:12-17 (sparse_filter.hpp:25-45;
                           kept in 128-byte tiles of 16 bins here, include/neo_hip.h)
  - MatrixConvolver        no reference class: output o = the sum over its routes (o, i) of
                           upols_convolver / upola_convolver on (x_i, h[o][i]) (include/neo_hip.h)
  - sparse_convolve        extra/plugin/src/dsp/DenseConvolution.cpp:124-186 (a mask of the caller's, or
                           the plugin's A-weighted threshold: PerceptualSparsity, perceptual_mask,
                           perceptual_histogram; a_weighting, amplitude_to_db as main.cpp:260-267)
Everything runs on the GPU through libneo_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native

__all__ = [
    "num_partitions",
    "host_register",
    "host_unregister",
    "uniform_partition",
    "normalize_impulse",
    "UpolsConvolver",
    "upols_convolver",
    "split_upols_convolver",
    "OverlapStage",
    "UpolsGroup",
    "overlap_save",
    "overlap_add",
    "upola_convolver",
    "split_upola_convolver",
    "upola_convolver_v2",
    "dense_convolve",
    "SparseUpolsConvolver",
    "sparse_upols_convolver",
    "sparse_upola_convolver",
    "sparse_plan",
    "sparse_window_plan",
    "sparse_fade_plan",
    "sparse_convolve",
    "MatrixConvolver",
    "matrix_plan",
    "matrix_batch_plan",
    "matrix_offline_plan",
    "matrix_level_plan",
    "matrix_convolve",
    "matrix_fade_gains",
    "fade_gains",
    "a_weighting",
    "amplitude_to_db",
    "PerceptualSparsity",
    "perceptual_weights",
    "perceptual_mask",
    "perceptual_mask_host",
    "perceptual_histogram",
    "perceptual_histogram_host",
    "tile_density_curve",
    "threshold_for_tile_density",
    "fft_convolve",
    "direct_convolve",
    "convolve",
    "UpolsConvolver64",
    "upols64_plan",
    "upols64_batch_plan",
    "upols64_offline_plan",
]


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda")


def _ptr(a: np.ndarray) -> ctypes.c_void_p:
    return a.ctypes.data_as(ctypes.c_void_p)


def _producer_join(t) -> None:
    """A device tensor handed to a synchronous setup call (filter, impulse, normalize, partition)
    is complete first: torch's current stream is its producer. The library orders such an input
    after the null stream (torch's default stream) itself, with a marker event, never after the
    whole device (a resident latency-mode kernel on another handle); a side stream
    (`with torch.cuda.stream(s)`) is synchronized here, that stream alone."""
    import torch

    s = torch.cuda.current_stream(t.device)
    if s.cuda_stream != 0:
        s.synchronize()


def num_partitions(length: int, block: int) -> int:
    """P = ceil(L / B) (stft.hpp:21-25 with overlap 0; clamped to 1 for L < B)."""
    p = ctypes.c_int64()
    _native.check(_native.load().neo_hip_num_partitions(int(length), int(block), ctypes.byref(p)))
    return p.value


def level_plan(partitions: int) -> dict:
    """The streaming level plan of a convolver with `partitions` partitions
    (neo_hip_upols_level_plan; no device needed): the block step takes [0, a0), Toeplitz
    level l a window of T[l] blocks over the band [a[l], b[l]), and nseg far segments of
    128 partitions from 256."""
    L = _native.load()
    a0, nl, ns = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    T, a, b = (ctypes.c_int * 8)(), (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    _native.check(L.neo_hip_upols_level_plan(int(partitions), ctypes.byref(a0), ctypes.byref(nl), T, a, b,
                                             ctypes.byref(ns)))
    n = nl.value
    return {"a0": a0.value, "T": list(T[:n]), "a": list(a[:n]), "b": list(b[:n]), "nseg": ns.value}


def part_plan(channels: int, block: int, partitions: int, step_group: int, uniform: bool = False) -> dict:
    """The background plan of step groups of `step_group` blocks (neo_hip_upols_part_plan; no
    device needed): per Toeplitz level the window offset phi, the cycle length in step groups,
    per background level (T >= 2 step_group) the unit cuts of each window of the cycle
    ({level: [[T / G cuts of window k], ...]}) and the predicted background bytes per step group
    of the cycle; uniform: equal parts, no offsets."""
    if step_group < 2:
        raise ValueError("part_plan: step groups of >= 2 blocks")
    L = _native.load()
    lp = level_plan(partitions)
    phi, cyc, nc = (ctypes.c_int * 8)(), ctypes.c_int(), ctypes.c_int()
    loads = (ctypes.c_double * 512)()
    args = (int(channels), int(block), int(partitions), int(step_group), int(uniform), phi, ctypes.byref(cyc))
    _native.check(L.neo_hip_upols_part_plan(*args, None, 0, ctypes.byref(nc), loads, 512))
    cuts = (ctypes.c_int * max(1, nc.value))()
    _native.check(L.neo_hip_upols_part_plan(*args, cuts, nc.value, ctypes.byref(nc), loads, 512))
    flat, out, i = list(cuts[:nc.value]), {}, 0
    for l, T in enumerate(lp["T"]):
        if T < 2 * step_group:
            continue  # in the block launches
        Tg = T // step_group
        out[l] = [flat[i + k:i + k + Tg] for k in range(0, cyc.value, Tg)]
        i += cyc.value
    return {"phi": list(phi[:len(lp["T"])]), "cycle": cyc.value, "cuts": out, "loads": list(loads[:cyc.value])}


def stagger_plan(channels: int, block: int, partitions: int, step_group: int = 0, far_group: int = 0) -> dict:
    """The staggered plan (options windows = 2) of a convolver with step groups of `step_group`
    blocks (neo_hip_upols_stagger_plan; no device needed). Returns a0, the levels' T / a / b and
    `staggered` flags, the far level's first partition `far_a` and `nseg`, `even_share` (1/1024ths
    of a class pair), `step_group`, and `classes`: {level index, or "far": [(first channel, end
    channel, group residue, window start modulo T), ...]} -- class k of a level of window T is
    computed in the background launches of the groups g = k mod T / G for its window starting at
    block (g + 2) G (far: phase 2 there, phase 1 two groups before) -- and `loads`, the predicted
    background bytes per group over the far window."""
    L = _native.load()
    nl, fa, ns, ef, nc, nld = (ctypes.c_int() for _ in range(6))
    T, a, b, st = ((ctypes.c_int * 8)() for _ in range(4))
    cuts, offs, loads = (ctypes.c_int * 256)(), (ctypes.c_int * 256)(), (ctypes.c_double * 64)()
    _native.check(L.neo_hip_upols_stagger_plan(int(channels), int(block), int(partitions), int(step_group),
                                               int(far_group), ctypes.byref(nl), T, a, b, st, ctypes.byref(fa),
                                               ctypes.byref(ns), ctypes.byref(ef), cuts, offs, 256, ctypes.byref(nc),
                                               loads, 64, ctypes.byref(nld)))
    n = nl.value
    out = {"a0": min(partitions, 8), "T": list(T[:n]), "a": list(a[:n]), "b": list(b[:n]),
           "staggered": [bool(v) for v in st[:n]], "far_a": fa.value, "nseg": ns.value, "even_share": ef.value,
           "loads": list(loads[:nld.value]), "classes": {}}
    G = out["step_group"] = 128 // nld.value
    i = 0
    for key, Tl in [(l, T[l]) for l in range(n) if st[l]] + ([("far", 128)] if ns.value else []):
        k = Tl // G
        out["classes"][key] = [(cuts[i + j], cuts[i + j + 1], j, offs[i + j]) for j in range(k)]
        i += k + 1
    assert i == nc.value
    return out


def host_register(array: np.ndarray) -> np.ndarray:
    """Page-lock a host array in place (neo_hip_host_register) so that host-buffer calls
    (UpolsConvolver.__call__) read and write it over PCIe without staging; call
    host_unregister before the array is freed."""
    if not (isinstance(array, np.ndarray) and array.flags.c_contiguous):
        raise TypeError("host_register takes a C-contiguous ndarray")
    _native.check(_native.load().neo_hip_host_register(_ptr(array), array.nbytes))
    return array


def host_unregister(array: np.ndarray) -> None:
    _native.check(_native.load().neo_hip_host_unregister(_ptr(array)))


def memory_info(device: int = 0) -> dict:
    """Device memory the library holds for convolver handles on `device` (neo_hip_memory_info):
    bytes reserved in its cached chunks and bytes in use by live handles."""
    r, u = ctypes.c_int64(), ctypes.c_int64()
    _native.check(_native.load().neo_hip_memory_info(device, ctypes.byref(r), ctypes.byref(u)))
    return {"reserved": r.value, "in_use": u.value}


def memory_trim(device: int = 0) -> None:
    """Return every cached chunk no handle uses to the driver (neo_hip_memory_trim)."""
    _native.check(_native.load().neo_hip_memory_trim(device))


def _f64(dtype) -> bool:
    """The dtype keyword of the float32 / float64 entry points: True for float64."""
    dt = np.dtype(dtype)
    if dt == np.float32:
        return False
    if dt == np.float64:
        return True
    raise TypeError(f"dtype must be np.float32 or np.float64, got {dtype!r}")


def uniform_partition(impulse_response, block_size: int, device: int = 0, *, dtype=np.float32):
    """[C][L] float32 -> [C][P][B+1] complex64: rfft_2B of each zero-padded B-sample partition.
    A CUDA tensor gives a CUDA tensor on its device (no host copies). dtype=np.float64: computed
    in double on the device, [C][L] float64 -> [C][P][B+1] complex128."""
    if _f64(dtype):
        lib = _native.load()
        if _is_torch(impulse_response) and impulse_response.is_cuda:
            import torch

            t = impulse_response
            if t.dtype != torch.float64 or not t.is_contiguous():
                raise TypeError("uniform_partition(dtype=float64) takes a contiguous float64 tensor")
            C, L = (1, t.shape[0]) if t.dim() == 1 else tuple(t.shape)
            P = num_partitions(L, block_size)
            out = torch.empty((C, P, block_size + 1), dtype=torch.complex128, device=t.device)
            _producer_join(t)
            _native.check(lib.neo_hip_uniform_partition_f64(ctypes.c_void_p(t.data_ptr()), C, L, int(block_size),
                                                            ctypes.c_void_p(out.data_ptr()), 1, t.device.index or 0))
            return out
        ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float64)))
        C, L = ir.shape
        P = num_partitions(L, block_size)
        out = np.empty((C, P, block_size + 1), dtype=np.complex128)
        _native.check(lib.neo_hip_uniform_partition_f64(_ptr(ir), C, L, int(block_size), _ptr(out), 0, int(device)))
        return out
    if _is_torch(impulse_response) and impulse_response.is_cuda:
        import torch

        t = impulse_response
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("uniform_partition takes a contiguous float32 tensor")
        C, L = (1, t.shape[0]) if t.dim() == 1 else tuple(t.shape)
        P = num_partitions(L, block_size)
        out = torch.empty((C, P, block_size + 1), dtype=torch.complex64, device=t.device)
        _producer_join(t)
        _native.check(_native.load().neo_hip_uniform_partition(ctypes.c_void_p(t.data_ptr()), C, L, int(block_size),
                                                               ctypes.c_void_p(out.data_ptr()), 1, t.device.index or 0))
        return out
    ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float32)))
    C, L = ir.shape
    P = num_partitions(L, block_size)
    out = np.empty((C, P, block_size + 1), dtype=np.complex64)
    _native.check(_native.load().neo_hip_uniform_partition(_ptr(ir), C, L, int(block_size), _ptr(out), 0, int(device)))
    return out


def normalize_impulse(impulse_response, device: int = 0, *, dtype=np.float32):
    """In place: scale every channel by min_c 1/sqrt(sum(ir[c]^2)), rounded exactly like the
    reference's sequential float sum. Accepts a float32 ndarray (rank 1 or 2) or CUDA tensor.
    dtype=np.float64: a float64 ndarray or CUDA tensor, in double (the energy summed in a fixed
    order, not the reference's sequential one: the two agree to ~1e-13)."""
    if _f64(dtype):
        lib = _native.load()
        if _is_torch(impulse_response):
            import torch

            t = impulse_response
            if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
                raise TypeError("normalize_impulse(dtype=float64) works in place on a contiguous float64 CUDA tensor")
            C, L = (1, t.shape[0]) if t.dim() == 1 else tuple(t.shape)
            _producer_join(t)
            _native.check(lib.neo_hip_normalize_impulse_f64(ctypes.c_void_p(t.data_ptr()), C, L, 1, t.device.index or 0))
            return t
        a = impulse_response
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
            raise TypeError("normalize_impulse(dtype=float64) works in place on a C-contiguous float64 array")
        C, L = (1, a.shape[0]) if a.ndim == 1 else a.shape
        _native.check(lib.neo_hip_normalize_impulse_f64(_ptr(a), C, L, 0, int(device)))
        return a
    if _is_torch(impulse_response):
        t = impulse_response
        C, L = (1, t.shape[0]) if t.dim() == 1 else tuple(t.shape)
        _producer_join(t)
        _native.check(_native.load().neo_hip_normalize_impulse(ctypes.c_void_p(t.data_ptr()), C, L, 1,
                                                               t.device.index or 0))
        return t
    a = impulse_response
    if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous):
        raise TypeError("normalize_impulse works in place on a C-contiguous float32 array")
    C, L = (1, a.shape[0]) if a.ndim == 1 else a.shape
    _native.check(_native.load().neo_hip_normalize_impulse(_ptr(a), C, L, 0, int(device)))
    return a


class UpolsConvolver:
    """C independent UPOLS convolvers stepped together (one launch pair per block).

    State lives in HBM: filter [C][P][B] and FDL [C][P][B] (packed bins),
    previous block [C][B]. Blocks are processed in place, zero latency
    (output block t corresponds to input block t, overlap_save.hpp:84-112).
    """

    OPTION_DEFAULTS = {"fused": -1, "split_workgroups": 0, "batch_blocks": 0, "batch_bins": 0, "levels": -1,
                       "far_level": -1, "far_group": 0, "toep_split": 0, "step_group": 0,
                       "far_phase2": 0, "windows": 0}

    def __init__(self, channels: int, block_size: int, partitions: int, device: int = 0, method: str = "upols",
                 options: dict | None = None):
        """`options` (neo_hip_upols_create_ex): explicit code-path choices instead of the
        shape-based defaults — fused (-1 auto / 0 / 1), split_workgroups (0 auto),
        batch_blocks (0 auto / 2..32), batch_bins (0 auto / 1 / 2), levels (-1 auto / 0 / 1),
        far_level (-1 auto / 0 Toeplitz window of 128 blocks / 1 partition-axis transform with stored spectra /
        2 the transform recomputed every window, for p >= 256),
        far_group (0 auto / 1..4 windows per far phase-1 pass over the stored segment spectra),
        toep_split (0 auto / 1 / 2 window parts per unit of the 32-block Toeplitz level),
        step_group (0 auto / 1 one launch per block / 2 or 4: the block of every call alone on the
        caller's stream, the level slices of G calls as one launch on a background stream),
        far_phase2 (G = 1: 0 auto / 1 one workgroup per unit / 2 the fresh transform one step
        before the products), windows (step groups: 0 auto / 1 aligned level windows / 2 staggered: a
        window phase per class of channels, bands from T + 4 G, fewer rows per step; see stagger_plan).
        Every choice gives the same results up to float summation order."""
        lib = _native.load()
        h = ctypes.c_void_p()
        methods = {"upols": 0, "upola": 1, "upola_v2": 2}
        if method not in methods:
            raise ValueError(f"method must be 'upols', 'upola' or 'upola_v2', got {method!r}")
        opts = dict(self.OPTION_DEFAULTS)
        for k, v in (options or {}).items():
            if k not in opts:
                raise ValueError(f"unknown convolver option {k!r}")
            opts[k] = int(v)
        o = _native.UpolsOpts(**opts)
        _native.check(lib.neo_hip_upols_create_ex(int(channels), int(block_size), int(partitions), int(device),
                                                  methods[method], ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        self.channels, self.block_size, self.partitions, self.device = channels, block_size, partitions, device
        self.method = method

    # -- setup ------------------------------------------------------------
    def filter(self, partitions) -> None:
        """uniform_partitioned_convolver::filter(): [C][P][B+1] complex64 (host array or
        CUDA tensor); resets FDL, window and write position."""
        if _is_torch(partitions):
            _producer_join(partitions)
            _native.check(_native.load().neo_hip_upols_set_filter(self._h, ctypes.c_void_p(partitions.data_ptr()), 1))
            return
        H = np.ascontiguousarray(partitions, dtype=np.complex64)
        if H.ndim == 2:
            H = H[None]
        if H.shape != (self.channels, self.partitions, self.block_size + 1):
            raise ValueError(f"filter shape {H.shape} != {(self.channels, self.partitions, self.block_size + 1)}")
        _native.check(_native.load().neo_hip_upols_set_filter(self._h, _ptr(H), 0))

    def set_impulse(self, impulse_response, normalize: bool = True) -> None:
        """normalize_impulse (optional) + uniform_partition straight into the device filter."""
        if _is_torch(impulse_response):
            t = impulse_response
            _producer_join(t)
            _native.check(_native.load().neo_hip_upols_set_impulse(self._h, ctypes.c_void_p(t.data_ptr()),
                                                                   t.shape[-1], int(normalize), 1))
            return
        ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float32)))
        if ir.shape[0] != self.channels:
            raise ValueError("impulse channel count mismatch")
        _native.check(_native.load().neo_hip_upols_set_impulse(self._h, _ptr(ir), ir.shape[1], int(normalize), 0))

    def reset(self) -> None:
        """Clears all state; a running fade (update_filter) completes: the new filter is the filter."""
        _native.check(_native.load().neo_hip_upols_reset(self._h))

    # -- live updates -------------------------------------------------------
    def update_filter(self, partitions, fade_blocks: int = 1, curve: str = "linear", stream: int = 0) -> None:
        """Live update (neo_hip_upols_update_filter): crossfade to `partitions` [C][P][B+1] complex64
        over the next fade_blocks blocks and KEEP ALL STATE (delay line, previous block, overlap-add
        tail); filter() remains the resetting call. Sample n of the fade is y_A + g[n] (y_B - y_A)
        with g = fade_gains(block_size, fade_blocks, curve), curve "linear" or "cosine"; every
        block of the fade runs as one two-bank step (about a plain step and a half), whatever the
        handle's modes. A CUDA tensor: asynchronous on torch's current stream (or `stream`), which
        must be the stream the process calls run on; an ndarray: complete on return. Dense upols /
        upola convolvers only (not sparse, upola_v2, group members or latency mode)."""
        c = _fade_curve(curve)
        lib = _native.load()
        if _is_torch(partitions) and partitions.is_cuda:
            import torch

            if (partitions.dtype != torch.complex64 or not partitions.is_contiguous() or
                    partitions.numel() != self.channels * self.partitions * (self.block_size + 1)):
                raise ValueError(f"filter must be a contiguous complex64 tensor of "
                                 f"{(self.channels, self.partitions, self.block_size + 1)}")
            _producer_join(partitions)
            current = torch.cuda.current_stream(partitions.device).cuda_stream
            _native.check(lib.neo_hip_upols_update_filter(self._h, ctypes.c_void_p(partitions.data_ptr()), 1,
                                                          int(fade_blocks), c, ctypes.c_void_p(stream or current or None)))
            return
        H = np.ascontiguousarray(partitions, dtype=np.complex64)
        if H.ndim == 2:
            H = H[None]
        if H.shape != (self.channels, self.partitions, self.block_size + 1):
            raise ValueError(f"filter shape {H.shape} != {(self.channels, self.partitions, self.block_size + 1)}")
        _native.check(lib.neo_hip_upols_update_filter(self._h, _ptr(H), 0, int(fade_blocks), c,
                                                      ctypes.c_void_p(stream or None)))

    def update_impulse(self, impulse_response, normalize: bool = True, fade_blocks: int = 1, curve: str = "linear",
                       stream: int = 0) -> None:
        """update_filter from impulse responses [C][L] float32 (host array or CUDA tensor):
        normalize_impulse over the new impulse's channels (optional), then uniform_partition on the
        device straight into the second bank (neo_hip_upols_update_impulse). Keeps all state."""
        c = _fade_curve(curve)
        lib = _native.load()
        if _is_torch(impulse_response) and impulse_response.is_cuda:
            import torch

            t = impulse_response
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.channels * t.shape[-1]:
                raise ValueError("impulse must be a contiguous float32 tensor of one row per channel")
            _producer_join(t)
            current = torch.cuda.current_stream(t.device).cuda_stream
            _native.check(lib.neo_hip_upols_update_impulse(self._h, ctypes.c_void_p(t.data_ptr()), t.shape[-1],
                                                           int(normalize), 1, int(fade_blocks), c,
                                                           ctypes.c_void_p(stream or current or None)))
            return
        ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float32)))
        if ir.shape[0] != self.channels:
            raise ValueError("impulse channel count mismatch")
        _native.check(lib.neo_hip_upols_update_impulse(self._h, _ptr(ir), ir.shape[1], int(normalize), 0,
                                                       int(fade_blocks), c, ctypes.c_void_p(stream or None)))

    def fade_info(self) -> dict:
        """remaining_blocks of the running fade (0: none), its fade_blocks (0: none) and bank_bytes,
        the second filter bank (0 until the first update; kept from then on)."""
        r, f, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols_fade_info(self._h, ctypes.byref(r), ctypes.byref(f), ctypes.byref(n)))
        return {"remaining_blocks": r.value, "fade_blocks": f.value, "bank_bytes": n.value}

    # -- processing ---------------------------------------------------------
    def __call__(self, block, stream: int = 0):
        """Process one block [C][B] in place (float32 ndarray or CUDA tensor)."""
        if _is_torch(block):
            import torch

            assert block.dtype == torch.float32 and block.is_contiguous()
            if block.numel() != self.channels * self.block_size:
                raise ValueError("block must hold channels * block_size samples")
            if not block.is_cuda:  # host tensor (pinned ones are read and written in place)
                _native.check(_native.load().neo_hip_upols_process(self._h, ctypes.c_void_p(block.data_ptr()), 0,
                                                                   None))
                return block
            s = stream or torch.cuda.current_stream(block.device).cuda_stream
            _native.check(_native.load().neo_hip_upols_process(self._h, ctypes.c_void_p(block.data_ptr()), 1,
                                                               ctypes.c_void_p(s)))
            return block
        if not (isinstance(block, np.ndarray) and block.dtype == np.float32 and block.flags.c_contiguous):
            raise TypeError("block must be a C-contiguous float32 array")
        if block.size != self.channels * self.block_size:
            raise ValueError("block must hold channels * block_size samples")
        _native.check(_native.load().neo_hip_upols_process(self._h, _ptr(block), 0, None))
        return block

    def process(self, samples, stream: int = 0):
        """Any number of samples per channel, in place: [C][n] float32 ndarray or CUDA
        tensor. upola_v2 splits at block boundaries like overlap_add_convolver::operator()
        (overlap_add_convolver.hpp:80-134); upols/upola need n % block_size == 0."""
        lib = _native.load()
        if _is_torch(samples):
            import torch

            assert samples.dtype == torch.float32 and samples.is_contiguous()
            n = samples.shape[-1]
            s = stream or torch.cuda.current_stream(samples.device).cuda_stream
            p = ctypes.c_void_p(samples.data_ptr())
            _native.check(lib.neo_hip_upols_process_samples(self._h, p, n, p, n, n, 1, ctypes.c_void_p(s)))
            return samples
        if not (isinstance(samples, np.ndarray) and samples.dtype == np.float32 and samples.flags.c_contiguous):
            raise TypeError("samples must be a C-contiguous float32 array")
        n = samples.shape[-1] if samples.ndim else 0
        if samples.size != self.channels * n:
            raise ValueError("samples must be [channels][n]")
        _native.check(lib.neo_hip_upols_process_samples(self._h, _ptr(samples), n, _ptr(samples), n, n, 0, None))
        return samples

    def process_device(self, in_ptr: int, ld_in: int, out_ptr: int, ld_out: int, stream: int = 0) -> None:
        _native.check(_native.load().neo_hip_upols_process_device(self._h, ctypes.c_void_p(in_ptr), int(ld_in),
                                                                  ctypes.c_void_p(out_ptr), int(ld_out),
                                                                  ctypes.c_void_p(stream)))

    def process_blocks(self, signal, out=None, stream: int = 0):
        """Run consecutive blocks of a CUDA tensor [C][nblocks*B] (out may alias signal)."""
        import torch

        out = signal if out is None else out
        nb = signal.shape[-1] // self.block_size
        s = stream or torch.cuda.current_stream(signal.device).cuda_stream
        _native.check(_native.load().neo_hip_upols_process_blocks(self._h, ctypes.c_void_p(signal.data_ptr()),
                                                                  ctypes.c_void_p(out.data_ptr()), signal.shape[-1],
                                                                  nb, ctypes.c_void_p(s)))
        return out

    def process_blocks_ptr(self, in_ptr: int, out_ptr: int, ld: int, nblocks: int, stream: int = 0) -> None:
        """nblocks consecutive blocks through the C-ABI loop: channel c of block t at
        in_ptr + 4*(c*ld + t*B) (device pointers)."""
        _native.check(_native.load().neo_hip_upols_process_blocks(self._h, ctypes.c_void_p(in_ptr),
                                                                  ctypes.c_void_p(out_ptr), int(ld), int(nblocks),
                                                                  ctypes.c_void_p(stream)))

    def process_samples_ptr(self, in_ptr: int, ld_in: int, out_ptr: int, ld_out: int, n: int, is_device: bool,
                            stream: int = 0) -> None:
        """n samples per channel through neo_hip_upols_process_samples: channel c at
        in_ptr + 4*c*ld_in / out_ptr + 4*c*ld_out, host (synchronous) or device pointers."""
        _native.check(_native.load().neo_hip_upols_process_samples(self._h, ctypes.c_void_p(in_ptr), int(ld_in),
                                                                   ctypes.c_void_p(out_ptr), int(ld_out), int(n),
                                                                   int(bool(is_device)), ctypes.c_void_p(stream)))

    def set_batch(self, enable: bool) -> None:
        """process_blocks: T blocks per MAC pass (default) or one block per pass."""
        _native.check(_native.load().neo_hip_upols_set_batch(self._h, int(enable)))

    def batch_info(self):
        """(blocks per process_blocks pass, splits per channel of that pass)."""
        t, s = ctypes.c_int(), ctypes.c_int()
        _native.check(_native.load().neo_hip_upols_batch_info(self._h, ctypes.byref(t), ctypes.byref(s)))
        return t.value, s.value

    def set_offline(self, enable: bool) -> None:
        """Offline windows for batched calls of >= 128 blocks (neo_hip_upols_set_offline; on by
        default from 128 partitions): 128-block windows through partition-axis transforms."""
        _native.check(_native.load().neo_hip_upols_set_offline(self._h, int(bool(enable))))

    def offline_info(self):
        """(offline windows on, 128-partition segments they transform)"""
        e, n = ctypes.c_int(), ctypes.c_int()
        _native.check(_native.load().neo_hip_upols_get_offline(self._h, ctypes.byref(e), ctypes.byref(n)))
        return bool(e.value), n.value

    def set_ahead(self, enable: bool) -> None:
        """Streaming levels for single-block steps (neo_hip_upols_set_ahead)."""
        _native.check(_native.load().neo_hip_upols_set_ahead(self._h, int(bool(enable))))

    def ahead_info(self):
        """(streaming levels enabled, block position in the current far window, longest
        window, number of levels)."""
        v = [ctypes.c_int() for _ in range(4)]
        _native.check(_native.load().neo_hip_upols_get_ahead(self._h, *[ctypes.byref(x) for x in v]))
        return bool(v[0].value), v[1].value, v[2].value, v[3].value

    def far_group(self) -> int:
        """Windows per far phase-1 pass this handle runs (0: no far transform level)."""
        k = ctypes.c_int()
        _native.check(_native.load().neo_hip_upols_get_far_group(self._h, ctypes.byref(k)))
        return k.value

    def step_group(self) -> int:
        """Steps per background launch of the streaming levels' slices (1: one launch per step)."""
        k = ctypes.c_int()
        _native.check(_native.load().neo_hip_upols_get_step_group(self._h, ctypes.byref(k)))
        return k.value

    def windows(self) -> int:
        """The level windows the handle runs: 1 aligned, 2 staggered (neo_hip_upols_get_windows)."""
        k = ctypes.c_int()
        _native.check(_native.load().neo_hip_upols_get_windows(self._h, ctypes.byref(k)))
        return k.value

    def far_form(self) -> int:
        """The p >= 256 band's form: 0 none, 1 transform with stored spectra, 2 transform recomputed
        every window, 3 the 128-block Toeplitz level (neo_hip_upols_get_far_form)."""
        k = ctypes.c_int()
        _native.check(_native.load().neo_hip_upols_get_far_form(self._h, ctypes.byref(k)))
        return k.value

    def join_background(self, stream=None) -> None:
        """Make `stream` (a raw hipStream_t, None = the null stream) wait for the background
        slice launches of the step groups issued so far (device-side; no host wait)."""
        _native.check(_native.load().neo_hip_upols_join_background(self._h, ctypes.c_void_p(stream)))

    def background_stream(self) -> int:
        """The step groups' background stream as a raw hipStream_t, 0 while there is none (before
        the first grouped step, one launch per step, latency mode). A setup call may destroy it:
        fetch it again after one (neo_hip_upols_get_background_stream)."""
        s = ctypes.c_void_p()
        _native.check(_native.load().neo_hip_upols_get_background_stream(self._h, ctypes.byref(s)))
        return s.value or 0

    def set_paced(self, enable) -> None:
        """Step groups: issue the group's background launch in pieces, each block after the
        piece before it (neo_hip_upols_set_paced): an even host round trip per block. True / 1:
        a piece per call; 2: two pieces per group; False / 0: off."""
        _native.check(_native.load().neo_hip_upols_set_paced(self._h, int(enable)))

    def set_persistent(self, enable: bool, idle_ms: float = 50.0) -> None:
        """Latency mode (neo_hip_upols_set_persistent): one persistent kernel steps every block;
        every process call is then synchronous (complete on return, the stream is not used).
        With the streaming levels it runs their block and slice roles (blocks up to 512); without
        them (fewer than 64 partitions) the plain fused step, blocks up to 4096. Raises for shapes
        it does not take (more than 16 channels, sub-block v2, B > 512 with the levels)."""
        _native.check(_native.load().neo_hip_upols_set_persistent(self._h, int(bool(enable)), float(idle_ms)))

    def persistent_info(self) -> dict:
        e, r, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols_get_persistent(self._h, ctypes.byref(e), ctypes.byref(r),
                                                                   ctypes.byref(n)))
        return {"enabled": bool(e.value), "running": bool(r.value), "launches": n.value}

    def persist_step_times(self, cap: int = 63):
        """GPU time (us) of the last latency-mode steps, oldest first: record read -> done signal."""
        buf, n = (ctypes.c_double * cap)(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols_persist_step_times(self._h, buf, cap, ctypes.byref(n)))
        return list(buf[: n.value])

    # -- instrumentation ------------------------------------------------------
    def set_timing(self, enable, every: int = 1) -> None:
        """HIP events around every `every`-th MAC launch while enabled (bench instrumentation)."""
        if every < 1:
            raise ValueError("every must be >= 1")
        _native.check(_native.load().neo_hip_upols_set_timing(self._h, int(every) if enable else 0))

    def timing(self):
        """(accumulated ms, timed launch groups) since the last call: the MAC kernel of
        plain / batched steps, the whole step of streaming-level steps."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols_timing(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def timing_detail(self):
        """Per part [(ms, count)] * 4 since the last call (neo_hip_upols_timing_detail):
        streaming-level steps 0 = the step kernel (k_lvl_step: block and level slices);
        plain / batched steps 0 = MAC kernel."""
        ms, n = (ctypes.c_double * 4)(), (ctypes.c_int64 * 4)()
        _native.check(_native.load().neo_hip_upols_timing_detail(self._h, ms, n))
        return [(ms[k], n[k]) for k in range(4)]

    def step_times(self, cap: int = 1 << 16):
        """Duration (ms) of every timed launch group since the last drain, in order (a
        streaming step: first to last event of the step)."""
        buf, n = (ctypes.c_double * cap)(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols_step_times(self._h, buf, cap, ctypes.byref(n)))
        return list(buf[: min(n.value, cap)])

    @property
    def splits(self) -> int:
        s = ctypes.c_int()
        _native.check(_native.load().neo_hip_upols_info(self._h, None, None, None, ctypes.byref(s)))
        return s.value

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _native.load().neo_hip_upols_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UpolsConvolver64:
    """C independent double-precision UPOLS / UPOLA convolvers stepped together (neo_hip_upols64:
    upols_convolver<complex<double>> / upola_convolver<complex<double>>), one launch pair per block.

    State lives in HBM in complex128 / float64: filter [C][P][B] and FDL [C][P][B] (packed bins),
    previous block or overlap tail [C][B]. Whole blocks, in place, zero latency. `split_workgroups`
    (0: automatic) is the number of workgroups the MAC launch aims for. set_batch() turns batched
    passes on for calls of many blocks (offline work): T blocks per read of the filter and the delay
    line. No streaming levels, live updates, latency mode or groups: the float32 UpolsConvolver has
    those."""

    def __init__(self, channels: int, block_size: int, partitions: int, device: int = 0, method: str = "upols",
                 split_workgroups: int = 0):
        methods = {"upols": 0, "upola": 1}
        if method not in methods:
            raise ValueError(f"method must be 'upols' or 'upola', got {method!r}")
        h = ctypes.c_void_p()
        _native.check(_native.load().neo_hip_upols64_create(int(channels), int(block_size), int(partitions), int(device),
                                                            methods[method], int(split_workgroups), ctypes.byref(h)))
        self._h = h
        self.channels, self.block_size, self.partitions, self.device = channels, block_size, partitions, device
        self.method = method

    def filter(self, partitions) -> None:
        """[C][P][B+1] complex128 (host array or CUDA tensor); resets FDL, window and write position."""
        shape = (self.channels, self.partitions, self.block_size + 1)
        if _is_torch(partitions):
            import torch

            t = partitions
            if t.dtype != torch.complex128 or not t.is_contiguous() or not t.is_cuda or t.numel() != int(np.prod(shape)):
                raise ValueError(f"filter must be a contiguous complex128 CUDA tensor of {shape}")
            _producer_join(t)
            _native.check(_native.load().neo_hip_upols64_set_filter(self._h, ctypes.c_void_p(t.data_ptr()), 1))
            return
        H = np.ascontiguousarray(partitions, dtype=np.complex128)
        if H.ndim == 2:
            H = H[None]
        if H.shape != shape:
            raise ValueError(f"filter shape {H.shape} != {shape}")
        _native.check(_native.load().neo_hip_upols64_set_filter(self._h, _ptr(H), 0))

    def set_impulse(self, impulse_response, normalize: bool = True) -> None:
        """normalize_impulse (optional) + uniform_partition in double straight into the device filter;
        [C][L] float64 (host array or CUDA tensor, left as it is)."""
        if _is_torch(impulse_response):
            import torch

            t = impulse_response
            if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda or t.numel() != self.channels * t.shape[-1]:
                raise ValueError("impulse must be a contiguous float64 CUDA tensor of one row per channel")
            _producer_join(t)
            _native.check(_native.load().neo_hip_upols64_set_impulse(self._h, ctypes.c_void_p(t.data_ptr()), t.shape[-1],
                                                                     int(normalize), 1))
            return
        ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float64)))
        if ir.shape[0] != self.channels:
            raise ValueError("impulse channel count mismatch")
        _native.check(_native.load().neo_hip_upols64_set_impulse(self._h, _ptr(ir), ir.shape[1], int(normalize), 0))

    def reset(self) -> None:
        _native.check(_native.load().neo_hip_upols64_reset(self._h))

    def process(self, samples, stream: int = 0):
        """Whole blocks per channel, in place: [C][k * block_size] float64 ndarray or CUDA tensor (a
        tensor: asynchronous on torch's current stream, or `stream`)."""
        lib = _native.load()
        if _is_torch(samples):
            import torch

            if samples.dtype != torch.float64 or not samples.is_contiguous() or not samples.is_cuda:
                raise TypeError("samples must be a contiguous float64 CUDA tensor")
            n = samples.shape[-1]
            if samples.numel() != self.channels * n:
                raise ValueError("samples must be [channels][n]")
            s = stream or torch.cuda.current_stream(samples.device).cuda_stream
            p = ctypes.c_void_p(samples.data_ptr())
            _native.check(lib.neo_hip_upols64_process_samples(self._h, p, n, p, n, n, 1, ctypes.c_void_p(s)))
            return samples
        if not (isinstance(samples, np.ndarray) and samples.dtype == np.float64 and samples.flags.c_contiguous):
            raise TypeError("samples must be a C-contiguous float64 array")
        n = samples.shape[-1] if samples.ndim else 0
        if samples.size != self.channels * n:
            raise ValueError("samples must be [channels][n]")
        _native.check(lib.neo_hip_upols64_process_samples(self._h, _ptr(samples), n, _ptr(samples), n, n, 0, None))
        return samples

    __call__ = process

    def process_device(self, in_ptr: int, ld_in: int, out_ptr: int, ld_out: int, n: int | None = None,
                       stream: int = 0, is_device: bool = True) -> None:
        """n samples (default: one block) of every channel, channel c at in_ptr + 8 c ld_in bytes and
        out_ptr + 8 c ld_out (strides in doubles, even, >= n; in_ptr == out_ptr allowed)."""
        n = self.block_size if n is None else n
        _native.check(_native.load().neo_hip_upols64_process_samples(self._h, ctypes.c_void_p(in_ptr), int(ld_in),
                                                                     ctypes.c_void_p(out_ptr), int(ld_out), int(n),
                                                                     int(bool(is_device)), ctypes.c_void_p(stream or None)))

    def info(self) -> dict:
        """splits per channel, partitions per split (rows; the last split may be shorter), device bytes."""
        s, r, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols64_info(self._h, ctypes.byref(s), ctypes.byref(r), ctypes.byref(b)))
        return {"splits": s.value, "rows": r.value, "state_bytes": b.value}

    def set_batch(self, enable=True) -> None:
        """Batched passes on or off (neo_hip_upols64_set_batch): a call of q T + r blocks then runs q
        passes of T blocks and r plain steps. True: the plan's T; 8 or 16: that T. Filter and state
        stay as they are, so it may come between any two process calls."""
        _native.check(_native.load().neo_hip_upols64_set_batch(self._h, int(enable)))

    def batch_info(self) -> dict:
        """blocks per pass (1 while batching is off), splits per channel of the pass's MAC, and the
        device bytes batching holds on top of info()['state_bytes']."""
        t, s, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols64_batch_info(self._h, ctypes.byref(t), ctypes.byref(s), ctypes.byref(b)))
        return {"blocks_per_pass": t.value, "splits": s.value, "extra_bytes": b.value}

    def set_offline(self, enable=True) -> None:
        """Offline windows on or off (neo_hip_upols64_set_offline): a call then runs a window pass of
        128 blocks (256-point transforms along the block axis) for every 128 blocks left, then batched
        passes if set_batch is on, then plain steps. Filter and state stay as they are, so it may come
        between any two process calls. It holds the segment spectra (about twice the filter) and
        offline_info()['extra_bytes'] more until it is turned off or the convolver is closed."""
        _native.check(_native.load().neo_hip_upols64_set_offline(self._h, int(enable)))

    def offline_info(self) -> dict:
        """blocks per window pass (128; 0 while off), segments = ceil(P / 128), the bytes of the segment
        spectra and of the scratch, the windows' spectra and the tails (0 while off)."""
        t, g, sb, eb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols64_offline_info(self._h, ctypes.byref(t), ctypes.byref(g), ctypes.byref(sb),
                                                                  ctypes.byref(eb)))
        return {"blocks_per_pass": t.value, "segments": g.value, "spectra_bytes": sb.value, "extra_bytes": eb.value}

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.check(_native.load().neo_hip_upols64_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upols64_plan(channels: int, block_size: int, partitions: int, split_workgroups: int = 0) -> dict:
    """UpolsConvolver64.info() for a shape, without a device (neo_hip_upols64_plan)."""
    s, r, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    _native.check(_native.load().neo_hip_upols64_plan(int(channels), int(block_size), int(partitions),
                                                      int(split_workgroups), ctypes.byref(s), ctypes.byref(r),
                                                      ctypes.byref(b)))
    return {"splits": s.value, "rows": r.value, "state_bytes": b.value}


def upols64_batch_plan(channels: int, block_size: int, partitions: int, method: str = "upols", split_workgroups: int = 0,
                       blocks: int = 0) -> dict:
    """The batched passes of a UpolsConvolver64 of this shape, without a device
    (neo_hip_upols64_batch_plan): what batch_info() reports once set_batch(blocks or True) is on, the
    partitions per split and the algorithmic bytes of one pass."""
    methods = {"upols": 0, "upola": 1}
    if method not in methods:
        raise ValueError(f"method must be 'upols' or 'upola', got {method!r}")
    t, s, r, e, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    _native.check(_native.load().neo_hip_upols64_batch_plan(int(channels), int(block_size), int(partitions), methods[method],
                                                            int(split_workgroups), int(blocks), ctypes.byref(t),
                                                            ctypes.byref(s), ctypes.byref(r), ctypes.byref(e), ctypes.byref(b)))
    return {"blocks_per_pass": t.value, "splits": s.value, "rows": r.value, "extra_bytes": e.value, "pass_bytes": b.value}


def upols64_offline_plan(channels: int, block_size: int, partitions: int, method: str = "upols") -> dict:
    """The offline windows of a UpolsConvolver64 of this shape, without a device
    (neo_hip_upols64_offline_plan): what offline_info() reports once set_offline() is on, and the
    algorithmic bytes of one window pass."""
    methods = {"upols": 0, "upola": 1}
    if method not in methods:
        raise ValueError(f"method must be 'upols' or 'upola', got {method!r}")
    t, g, sb, eb, pb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _native.check(_native.load().neo_hip_upols64_offline_plan(int(channels), int(block_size), int(partitions), methods[method],
                                                              ctypes.byref(t), ctypes.byref(g), ctypes.byref(sb),
                                                              ctypes.byref(eb), ctypes.byref(pb)))
    return {"blocks_per_pass": t.value, "segments": g.value, "spectra_bytes": sb.value, "extra_bytes": eb.value,
            "pass_bytes": pb.value}


class UpolsMultiConvolver:
    """C channels sharded over several devices of one node (neo_hip_upols_multi_*): shard i
    = channels [C i / n, C (i + 1) / n) on devices[i] (a device may repeat), one handle and
    stream each, no collective (the reference steps all channels in one loop,
    DenseConvolution.hpp:35,50-67). Host I/O; every call runs the shards concurrently and
    returns when all are done. Results equal one UpolsConvolver over all channels bit for
    bit."""

    def __init__(self, channels: int, block_size: int, partitions: int, devices, method: str = "upols",
                 options: dict | None = None):
        lib = _native.load()
        methods = {"upols": 0, "upola": 1, "upola_v2": 2}
        if method not in methods:
            raise ValueError(f"method must be 'upols', 'upola' or 'upola_v2', got {method!r}")
        opts = dict(UpolsConvolver.OPTION_DEFAULTS)
        for k, v in (options or {}).items():
            if k not in opts:
                raise ValueError(f"unknown convolver option {k!r}")
            opts[k] = int(v)
        o = _native.UpolsOpts(**opts)
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        h = ctypes.c_void_p()
        _native.check(lib.neo_hip_upols_multi_create(int(channels), int(block_size), int(partitions), devs,
                                                     len(devices), methods[method], ctypes.byref(o), ctypes.byref(h)))
        self._h = h
        self.channels, self.block_size, self.partitions = channels, block_size, partitions
        self.devices = list(devices)

    def shards(self):
        """[(device, first_channel, channels)] per shard"""
        lib = _native.load()
        n = ctypes.c_int()
        _native.check(lib.neo_hip_upols_multi_shards(self._h, ctypes.byref(n)))
        out = []
        for i in range(n.value):
            d, c0, nc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            _native.check(lib.neo_hip_upols_multi_shard(self._h, i, None, ctypes.byref(d), ctypes.byref(c0),
                                                        ctypes.byref(nc)))
            out.append((d.value, c0.value, nc.value))
        return out

    def filter(self, partitions) -> None:
        H = np.ascontiguousarray(partitions, dtype=np.complex64)
        if H.shape != (self.channels, self.partitions, self.block_size + 1):
            raise ValueError(f"filter shape {H.shape} != {(self.channels, self.partitions, self.block_size + 1)}")
        _native.check(_native.load().neo_hip_upols_multi_set_filter(self._h, _ptr(H)))

    def set_impulse(self, impulse_response, normalize: bool = True) -> None:
        ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float32)))
        if ir.shape[0] != self.channels:
            raise ValueError("impulse channel count mismatch")
        _native.check(_native.load().neo_hip_upols_multi_set_impulse(self._h, _ptr(ir), ir.shape[1], int(normalize)))

    def update_filter(self, partitions, fade_blocks: int = 1, curve: str = "linear", stream: int = 0) -> None:
        """UpolsConvolver.update_filter on every shard (neo_hip_upols_multi_update_filter): host
        partitions [C][P][B+1], complete on return (`stream` must stay 0: every shard has its own)."""
        if stream:
            raise ValueError("a multi-device convolver runs every shard on its own stream")
        H = np.ascontiguousarray(partitions, dtype=np.complex64)
        if H.shape != (self.channels, self.partitions, self.block_size + 1):
            raise ValueError(f"filter shape {H.shape} != {(self.channels, self.partitions, self.block_size + 1)}")
        _native.check(_native.load().neo_hip_upols_multi_update_filter(self._h, _ptr(H), int(fade_blocks),
                                                                       _fade_curve(curve)))

    def update_impulse(self, impulse_response, normalize: bool = True, fade_blocks: int = 1, curve: str = "linear",
                       stream: int = 0) -> None:
        """UpolsConvolver.update_impulse on every shard; the normalisation factor is taken once over
        all channels, as set_impulse takes it."""
        if stream:
            raise ValueError("a multi-device convolver runs every shard on its own stream")
        ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float32)))
        if ir.shape[0] != self.channels:
            raise ValueError("impulse channel count mismatch")
        _native.check(_native.load().neo_hip_upols_multi_update_impulse(self._h, _ptr(ir), ir.shape[1], int(normalize),
                                                                        int(fade_blocks), _fade_curve(curve)))

    def fade_info(self) -> dict:
        """The shards' fades run in step: remaining_blocks and fade_blocks of shard 0, bank_bytes
        summed over the shards."""
        lib = _native.load()
        out = {"remaining_blocks": 0, "fade_blocks": 0, "bank_bytes": 0}
        for i in range(len(self.shards())):
            h = ctypes.c_void_p()
            _native.check(lib.neo_hip_upols_multi_shard(self._h, i, ctypes.byref(h), None, None, None))
            r, f, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
            _native.check(lib.neo_hip_upols_fade_info(h, ctypes.byref(r), ctypes.byref(f), ctypes.byref(n)))
            if i == 0:
                out["remaining_blocks"], out["fade_blocks"] = r.value, f.value
            out["bank_bytes"] += n.value
        return out

    def process(self, samples) -> np.ndarray:
        """[C][n] float32 host samples (n a multiple of the block except for upola_v2) ->
        [C][n] output; the shards run concurrently."""
        x = np.ascontiguousarray(samples, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] != self.channels:
            raise ValueError(f"samples must be [{self.channels}][n]")
        y = np.empty_like(x)
        n = x.shape[1]
        _native.check(_native.load().neo_hip_upols_multi_process_samples(self._h, _ptr(x), n, _ptr(y), n, n))
        return y

    def process_samples_ptr(self, in_ptr: int, ld_in: int, out_ptr: int, ld_out: int, n: int) -> None:
        """n samples per channel through neo_hip_upols_multi_process_samples: channel c at
        in_ptr + 4*c*ld_in / out_ptr + 4*c*ld_out, host pointers (synchronous)."""
        _native.check(_native.load().neo_hip_upols_multi_process_samples(self._h, ctypes.c_void_p(in_ptr), int(ld_in),
                                                                         ctypes.c_void_p(out_ptr), int(ld_out), int(n)))

    def reset(self) -> None:
        _native.check(_native.load().neo_hip_upols_multi_reset(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _native.load().neo_hip_upols_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OverlapStage:
    """C independent overlap stages on the GPU (neo_hip_overlap_*): overlap_save
    (overlap_save.hpp:19-112) or overlap_add (overlap_add.hpp:23-107) of block B for F-tap
    filters, transform size 2^next_order(B + F - 1). forward(block) updates the window and
    returns the n/2 + 1 bins the reference's callback sees; inverse(spectrum, out) runs the
    irfft, 1/n and writes the output block. Host arrays (synchronous) or CUDA tensors."""

    KINDS = {"save": 0, "add": 1}

    def __init__(self, kind: str, channels: int, block_size: int, filter_size: int, device: int = 0):
        if kind not in self.KINDS:
            raise ValueError(f"kind must be 'save' or 'add', got {kind!r}")
        h = ctypes.c_void_p()
        _native.check(_native.load().neo_hip_overlap_create(self.KINDS[kind], int(channels), int(block_size),
                                                            int(filter_size), int(device), ctypes.byref(h)))
        self._h = h
        self.kind, self.channels, self.device = kind, channels, device
        b, f, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_overlap_info(h, ctypes.byref(b), ctypes.byref(f), ctypes.byref(n)))
        self._block, self._filter, self._n = b.value, f.value, n.value

    def block_size(self) -> int:
        return self._block

    def filter_size(self) -> int:
        return self._filter

    def transform_size(self) -> int:
        return self._n

    def forward(self, block, spectrum=None, stream: int = 0):
        """block [C][B] float32 -> spectrum [C][n/2 + 1] complex64 (new array / tensor if None)."""
        lib = _native.load()
        bins = self._n // 2 + 1
        if _is_torch(block) and block.is_cuda:
            import torch

            spec = spectrum if spectrum is not None else torch.empty((self.channels, bins), dtype=torch.complex64,
                                                                     device=block.device)
            s = stream or torch.cuda.current_stream(block.device).cuda_stream
            ld = block.stride(0) if block.dim() == 2 else block.shape[-1]  # channel c at c * ld
            _native.check(lib.neo_hip_overlap_forward(self._h, ctypes.c_void_p(block.data_ptr()), ld,
                                                      ctypes.c_void_p(spec.data_ptr()), 1, ctypes.c_void_p(s)))
            return spec
        x = np.ascontiguousarray(np.asarray(block, dtype=np.float32).reshape(self.channels, -1))
        if x.shape[1] != self._block:
            raise ValueError(f"block must be [{self.channels}][{self._block}]")
        spec = np.empty((self.channels, bins), np.complex64) if spectrum is None else spectrum
        _native.check(lib.neo_hip_overlap_forward(self._h, _ptr(x), x.shape[1], _ptr(spec), 0, None))
        return spec

    def inverse(self, spectrum, out, stream: int = 0):
        """spectrum [C][n/2 + 1] complex64 -> out [C][B] float32 (in place)."""
        lib = _native.load()
        if _is_torch(out) and out.is_cuda:
            import torch

            s = stream or torch.cuda.current_stream(out.device).cuda_stream
            ld = out.stride(0) if out.dim() == 2 else out.shape[-1]
            _native.check(lib.neo_hip_overlap_inverse(self._h, ctypes.c_void_p(spectrum.data_ptr()),
                                                      ctypes.c_void_p(out.data_ptr()), ld, 1, ctypes.c_void_p(s)))
            return out
        spec = np.ascontiguousarray(spectrum, dtype=np.complex64)
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous):
            raise TypeError("out must be a C-contiguous float32 array")
        _native.check(lib.neo_hip_overlap_inverse(self._h, _ptr(spec), _ptr(out), out.shape[-1], 0, None))
        return out

    def reset(self) -> None:
        _native.check(_native.load().neo_hip_overlap_reset(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _native.load().neo_hip_overlap_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class overlap_save:
    """Drop-in for neo::convolution::overlap_save<complex<float>> (overlap_save.hpp:19-112):
    overlap_save(block_size, filter_size); __call__(block, callback) processes one block of a
    1-D float32 array in place, callback(bins) sees (and may modify in place) the
    transform_size() / 2 + 1 bins."""

    _kind = "save"

    def __init__(self, block_size: int, filter_size: int, device: int = 0):
        self._stage = OverlapStage(self._kind, 1, block_size, filter_size, device)

    def block_size(self) -> int:
        return self._stage.block_size()

    def filter_size(self) -> int:
        return self._stage.filter_size()

    def transform_size(self) -> int:
        return self._stage.transform_size()

    def __call__(self, block, callback):
        if not (isinstance(block, np.ndarray) and block.dtype == np.float32 and block.flags.c_contiguous):
            raise TypeError("block must be a C-contiguous float32 array")
        if block.size != self.block_size():
            raise ValueError(f"block must hold {self.block_size()} samples")
        spec = self._stage.forward(block.reshape(1, -1))
        callback(spec[0])
        self._stage.inverse(spec, block.reshape(1, -1))
        return block


class overlap_add(overlap_save):
    """Drop-in for neo::convolution::overlap_add<complex<float>> (overlap_add.hpp:23-107)."""

    _kind = "add"


class UpolsGroup:
    """Single-channel convolvers of one shape stepped together (neo_hip_upols_group_*): members
    join(), take a filter [P][B+1] each and process one host block [B] per call, in place; while
    the calls follow the plugin's frame pattern (DenseConvolution.cpp:62-74: every member once
    per frame, each on a buffer of its own) and every member's buffer is registered with the
    group (register(): the owner keeps it allocated until unregister()), a frame is ONE launch,
    else each member runs on a handle of its own; outputs are each member's own sequential
    convolver's either way (up to float summation order after a mode switch)."""

    def __init__(self, block_size: int, partitions: int, method: str = "upols", device: int = 0):
        methods = {"upols": 0, "upola": 1}
        if method not in methods:
            raise ValueError("groups take method 'upols' or 'upola'")
        h = ctypes.c_void_p()
        _native.check(_native.load().neo_hip_upols_group_create(int(block_size), int(partitions), methods[method],
                                                                int(device), ctypes.byref(h)))
        self._h = h
        self.block_size, self.partitions = block_size, partitions

    def join(self) -> int:
        i = ctypes.c_int()
        _native.check(_native.load().neo_hip_upols_group_join(self._h, ctypes.byref(i)))
        return i.value

    def leave(self, member: int) -> None:
        _native.check(_native.load().neo_hip_upols_group_leave(self._h, int(member)))

    def filter(self, member: int, partitions) -> None:
        H = np.ascontiguousarray(partitions, dtype=np.complex64)
        if H.shape != (self.partitions, self.block_size + 1):
            raise ValueError(f"filter shape {H.shape} != {(self.partitions, self.block_size + 1)}")
        _native.check(_native.load().neo_hip_upols_group_set_filter(self._h, int(member), _ptr(H), 0))

    def __call__(self, member: int, block: np.ndarray) -> np.ndarray:
        if not (isinstance(block, np.ndarray) and block.dtype == np.float32 and block.flags.c_contiguous
                and block.size == self.block_size):
            raise TypeError("block must be a C-contiguous float32 array of block_size samples")
        _native.check(_native.load().neo_hip_upols_group_process(self._h, int(member), _ptr(block)))
        return block

    def reset(self, member: int) -> None:
        _native.check(_native.load().neo_hip_upols_group_reset(self._h, int(member)))

    def register(self, buffer: np.ndarray, frame_stable: bool = False, in_place: bool = False) -> None:
        """the group may read `buffer` (host memory the caller keeps alive until unregister).
        frame_stable: the caller also promises that during a frame nothing but the members' own
        calls writes it (neo_hip_upols_group_register_ex, NEO_HIP_GROUP_FRAME_STABLE): members then
        commit without comparing their blocks with a snapshot. in_place (NEO_HIP_GROUP_FRAME_INPLACE,
        implies frame_stable): it also reads each member's block only through that member's call,
        each member on the same block every frame: the frame's first call writes every output in place.
        Under the in-place promise a frame's blocks are consumed at its first call, and a state change
        in mid-frame takes effect after them: after filter(), reset(), join(), leave() or a member's
        second call in a one-launch frame, a member that has not made its call of the frame yet finds
        its output in its block (that call returns at once), and its new filter or zero state starts
        with its next frame; called on another buffer instead it is stepped on that as a new block (the
        promise is broken). Plain and frame_stable ranges keep their inputs: a change applies where it
        is made."""
        if not isinstance(buffer, np.ndarray) or not buffer.flags.c_contiguous:
            raise TypeError("register takes a C-contiguous numpy array")
        self._keep = getattr(self, "_keep", {})
        self._keep[buffer.ctypes.data] = buffer  # keeps the registered array alive on the Python side too
        _native.check(_native.load().neo_hip_upols_group_register_ex(self._h, ctypes.c_void_p(buffer.ctypes.data),
                                                                     int(buffer.nbytes),
                                                                     3 if in_place else (1 if frame_stable else 0)))

    def unregister(self, buffer=None) -> None:
        """stop reading `buffer` (None: every registered range)"""
        ptr = None if buffer is None else buffer.ctypes.data
        _native.check(_native.load().neo_hip_upols_group_unregister(self._h, ctypes.c_void_p(ptr)))
        keep = getattr(self, "_keep", {})
        if ptr is None:
            keep.clear()
        else:
            keep.pop(ptr, None)

    def stats(self) -> dict:
        c = ctypes.c_int()
        v = [ctypes.c_int64() for _ in range(4)]
        _native.check(_native.load().neo_hip_upols_group_stats(self._h, ctypes.byref(c), *[ctypes.byref(x) for x in v]))
        return {"coalesced": bool(c.value), "frame_steps": v[0].value, "calls": v[1].value, "redos": v[2].value,
                "switches": v[3].value}

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _native.load().neo_hip_upols_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class upols_convolver:
    """Single-channel drop-in for upols_convolver<complex<float>>: default-constructible,
    filter([P][B+1]) then __call__(block[B]) in place."""

    _method = "upols"

    def __init__(self, device: int = 0, *, dtype=np.float32):
        """dtype=np.float64: upols_convolver<complex<double>> (complex128 filter, float64 blocks)."""
        self._impl = None
        self._device = device
        self._f64 = _f64(dtype)
        if self._f64 and self._method == "upola_v2":
            raise TypeError("upola_convolver_v2 is float32 only")

    def filter(self, filt) -> None:
        H = np.ascontiguousarray(filt, dtype=np.complex128 if self._f64 else np.complex64)
        if H.ndim != 2:
            raise ValueError("filter must be [P][B+1]")
        P, bins = H.shape
        impl = self._impl
        if impl is None or (impl.partitions, impl.block_size) != (P, bins - 1):
            make = UpolsConvolver64 if self._f64 else UpolsConvolver
            impl = make(1, bins - 1, P, self._device, method=self._method)
        impl.filter(H[None])
        self._impl = impl

    def __call__(self, block):
        if self._impl is None:
            raise RuntimeError("filter() must be called first")
        if self._f64:
            if _is_torch(block):
                self._impl.process(block.view(1, -1))
                return block
            if not (isinstance(block, np.ndarray) and block.dtype == np.float64 and block.flags.c_contiguous):
                raise TypeError("block must be a C-contiguous float64 array")
            if block.size != self._impl.block_size:
                raise ValueError("block must hold block_size samples")
            self._impl.process(block.reshape(1, -1))  # a view: processed in place
            return block
        return self._impl(block)


split_upols_convolver = upols_convolver


class upola_convolver(upols_convolver):
    """Single-channel drop-in for upola_convolver<complex<float>> (overlap-add stage)."""

    _method = "upola"


split_upola_convolver = upola_convolver


class upola_convolver_v2(upols_convolver):
    """Single-channel drop-in for upola_convolver_v2<complex<float>> (overlap_add_convolver.hpp:
    20-136): __call__ takes any number of samples, in place."""

    _method = "upola_v2"

    def __call__(self, samples):
        if self._impl is None:
            raise RuntimeError("filter() must be called first")
        if _is_torch(samples):
            return self._impl.process(samples.view(1, -1))
        if not (isinstance(samples, np.ndarray) and samples.dtype == np.float32 and samples.flags.c_contiguous):
            raise TypeError("samples must be a C-contiguous float32 array")
        self._impl.process(samples.reshape(1, -1))  # a view: processed in place
        return samples


def dense_convolve(signal, impulse_response, block_size: int, device: int = 0, method: str = "upols",
                   options: dict | None = None, *, dtype=np.float32, batch: bool = False,
                   offline: bool = False) -> np.ndarray:
    """dense_convolve<upols_convolver | upola_convolver> (DenseConvolution.hpp:39-70): normalize
    the IR matrix, partition it, run every block (tail zero-padded), output truncated to N.
    `options`: UpolsConvolver code-path choices (same results). dtype=np.float64: the whole chain in
    double (UpolsConvolver64; of `options` it reads split_workgroups alone), float64 out; with
    batch=True in batched passes (UpolsConvolver64.set_batch), with offline=True in offline windows of
    128 blocks (UpolsConvolver64.set_offline; what is left of a chunk goes by batch), the default is
    the loop of steps. `batch` and `offline` belong to float64 alone."""
    if (batch or offline) and not _f64(dtype):
        raise ValueError("batch=True / offline=True take dtype=np.float64 (the float32 path chooses its passes by `options`)")
    if _f64(dtype):
        sig = np.ascontiguousarray(np.atleast_2d(np.asarray(signal, dtype=np.float64)))
        ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float64)))
        C, N = sig.shape
        if ir.shape[0] != C:
            raise ValueError("signal and impulse response channel counts differ")
        for k in options or {}:
            if k not in UpolsConvolver.OPTION_DEFAULTS:
                raise ValueError(f"unknown convolver option {k!r}")
        conv = UpolsConvolver64(C, block_size, num_partitions(ir.shape[1], block_size), device, method=method,
                                split_workgroups=int((options or {}).get("split_workgroups", 0)))
        conv.set_impulse(ir, normalize=True)
        if batch:
            conv.set_batch(True)
        if offline:
            conv.set_offline(True)
        nb = -(-N // block_size)
        chunk = max(1, (1 << 25) // (C * block_size))  # <= 2^25 doubles per upload
        if offline:
            chunk = max(128, chunk // 128 * 128)  # whole windows
        out = np.empty_like(sig)
        for t0 in range(0, nb, chunk):
            t1 = min(nb, t0 + chunk)
            lo, hi = t0 * block_size, min(N, t1 * block_size)
            buf = np.zeros((C, (t1 - t0) * block_size), dtype=np.float64)
            buf[:, : hi - lo] = sig[:, lo:hi]
            conv.process(buf)
            out[:, lo:hi] = buf[:, : hi - lo]
        conv.close()
        return out
    sig = np.ascontiguousarray(np.atleast_2d(np.asarray(signal, dtype=np.float32)))
    ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float32)))
    C, N = sig.shape
    if ir.shape[0] != C:
        raise ValueError("signal and impulse response channel counts differ")
    P = num_partitions(ir.shape[1], block_size)
    conv = UpolsConvolver(C, block_size, P, device, method=method, options=options)
    conv.set_impulse(ir, normalize=True)
    nb = -(-N // block_size)
    # whole signal in chunks of <= 2^26 samples: one upload, batched passes (T blocks per
    # pass over filter + FDL), one download per chunk; the tail block is zero-padded
    chunk = max(1, (1 << 26) // (C * block_size))
    chunk = max(256, chunk // 256 * 256)  # whole offline passes (256 blocks: two windows of 128)
    out = np.empty_like(sig)
    for t0 in range(0, nb, chunk):
        t1 = min(nb, t0 + chunk)
        lo, hi = t0 * block_size, min(N, t1 * block_size)
        buf = np.zeros((C, (t1 - t0) * block_size), dtype=np.float32)
        buf[:, : hi - lo] = sig[:, lo:hi]
        conv.process(buf)
        out[:, lo:hi] = buf[:, : hi - lo]
    conv.close()
    return out


def sparse_plan(mask, block_size: int) -> dict:
    """The tile-compacted format of a sparse filter for `mask` ([C][P][B+1] or [P][B+1], true =
    keep), on the host (neo_hip_upols_sparse_plan; no device needed): per row a bitmap of kept
    128-byte tiles (16 packed bins; columns 0 and B both in tile 0) `tile_mask` [C][P][NW] uint32
    and `row_off` [C][P+1], the exclusive prefix sum of the rows' kept tiles within a channel;
    `kept_bins`, `kept_tiles` over all channels."""
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[2] != block_size + 1:
        raise ValueError(f"mask must be [C][P][{block_size + 1}], got {m.shape}")
    C, P, _ = m.shape
    nw = max(1, block_size // 512)
    tm = np.zeros((C, P, nw), dtype=np.uint32)
    ro = np.zeros((C, P + 1), dtype=np.uint32)
    kb, kt = ctypes.c_int64(), ctypes.c_int64()
    _native.check(_native.load().neo_hip_upols_sparse_plan(_ptr(m), C, int(block_size), P, _ptr(tm), _ptr(ro),
                                                           ctypes.byref(kb), ctypes.byref(kt)))
    return {"tile_mask": tm, "row_off": ro, "kept_bins": kb.value, "kept_tiles": kt.value}


def sparse_window_plan(tile_mask, block_size: int, window: int) -> dict:
    """The window bitmaps of a batched sparse pass of `window` blocks (a power of two, 2..32), on
    the host (neo_hip_upols_sparse_window_plan; no device needed): `tile_mask` [C][P][NW] uint32
    (sparse_plan's) -> `win_mask` [C][P][NW], row p the OR of tile_mask rows [p, min(P, p + window)):
    the FDL tiles the row entering the pass at partition p is needed for; `window_tiles`, the sum
    of its popcounts."""
    nw = max(1, int(block_size) // 512)
    tm = np.ascontiguousarray(tile_mask, dtype=np.uint32)
    if tm.ndim == 2:
        tm = tm[None]
    if tm.ndim != 3 or tm.shape[2] != nw:
        raise ValueError(f"tile_mask must be [C][P][{nw}], got {tm.shape}")
    C, P, _ = tm.shape
    wm = np.zeros_like(tm)
    wt = ctypes.c_int64()
    _native.check(_native.load().neo_hip_upols_sparse_window_plan(_ptr(tm), C, int(block_size), P, int(window),
                                                                  _ptr(wm), ctypes.byref(wt)))
    return {"win_mask": wm, "window_tiles": wt.value}


def sparse_fade_plan(mask_a, mask_b, block_size: int) -> dict:
    """What one block of a sparse fade from mask A to mask B will cost, on the host
    (neo_hip_upols_sparse_fade_plan; no device or handle needed). Masks [C][P][B+1] or [P][B+1],
    true = keep. Returns `tiles_a`, `tiles_b`, `tiles_union` (kept 128-byte tiles of A, of B and
    of A | B: a fade step loads each bank's kept filter tiles and each delay-line tile of the union
    once), `splits` (of a sparse handle of that shape with default options) and `step_bytes`, the
    model bytes of one fade step: 128 (tiles_a + tiles_b + tiles_union) + both banks' bitmap words
    and offsets + the inserted row + the slabs + the block in and out."""
    ms = []
    for mask in (mask_a, mask_b):
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[2] != block_size + 1:
            raise ValueError(f"mask must be [C][P][{block_size + 1}], got {m.shape}")
        ms.append(m)
    if ms[0].shape != ms[1].shape:
        raise ValueError(f"the two masks differ in shape: {ms[0].shape} and {ms[1].shape}")
    C, P, _ = ms[0].shape
    ta, tb, tu, sb, sp = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    _native.check(_native.load().neo_hip_upols_sparse_fade_plan(_ptr(ms[0]), _ptr(ms[1]), C, int(block_size), P,
                                                                ctypes.byref(ta), ctypes.byref(tb), ctypes.byref(tu),
                                                                ctypes.byref(sp), ctypes.byref(sb)))
    return {"tiles_a": ta.value, "tiles_b": tb.value, "tiles_union": tu.value, "splits": sp.value,
            "step_bytes": sb.value}


def a_weighting(frequency):
    """neo::a_weighting (src/neo/math/a_weighting.hpp; extra/python/src/main.cpp:260-263): the
    A-weighting in dB at `frequency` Hz, vectorised, in the input's float dtype (float64 for
    anything that is not float32)."""
    f = np.asarray(frequency)
    dt = np.float32 if f.dtype == np.float32 else np.float64
    f = f.astype(dt, copy=False)
    c = np.array([12194.217, 20.598997, 107.65265, 737.86223], dtype=dt) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        f2 = f * f
        out = dt(2) + dt(20) * (np.log10(c[0]) + dt(2) * np.log10(f2) - np.log10(f2 + c[0]) - np.log10(f2 + c[1])
                                - dt(0.5) * np.log10(f2 + c[2]) - dt(0.5) * np.log10(f2 + c[3]))
    return out.astype(dt, copy=False) if out.ndim else dt(out)


def amplitude_to_db(gain, infinity=-144.0):
    """neo::amplitude_to_db (src/neo/unit/decibel.hpp; main.cpp:264-267): 20 log10(gain), floored
    at `infinity`, which is also the value for gain <= 0; vectorised, in the input's float dtype."""
    g = np.asarray(gain)
    dt = np.float32 if g.dtype == np.float32 else np.float64
    g = g.astype(dt, copy=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = np.maximum(dt(infinity), dt(20) * np.log10(g))
    out = np.where(g <= 0, dt(infinity), db).astype(dt, copy=False)
    return out if out.ndim else dt(out)


class PerceptualSparsity:
    """The plugin's sparsity rule (sparse_convolve, DenseConvolution.cpp:110-170; neo_hip_perceptual
    in include/neo_hip.h): keep a filter bin iff its level relative to its channel's strongest bin,
    in dB, plus the weight of its column (A-weighting at `sample_rate`, or none; 100 for the first
    `low_bins_to_keep` columns) exceeds `threshold_db`. Accepted wherever a sparse filter takes a
    mask; the mask is then made on the device."""

    WEIGHTINGS = {"none": 0, "a": 1}

    def __init__(self, sample_rate: float, threshold_db: float, low_bins_to_keep: int = 0, weighting: str = "a"):
        if weighting not in self.WEIGHTINGS:
            raise ValueError(f"weighting must be 'a' or 'none', got {weighting!r}")
        self.sample_rate, self.threshold_db = float(sample_rate), float(threshold_db)
        self.low_bins_to_keep, self.weighting = int(low_bins_to_keep), weighting

    def _c(self) -> "_native.Perceptual":
        return _native.Perceptual(self.sample_rate, self.threshold_db, self.low_bins_to_keep,
                                  self.WEIGHTINGS[self.weighting])

    def __repr__(self) -> str:
        return (f"PerceptualSparsity(sample_rate={self.sample_rate}, threshold_db={self.threshold_db}, "
                f"low_bins_to_keep={self.low_bins_to_keep}, weighting={self.weighting!r})")


PERCEPTUAL_BUCKETS = 144


def perceptual_weights(block_size: int, sparsity: PerceptualSparsity) -> np.ndarray:
    """The weight table [B+1] float32 of `sparsity` for blocks of `block_size` (no device needed)."""
    p = sparsity._c()
    w = np.empty(min(max(0, int(block_size)), 4096) + 1, dtype=np.float32)  # other blocks are refused
    _native.check(_native.load().neo_hip_perceptual_weights(int(block_size), ctypes.byref(p), _ptr(w)))
    return w


def _host_partitions(partitions) -> np.ndarray:
    H = np.ascontiguousarray(partitions, dtype=np.complex64)
    if H.ndim == 2:
        H = H[None]
    if H.ndim != 3 or H.shape[2] < 2:
        raise ValueError(f"partitions must be [C][P][B+1], got {H.shape}")
    return H


def _device_partitions(t):
    import torch

    if t.dtype != torch.complex64 or not t.is_contiguous():
        raise TypeError("partitions must be a contiguous complex64 tensor")
    shape = (1,) + tuple(t.shape) if t.dim() == 2 else tuple(t.shape)
    if len(shape) != 3 or shape[2] < 2:
        raise ValueError(f"partitions must be [C][P][B+1], got {tuple(t.shape)}")
    return shape


def perceptual_mask_host(partitions, sparsity: PerceptualSparsity) -> np.ndarray:
    """The definition of the predicate, on the host (neo_hip_perceptual_mask_host; no device
    needed): `partitions` [C][P][B+1] complex64 -> bool mask of the same shape."""
    H = _host_partitions(partitions)
    C, P, bins = H.shape
    p = sparsity._c()
    m = np.empty(H.shape, dtype=np.uint8)
    _native.check(_native.load().neo_hip_perceptual_mask_host(_ptr(H), C, bins - 1, P, ctypes.byref(p), _ptr(m)))
    return m.view(np.bool_)


def perceptual_mask(partitions, sparsity: PerceptualSparsity, device: int = 0):
    """The predicate on the device (neo_hip_perceptual_mask): a host array gives a host bool array,
    a CUDA tensor a CUDA bool tensor on its device (nothing crosses PCIe)."""
    p = sparsity._c()
    if _is_torch(partitions) and partitions.is_cuda:
        import torch

        C, P, bins = _device_partitions(partitions)
        m = torch.empty((C, P, bins), dtype=torch.uint8, device=partitions.device)
        _producer_join(partitions)
        _native.check(_native.load().neo_hip_perceptual_mask(ctypes.c_void_p(partitions.data_ptr()), C, bins - 1, P,
                                                             ctypes.byref(p), ctypes.c_void_p(m.data_ptr()), 1,
                                                             partitions.device.index or 0))
        return m.view(torch.bool)
    if _is_torch(partitions):
        partitions = partitions.numpy()
    H = _host_partitions(partitions)
    C, P, bins = H.shape
    m = np.empty(H.shape, dtype=np.uint8)
    _native.check(_native.load().neo_hip_perceptual_mask(_ptr(H), C, bins - 1, P, ctypes.byref(p), _ptr(m), 0,
                                                         int(device)))
    return m.view(np.bool_)


def perceptual_histogram_host(partitions, sparsity: PerceptualSparsity) -> dict:
    """perceptual_histogram on the host (neo_hip_perceptual_hist_host; no device needed)."""
    H = _host_partitions(partitions)
    C, P, bins = H.shape
    p = sparsity._c()
    hb = np.zeros((C, PERCEPTUAL_BUCKETS), dtype=np.int64)
    ht = np.zeros((C, PERCEPTUAL_BUCKETS), dtype=np.int64)
    _native.check(_native.load().neo_hip_perceptual_hist_host(_ptr(H), C, bins - 1, P, ctypes.byref(p), _ptr(hb),
                                                              _ptr(ht)))
    return {"bins": hb, "tiles": ht}


def perceptual_histogram(partitions, sparsity: PerceptualSparsity, device: int = 0) -> dict:
    """How many columns ("bins") and how many 128-byte tiles ("tiles") of every channel lie at which
    level: [C][144] int64 each, bucket j = levels in (-j - 1, -j] dB (bucket 0 also everything above
    0 dB, bucket 143 everything below). `sparsity.threshold_db` plays no part. The tiles an integer
    threshold -k keeps are tiles[:, :k].sum(axis=1): see tile_density_curve. Host array or CUDA
    tensor; computed on the device either way, the histograms are host arrays."""
    p = sparsity._c()
    if _is_torch(partitions) and partitions.is_cuda:
        C, P, bins = _device_partitions(partitions)
        ptr, on_device, device = ctypes.c_void_p(partitions.data_ptr()), 1, partitions.device.index or 0
        _producer_join(partitions)
    else:
        H = _host_partitions(partitions.numpy() if _is_torch(partitions) else partitions)
        C, P, bins = H.shape
        ptr, on_device = _ptr(H), 0
    hb = np.zeros((C, PERCEPTUAL_BUCKETS), dtype=np.int64)
    ht = np.zeros((C, PERCEPTUAL_BUCKETS), dtype=np.int64)
    _native.check(_native.load().neo_hip_perceptual_histogram(ptr, C, bins - 1, P, ctypes.byref(p), _ptr(hb), _ptr(ht),
                                                              on_device, int(device)))
    return {"bins": hb, "tiles": ht}


def tile_density_curve(hist_tiles) -> np.ndarray:
    """[C][144] kept-tile fractions per channel at the thresholds 0, -1, ..., -143 dB from
    perceptual_histogram's "tiles": entry k is the fraction of the channel's tiles in buckets j < k
    (exactly the tiles a threshold of -k dB keeps; 0 at a threshold of 0 dB, where only a level
    above 0 dB would pass)."""
    h = np.atleast_2d(np.asarray(hist_tiles, dtype=np.int64))
    if h.shape[1] != PERCEPTUAL_BUCKETS:
        raise ValueError(f"hist_tiles must be [C][{PERCEPTUAL_BUCKETS}], got {h.shape}")
    kept = np.zeros(h.shape, dtype=np.float64)
    kept[:, 1:] = np.cumsum(h, axis=1)[:, :-1]
    total = h.sum(axis=1, keepdims=True)
    return kept / np.maximum(total, 1)


def threshold_for_tile_density(hist_tiles, target: float):
    """The lowest integer threshold in dB (the widest dynamic range) among -1 .. -143, where the
    histogram's counts are exact, at which the kept tiles over ALL channels are at most `target`
    of all tiles, or None if none is (bucket 0 is kept at every one of them: levels above -1 dB,
    low_bins_to_keep's +100 among them). Host logic on perceptual_histogram's "tiles"; a sparse
    handle beats the dense step below about 2 % kept tiles."""
    h = np.atleast_2d(np.asarray(hist_tiles, dtype=np.int64))
    if h.shape[1] != PERCEPTUAL_BUCKETS:
        raise ValueError(f"hist_tiles must be [C][{PERCEPTUAL_BUCKETS}], got {h.shape}")
    total = int(h.sum())
    if total == 0:
        return None
    kept = np.concatenate([[0], np.cumsum(h.sum(axis=0))[:-1]])  # at thresholds 0, -1, ..., -143
    ok = np.nonzero(kept[1:] <= float(target) * total)[0]  # kept grows with k: the last one is the lowest
    return -int(ok[-1] + 1) if ok.size else None


class SparseUpolsConvolver(UpolsConvolver):
    """C independent sparse UPOLS / UPOLA convolvers stepped together (neo_hip_upols_create_sparse):
    only the filter bins a mask keeps take part, kept as 128-byte tiles of 16 packed bins; a block
    step reads the kept tiles of the filter and of the FDL rows only. Results are those of the
    dense convolver on the filter with the dropped columns zeroed. Of `options` only fused and
    split_workgroups apply; there are no streaming levels, offline windows or latency mode (their
    setters raise), and the dense forms filter(partitions) and set_impulse(ir) do not apply: a
    sparse filter takes a mask or a PerceptualSparsity. Batched passes are off by default (one
    block per pass); set_batch(True) lets process_blocks / process run T blocks per pass over the
    kept tiles, as an offline caller wants them (sparse_convolve does)."""

    def __init__(self, channels: int, block_size: int, partitions: int, device: int = 0, method: str = "upols",
                 options: dict | None = None):
        methods = {"upols": 0, "upola": 1}
        if method not in methods:
            raise ValueError(f"method must be 'upols' or 'upola', got {method!r}")
        opts = dict(self.OPTION_DEFAULTS)
        for k, v in (options or {}).items():
            if k not in ("fused", "split_workgroups"):
                raise ValueError(f"sparse convolvers take the options fused and split_workgroups, got {k!r}")
            opts[k] = int(v)
        o = _native.UpolsOpts(**opts)
        h = ctypes.c_void_p()
        _native.check(_native.load().neo_hip_upols_create_sparse(int(channels), int(block_size), int(partitions),
                                                                 int(device), methods[method], ctypes.byref(o),
                                                                 ctypes.byref(h)))
        self._h = h
        self.channels, self.block_size, self.partitions, self.device = channels, block_size, partitions, device
        self.method = method

    def filter(self, partitions, mask) -> None:
        """sparse_filter's filter(matrix, sparsity) for every channel: `partitions` [C][P][B+1]
        complex64 and `mask` [C][P][B+1] (true = keep), host arrays or CUDA tensors (both on the
        same side); resets FDL, window and write position. `mask` may be a PerceptualSparsity: the
        mask is then made on the device from the partitions (neo_hip_upols_set_filter_perceptual;
        the same handle as filter(partitions, perceptual_mask(partitions, sparsity)))."""
        shape = (self.channels, self.partitions, self.block_size + 1)
        lib = _native.load()
        if isinstance(mask, PerceptualSparsity):
            p = mask._c()
            if _is_torch(partitions) and partitions.is_cuda:
                if _device_partitions(partitions) != shape:
                    raise ValueError(f"filter must be {shape}")
                _producer_join(partitions)
                _native.check(lib.neo_hip_upols_set_filter_perceptual(self._h, ctypes.c_void_p(partitions.data_ptr()),
                                                                      ctypes.byref(p), 1))
                return
            H = _host_partitions(partitions.numpy() if _is_torch(partitions) else partitions)
            if H.shape != shape:
                raise ValueError(f"filter shape {H.shape} != {shape}")
            _native.check(lib.neo_hip_upols_set_filter_perceptual(self._h, _ptr(H), ctypes.byref(p), 0))
            return
        if _is_torch(partitions) and partitions.is_cuda:
            import torch

            m = mask if _is_torch(mask) else torch.as_tensor(np.asarray(mask))
            m = (m != 0).to(device=partitions.device, dtype=torch.uint8).contiguous()
            if partitions.dtype != torch.complex64 or not partitions.is_contiguous():
                raise TypeError("filter takes a contiguous complex64 tensor")
            if partitions.numel() != int(np.prod(shape)) or m.numel() != partitions.numel():
                raise ValueError(f"filter and mask must be {shape}")
            _producer_join(partitions)
            torch.cuda.current_stream(partitions.device).synchronize()  # the mask made above
            _native.check(lib.neo_hip_upols_set_filter_sparse(self._h, ctypes.c_void_p(partitions.data_ptr()),
                                                              ctypes.c_void_p(m.data_ptr()), 1))
            return
        if _is_torch(partitions):
            partitions = partitions.numpy()
        if _is_torch(mask):
            mask = mask.cpu().numpy()
        H = np.ascontiguousarray(partitions, dtype=np.complex64)
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if H.ndim == 2:
            H = H[None]
        if m.ndim == 2:
            m = m[None]
        if H.shape != shape or m.shape != shape:
            raise ValueError(f"filter shape {H.shape} / mask shape {m.shape} != {shape}")
        _native.check(lib.neo_hip_upols_set_filter_sparse(self._h, _ptr(H), _ptr(m), 0))

    def set_impulse(self, impulse_response, sparsity=None, normalize: bool = True) -> None:
        """normalize_impulse (optional), uniform_partition, the mask of `sparsity` (a
        PerceptualSparsity) and the tiles, all on the device (neo_hip_upols_set_impulse_perceptual):
        [C][L] float32, host array or CUDA tensor. Without a PerceptualSparsity there is no
        rule to thin by: that form stays refused, as on every sparse handle."""
        lib = _native.load()
        if not isinstance(sparsity, PerceptualSparsity):
            if isinstance(sparsity, (bool, np.bool_)):  # the base class's (impulse_response, normalize)
                return super().set_impulse(impulse_response, bool(sparsity))
            if sparsity is not None:
                raise TypeError("set_impulse on a sparse convolver takes a PerceptualSparsity")
            return super().set_impulse(impulse_response, normalize)
        p = sparsity._c()
        if _is_torch(impulse_response) and impulse_response.is_cuda:
            import torch

            t = impulse_response
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError("set_impulse takes a contiguous float32 tensor")
            if (1 if t.dim() == 1 else t.shape[0]) != self.channels:
                raise ValueError("impulse channel count mismatch")
            _producer_join(t)
            _native.check(lib.neo_hip_upols_set_impulse_perceptual(self._h, ctypes.c_void_p(t.data_ptr()), t.shape[-1],
                                                                   int(normalize), ctypes.byref(p), 1))
            return
        if _is_torch(impulse_response):
            impulse_response = impulse_response.numpy()
        ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float32)))
        if ir.shape[0] != self.channels:
            raise ValueError("impulse channel count mismatch")
        _native.check(lib.neo_hip_upols_set_impulse_perceptual(self._h, _ptr(ir), ir.shape[1], int(normalize),
                                                               ctypes.byref(p), 0))

    # -- live updates -------------------------------------------------------
    def update_filter(self, partitions, mask=None, fade_blocks: int = 1, curve: str = "linear", stream: int = 0) -> None:
        """Live update of a sparse convolver (neo_hip_upols_update_filter_sparse / _perceptual):
        crossfade from the current sparse filter to `partitions` [C][P][B+1] under `mask` (an array
        or tensor [C][P][B+1], true = keep, or a PerceptualSparsity, as filter() takes it) over the
        next fade_blocks blocks and KEEP ALL STATE; filter() and set_impulse() remain the resetting
        calls. Sample n of the fade is y_A + g[n] (y_B - y_A) with g = fade_gains(block_size,
        fade_blocks, curve), y_A and y_B the outputs of two sparse convolvers that had the old and
        the new filter from the start. Turning the threshold knob is update_filter(the same
        partitions, another PerceptualSparsity). Host arrays and CUDA tensors; unlike the dense
        update a CUDA tensor's call is NOT asynchronous: it waits on its stream (torch's current
        stream, or `stream`; the stream the process calls run on) for the kept-tile counts that size
        the new tiles. Without a mask the call falls through to the dense form, which the library
        refuses on a sparse handle."""
        if mask is None:
            return super().update_filter(partitions, fade_blocks, curve, stream)
        c = _fade_curve(curve)
        lib = _native.load()
        shape = (self.channels, self.partitions, self.block_size + 1)
        perceptual = mask._c() if isinstance(mask, PerceptualSparsity) else None
        if _is_torch(partitions) and partitions.is_cuda:
            import torch

            if partitions.dtype != torch.complex64 or not partitions.is_contiguous() or partitions.numel() != int(np.prod(shape)):
                raise ValueError(f"filter must be a contiguous complex64 tensor of {shape}")
            _producer_join(partitions)
            current = torch.cuda.current_stream(partitions.device)
            s = ctypes.c_void_p(stream or current.cuda_stream or None)
            if perceptual is not None:
                _native.check(lib.neo_hip_upols_update_filter_perceptual(self._h, ctypes.c_void_p(partitions.data_ptr()),
                                                                         ctypes.byref(perceptual), 1, int(fade_blocks), c, s))
                return
            m = mask if _is_torch(mask) else torch.as_tensor(np.asarray(mask))
            m = (m != 0).to(device=partitions.device, dtype=torch.uint8).contiguous()
            if m.numel() != partitions.numel():
                raise ValueError(f"mask must be {shape}")
            if stream and stream != current.cuda_stream:
                current.synchronize()  # the mask made above, on another stream than the call's
            _native.check(lib.neo_hip_upols_update_filter_sparse(self._h, ctypes.c_void_p(partitions.data_ptr()),
                                                                 ctypes.c_void_p(m.data_ptr()), 1, int(fade_blocks), c, s))
            return
        H = _host_partitions(partitions.numpy() if _is_torch(partitions) else partitions)
        if H.shape != shape:
            raise ValueError(f"filter shape {H.shape} != {shape}")
        s = ctypes.c_void_p(stream or None)
        if perceptual is not None:
            _native.check(lib.neo_hip_upols_update_filter_perceptual(self._h, _ptr(H), ctypes.byref(perceptual), 0,
                                                                     int(fade_blocks), c, s))
            return
        if _is_torch(mask):
            mask = mask.cpu().numpy()
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.ndim == 2:
            m = m[None]
        if m.shape != shape:
            raise ValueError(f"mask shape {m.shape} != {shape}")
        _native.check(lib.neo_hip_upols_update_filter_sparse(self._h, _ptr(H), _ptr(m), 0, int(fade_blocks), c, s))

    def update_impulse(self, impulse_response, sparsity=None, normalize: bool = True, fade_blocks: int = 1,
                       curve: str = "linear", stream: int = 0) -> None:
        """update_filter from impulse responses [C][L] float32 (host array or CUDA tensor) under a
        PerceptualSparsity: normalize_impulse (optional), uniform_partition, the mask and the tiles
        on the device (neo_hip_upols_update_impulse_perceptual), the same handle as
        update_filter(P, perceptual_mask(P, sparsity)) with P = uniform_partition(normalize_impulse
        (ir)). Keeps all state. Without a sparsity the call falls through to the dense form, which
        the library refuses on a sparse handle."""
        if sparsity is None:
            return super().update_impulse(impulse_response, normalize, fade_blocks, curve, stream)
        if not isinstance(sparsity, PerceptualSparsity):
            raise TypeError("update_impulse on a sparse convolver takes a PerceptualSparsity")
        c = _fade_curve(curve)
        lib = _native.load()
        p = sparsity._c()
        if _is_torch(impulse_response) and impulse_response.is_cuda:
            import torch

            t = impulse_response
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.channels * t.shape[-1]:
                raise ValueError("impulse must be a contiguous float32 tensor of one row per channel")
            _producer_join(t)
            current = torch.cuda.current_stream(t.device).cuda_stream
            _native.check(lib.neo_hip_upols_update_impulse_perceptual(self._h, ctypes.c_void_p(t.data_ptr()), t.shape[-1],
                                                                      int(normalize), ctypes.byref(p), 1, int(fade_blocks), c,
                                                                      ctypes.c_void_p(stream or current or None)))
            return
        if _is_torch(impulse_response):
            impulse_response = impulse_response.numpy()
        ir = np.ascontiguousarray(np.atleast_2d(np.asarray(impulse_response, dtype=np.float32)))
        if ir.shape[0] != self.channels:
            raise ValueError("impulse channel count mismatch")
        _native.check(lib.neo_hip_upols_update_impulse_perceptual(self._h, _ptr(ir), ir.shape[1], int(normalize),
                                                                  ctypes.byref(p), 0, int(fade_blocks), c,
                                                                  ctypes.c_void_p(stream or None)))

    def sparse_info(self) -> dict:
        """The current filter's kept columns and kept 128-byte tiles over all channels, and the
        device bytes (tiles, bitmaps, offsets) that stand in for a dense handle's filter buffer;
        from an update_filter / update_impulse call on, the filter being faded to."""
        kb, kt, fb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols_sparse_info(self._h, ctypes.byref(kb), ctypes.byref(kt),
                                                               ctypes.byref(fb)))
        return {"kept_bins": kb.value, "kept_tiles": kt.value, "filter_bytes": fb.value}

    def sparse_batch_info(self) -> dict:
        """The batched pass of this handle, on or off (neo_hip_upols_sparse_batch_info): its blocks
        per pass T, its splits per channel, and the popcount sum of the window bitmaps the device
        made for T at the last filter change (sparse_window_plan's `window_tiles`)."""
        t, sp, wt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_upols_sparse_batch_info(self._h, ctypes.byref(t), ctypes.byref(sp),
                                                                     ctypes.byref(wt)))
        return {"blocks_per_pass": t.value, "splits": sp.value, "window_tiles": wt.value}


class sparse_upols_convolver:
    """Single-channel drop-in for sparse_upols_convolver<complex<float>> (sparse_convolver.hpp:
    12-13): filter([P][B+1], sparsity) then __call__(block[B]) in place. `sparsity` is a bool
    array [P][B+1] or a callable (row, col, value) -> bool, as sparse_filter::filter takes it
    (sparse_filter.hpp:25-28, csr_matrix.hpp:32-34)."""

    _method = "upols"

    def __init__(self, device: int = 0):
        self._impl = None
        self._device = device

    def filter(self, filt, sparsity) -> None:
        H = np.ascontiguousarray(filt, dtype=np.complex64)
        if H.ndim != 2:
            raise ValueError("filter must be [P][B+1]")
        P, bins = H.shape
        if isinstance(sparsity, PerceptualSparsity):  # the mask is made on the device
            mask = sparsity
        elif callable(sparsity):
            mask = np.array([[bool(sparsity(r, c, H[r, c])) for c in range(bins)] for r in range(P)], dtype=bool)[None]
        else:
            mask = (np.asarray(sparsity) != 0)
            if mask.shape != H.shape:
                raise ValueError(f"sparsity shape {mask.shape} != filter shape {H.shape}")
            mask = mask[None]
        impl = self._impl
        if impl is None or (impl.partitions, impl.block_size) != (P, bins - 1):
            impl = SparseUpolsConvolver(1, bins - 1, P, self._device, method=self._method)
        impl.filter(H[None], mask)
        self._impl = impl

    def __call__(self, block):
        if self._impl is None:
            raise RuntimeError("filter() must be called first")
        return self._impl(block)


class sparse_upola_convolver(sparse_upols_convolver):
    """Single-channel drop-in for sparse_upola_convolver<complex<float>> (sparse_convolver.hpp:16-17)."""

    _method = "upola"


def sparse_convolve(signal, impulse_response, block_size: int, mask, method: str = "upola", device: int = 0,
                    options: dict | None = None) -> np.ndarray:
    """The plugin's sparse_convolve loop (DenseConvolution.cpp:124-186): normalize the IR matrix,
    partition it, keep the filter bins `mask` ([C][P][B+1], true = keep, or a PerceptualSparsity:
    the plugin's own A-weighted threshold from sampleRate, thresholdDB and lowBinsToKeep, applied
    on the device) and run every block (tail zero-padded) through sparse_upola_convolver (or
    sparse_upols_convolver) per channel; output truncated to N. Every block is known up front, so
    the handle runs batched passes (T blocks per pass over the kept tiles)."""
    sig = np.ascontiguousarray(np.atleast_2d(np.asarray(signal, dtype=np.float32)))
    ir = np.array(np.atleast_2d(np.asarray(impulse_response, dtype=np.float32)), order="C")
    C, N = sig.shape
    if ir.shape[0] != C:
        raise ValueError("signal and impulse response channel counts differ")
    if isinstance(mask, PerceptualSparsity):
        conv = SparseUpolsConvolver(C, block_size, num_partitions(ir.shape[1], block_size), device, method=method,
                                    options=options)
        conv.set_impulse(ir, mask, normalize=True)
    else:
        parts = uniform_partition(normalize_impulse(ir, device), block_size, device)
        conv = SparseUpolsConvolver(C, block_size, parts.shape[1], device, method=method, options=options)
        conv.filter(parts, mask)
    conv.set_batch(True)
    nb = -(-N // block_size)
    buf = np.zeros((C, nb * block_size), dtype=np.float32)
    buf[:, :N] = sig
    conv.process(buf)
    conv.close()
    return buf[:, :N].copy()


def _one_shot(name, signal, patch, device):
    """The reference binds float then double (main.cpp:255-258): a float64 pair picks the
    double overload, anything else converts to float32 (pybind11's converting pass)."""
    a = np.asarray(signal)
    b = np.asarray(patch)
    if a.ndim != 1 or b.ndim != 1:
        raise RuntimeError("unsupported dimension: in1 and in2 must be 1-D")  # main.cpp:173-175
    f64 = a.dtype == np.float64 and b.dtype == np.float64
    dt = np.float64 if f64 else np.float32
    a = np.ascontiguousarray(a, dtype=dt)
    b = np.ascontiguousarray(b, dtype=dt)
    if a.size == 0 or b.size == 0:
        return np.zeros(0, dt)
    out = np.empty(a.size + b.size - 1, dt)
    fn = getattr(_native.load(), name + ("_f64" if f64 else ""))
    _native.check(fn(_ptr(a), a.size, _ptr(b), b.size, _ptr(out), 0, int(device)))
    return out


def fft_convolve(signal, patch, device: int = 0) -> np.ndarray:
    """Full linear convolution through one r2c/c2r pair (fft_convolver.hpp:19-93)."""
    return _one_shot("neo_hip_fft_convolve", signal, patch, device)


def direct_convolve(signal, patch, device: int = 0) -> np.ndarray:
    """Full linear convolution, direct sum (direct_convolve.hpp:14-56), bit-identical loop order."""
    return _one_shot("neo_hip_direct_convolve", signal, patch, device)


def convolve(in1, in2, mode: str = "full", method: str = "auto", device: int = 0) -> np.ndarray:
    """neo.convolve (extra/python/src/neo/__init__.py:43-48): method "fft" -> fft_convolve,
    anything else -> direct_convolve; only mode "full" (others raise RuntimeError, main.cpp:197)."""
    if mode not in ("full", "valid", "same"):
        raise KeyError(mode)
    if mode != "full":
        raise RuntimeError("unsupported convolution mode")
    if method == "fft":
        return fft_convolve(in1, in2, device)
    return direct_convolve(in1, in2, device)


# -- matrix (multi-input, multi-output) convolver ------------------------------------------------

def _routes(routes, inputs: int, outputs: int):
    """routes=None: the dense list of all (out, in) pairs, row-major. -> two int32 arrays."""
    if routes is None:
        ro, ri = np.divmod(np.arange(int(outputs) * int(inputs), dtype=np.int32), np.int32(inputs))
    else:
        r = np.asarray(list(routes), dtype=np.int64).reshape(-1, 2)
        ro, ri = r[:, 0], r[:, 1]
    return np.ascontiguousarray(ro, dtype=np.int32), np.ascontiguousarray(ri, dtype=np.int32)


def _matrix_opts(options) -> "_native.MatrixOpts":
    opts = dict(MatrixConvolver.OPTION_DEFAULTS)
    for k, v in (options or {}).items():
        if k not in opts:
            raise ValueError(f"unknown matrix convolver option {k!r}")
        opts[k] = int(v)
    return _native.MatrixOpts(**opts)


def matrix_plan(inputs: int, outputs: int, block_size: int, partitions: int, routes=None, options=None) -> dict:
    """The plan of a matrix convolver for a route list and options (neo_hip_matrix_plan; no device
    needed, the function the handle itself is built from): the out_tile in use, fused, splits, the
    tiles (first output, count, row count, the union of their inputs, the split cuts into the row
    list) and the step's totals of FDL-row and filter-row loads; `bytes` = 8 B (loads) plus the
    block I/O, the algorithmic bytes of one step."""
    ro, ri = _routes(routes, inputs, outputs)
    o = _matrix_opts(options)
    info = _native.MatrixPlanInfo()
    O, I = max(1, int(outputs)), max(1, int(inputs))
    first, count, rows = (np.zeros(O, np.int32) for _ in range(3))
    uoff, uin, cuts = np.zeros(O + 1, np.int32), np.zeros(O * I, np.int32), np.zeros((O, 65), np.int32)
    _native.check(_native.load().neo_hip_matrix_plan(int(inputs), int(outputs), int(block_size), int(partitions),
                                                     _ptr(ro), _ptr(ri), len(ro), ctypes.byref(o), ctypes.byref(info),
                                                     _ptr(first), _ptr(count), _ptr(rows), _ptr(uoff), _ptr(uin),
                                                     _ptr(cuts)))
    n, S = info.tiles, info.splits
    tiles = [{"first": int(first[t]), "count": int(count[t]), "rows": int(rows[t]),
              "inputs": [int(i) for i in uin[uoff[t]:uoff[t + 1]]], "cuts": [int(c) for c in cuts[t, :S + 1]]}
             for t in range(n)]
    loads = info.fdl_row_loads + info.filter_row_loads
    return {"out_tile": info.out_tile, "fused": bool(info.fused), "splits": S, "tiles": tiles,
            "fdl_row_loads": info.fdl_row_loads, "filter_row_loads": info.filter_row_loads,
            "bytes": 8 * int(block_size) * loads + 4 * int(block_size) * (int(inputs) + int(outputs))}


def matrix_batch_plan(inputs: int, outputs: int, block_size: int, partitions: int, routes=None, blocks: int = 32,
                      split_workgroups: int = 0) -> dict:
    """The plan of a batched pass of `blocks` blocks of a matrix convolver (neo_hip_matrix_batch_plan;
    no device needed, the function the handle itself is built from): the splits per output, the bin
    chunks per row, per output its row count and per split its runs (input, first partition, one
    past the last), and the pass's totals: filter_row_loads (routes x P), fdl_row_loads (per run its
    length + blocks - 1), slab_rows and `bytes` = 8 B (filter + FDL rows + 2 slab rows) plus the
    block I/O of all `blocks` blocks."""
    ro, ri = _routes(routes, inputs, outputs)
    info = _native.MatrixBatchPlanInfo()
    O = max(1, int(outputs))
    rows, off = np.zeros(O, np.int32), np.zeros((O, 65), np.int32)
    rin, rfirst, rlast = (np.zeros(len(ro) + 63 * O, np.int32) for _ in range(3))
    _native.check(_native.load().neo_hip_matrix_batch_plan(int(inputs), int(outputs), int(block_size), int(partitions),
                                                           _ptr(ro), _ptr(ri), len(ro), int(blocks),
                                                           int(split_workgroups), ctypes.byref(info), _ptr(rows),
                                                           _ptr(off), _ptr(rin), _ptr(rfirst), _ptr(rlast)))
    S = info.splits
    outs = [{"rows": int(rows[o]),
             "splits": [[(int(rin[k]), int(rfirst[k]), int(rlast[k])) for k in range(off[o, s], off[o, s + 1])]
                        for s in range(S)]} for o in range(int(outputs))]
    return {"blocks": info.blocks, "splits": S, "chunks": info.chunks, "runs": info.runs, "outputs": outs,
            "filter_row_loads": info.filter_row_loads, "fdl_row_loads": info.fdl_row_loads,
            "slab_rows": info.slab_rows, "bytes": info.bytes}


def matrix_offline_plan(inputs: int, outputs: int, block_size: int, partitions: int, routes=None, windows: int = 0,
                        write_pos: int = 0, ring_rows: int = 0) -> dict:
    """The plan of an offline pass of a matrix convolver (neo_hip_matrix_offline_plan; no device
    needed, the function the launcher takes its rows from): `windows` (0 = automatic = 2, 1 or 2)
    windows of 128 blocks at ring row `write_pos` of a ring of `ring_rows` rows (0 = the least a
    handle takes, min_ring_rows). segments = ceil(P / 128); a PAIR is 256 consecutive ring rows
    (mod ring_rows): pair_rows[k] is the first row of pair k and pair_of[window][segment] the pair
    that window's segment multiplies. hf_bytes / xf_bytes are the payloads of the segment and pair
    spectra; `bytes` is the pass's model: 8 B (spectrum_rows + pair_cache_rows + fdl_rows +
    pair_rows_written + output_rows) plus the block I/O, of which cache_bytes (the pair spectra
    re-read once per route, expected from L2 / Infinity Cache) are 8 B pair_cache_rows."""
    ro, ri = _routes(routes, inputs, outputs)
    info = _native.MatrixOfflinePlanInfo()
    nseg = max(1, (max(1, int(partitions)) + 127) // 128)
    rows, of = np.zeros(nseg + 1, np.int32), np.zeros((2, nseg), np.int32)
    _native.check(_native.load().neo_hip_matrix_offline_plan(int(inputs), int(outputs), int(block_size),
                                                             int(partitions), _ptr(ro), _ptr(ri), len(ro), int(windows),
                                                             int(write_pos), int(ring_rows), ctypes.byref(info),
                                                             _ptr(rows), _ptr(of)))
    d = {n: int(getattr(info, n)) for n, _ in _native.MatrixOfflinePlanInfo._fields_}
    d["pair_rows"] = [int(r) for r in rows[:info.pairs]]
    d["pair_of"] = [[int(k) for k in of[w, :info.segments]] for w in range(info.windows)]
    return d


def _windows(windows):
    """windows=None: the library's default (a NULL list). -> (int32 array or None, pointer, count)"""
    if windows is None:
        return None, None, 0
    w = np.ascontiguousarray(list(windows), dtype=np.int32).reshape(-1)
    n = len(w)
    if not n:  # an empty list is not the default: a real pointer and a count of 0, the library's refusal
        w = np.zeros(1, np.int32)
    return w, _ptr(w), n


def matrix_level_plan(inputs: int, outputs: int, block_size: int, partitions: int, routes=None, windows=None,
                      split_workgroups: int = 0) -> dict:
    """The window-level plan of a matrix convolver (neo_hip_matrix_level_plan; no device needed, the
    function the handle itself is built from). `windows`: ascending powers of two from 2 .. 32, each
    at least twice the one before (None: the default, 8, 32). The head, the ordinary step, takes partitions
    [0, head); level l with window length `window` takes the band [first, last) and is, per window of
    `window` blocks, `workgroups` = outputs x splits x chunks workgroups (workgroup = (output x splits
    + split) x chunks + chunk), cut into `window` parts: part k is the workgroups [part_cuts[k],
    part_cuts[k + 1]), launched at block n = k (mod window) for the window after that block's.
    Per level, outputs[o][s] lists the runs (input, first partition, one past the last) of split s of
    output o; filter_rows and fdl_rows are the row loads of one window. ring_rows: the least ring of
    the schedule, priming included. partial_bytes: the levels' double-buffered slabs;
    head_bank_bytes: the head's compact bank. `bytes`: the model of ONE block (include/neo_hip.h).
    levels == [] (partitions <= head): the handle runs the ordinary step."""
    ro, ri = _routes(routes, inputs, outputs)
    w, wp, nw = _windows(windows)
    info = _native.MatrixLevelPlanInfo()
    O, L = max(1, int(outputs)), _native.MATRIX_MAX_LEVELS
    cuts, off = np.zeros((L, 33), np.int32), np.zeros((L, 64 * O + 1), np.int32)
    rin, rfirst, rlast = (np.zeros((L, len(ro) + 63 * O), np.int32) for _ in range(3))
    _native.check(_native.load().neo_hip_matrix_level_plan(int(inputs), int(outputs), int(block_size), int(partitions),
                                                           _ptr(ro), _ptr(ri), len(ro), wp, nw, int(split_workgroups),
                                                           ctypes.byref(info), _ptr(cuts), _ptr(off), _ptr(rin),
                                                           _ptr(rfirst), _ptr(rlast)))
    levels = []
    for l in range(info.levels):
        T, S = info.window[l], info.splits[l]
        outs = [[[(int(rin[l, k]), int(rfirst[l, k]), int(rlast[l, k])) for k in range(off[l, o * S + s], off[l, o * S + s + 1])]
                 for s in range(S)] for o in range(int(outputs))]
        levels.append({"window": T, "first": info.first[l], "last": info.last[l], "splits": S,
                       "workgroups": info.workgroups[l], "runs": info.runs[l],
                       "part_cuts": [int(c) for c in cuts[l, :T + 1]], "outputs": outs,
                       "filter_rows": info.filter_rows[l], "fdl_rows": info.fdl_rows[l]})
    return {"head": info.head, "levels": levels, "ring_rows": info.ring_rows, "chunks": info.chunks,
            "head_splits": info.head_splits, "head_out_tile": info.head_out_tile,
            "head_filter_rows": info.head_filter_rows, "head_fdl_rows": info.head_fdl_rows,
            "partial_bytes": info.partial_bytes, "head_bank_bytes": info.head_bank_bytes, "bytes": info.bytes}


def _fade_curve(curve) -> int:
    if isinstance(curve, str):
        if curve not in MatrixConvolver.FADE_CURVES:
            raise ValueError(f"curve must be one of {sorted(MatrixConvolver.FADE_CURVES)}, got {curve!r}")
        return MatrixConvolver.FADE_CURVES[curve]
    return int(curve)  # the library's number (an unknown one is its EINVAL)


def matrix_fade_gains(block: int, fade_blocks: int, curve="linear") -> np.ndarray:
    """The fade_blocks * block float32 gains g[n] of a live filter update (neo_hip_matrix_fade_gains;
    no device needed, the expression the kernel evaluates): t = n / (fade_blocks * block), "linear"
    (0) g = t, "cosine" (1) g = 0.5 - 0.5 cos(pi t). Sample n of the fade is y_A + g[n] (y_B - y_A)."""
    c = _fade_curve(curve)
    ok = 1 <= int(fade_blocks) <= 1 << 20 and 16 <= int(block) <= 4096  # else the library's EINVAL, nothing written
    g = np.zeros(int(fade_blocks) * int(block) if ok else 1, np.float32)
    _native.check(_native.load().neo_hip_matrix_fade_gains(int(block), int(fade_blocks), c, _ptr(g)))
    return g


fade_gains = matrix_fade_gains  # shape-free: the dense convolvers' updates (UpolsConvolver.update_filter) fade by it too


def _matrix_arg(x, np_dtype, count, bad_tensor: str, bad_array: str):
    """A filter or impulse argument of MatrixConvolver -> (array or tensor, which the caller keeps
    alive over the call; its pointer; is_device; torch's current stream or 0). A CUDA tensor must be
    contiguous, of the dtype and hold count(x) elements, and is complete first (_producer_join);
    anything else becomes a contiguous host array of the dtype."""
    if _is_torch(x) and x.is_cuda:
        import torch

        if x.dtype != getattr(torch, np.dtype(np_dtype).name) or not x.is_contiguous() or x.numel() != count(x):
            raise ValueError(bad_tensor)
        _producer_join(x)
        return x, ctypes.c_void_p(x.data_ptr()), 1, torch.cuda.current_stream(x.device).cuda_stream
    a = np.ascontiguousarray(x, dtype=np_dtype)
    if a.size != count(a):
        raise ValueError(bad_array.format(a.shape))
    return a, _ptr(a), 0, 0


def _matrix_filter_arg(partitions, shape):
    return _matrix_arg(partitions, np.complex64, lambda _: int(np.prod(shape)),
                       f"filter must be a contiguous complex64 tensor of {shape} elements",
                       f"filter of {{}} does not hold {shape}")


def _matrix_impulse_arg(ir, nroutes: int):
    """(the rows' length is the last dimension of what comes back)"""
    return _matrix_arg(ir, np.float32, lambda a: nroutes * a.shape[-1],
                       "impulse must be a contiguous float32 tensor of one row per route",
                       "impulse must hold one row per route")


class MatrixConvolver:
    """I inputs routed to O outputs: output o = the sum over its routes (o, i) of the UPOLS (or
    UPOLA) convolution of input i with that route's filter. One delay line per input, one inverse
    transform per output (neo_hip_matrix_*, include/neo_hip.h). Whole blocks: one block per step,
    with set_batch(True) up to 32 blocks of a call per pass over the filters, with set_offline(True)
    windows of 128 blocks by 256-point transforms along the block axis (long filters), with
    set_levels(True) long filters one block per call (the tail of the filter once per window)."""

    OPTION_DEFAULTS = {"fused": -1, "split_workgroups": 0, "out_tile": 0}

    def __init__(self, inputs: int, outputs: int, block_size: int, partitions: int, method: str = "upols",
                 options: dict | None = None, device: int = 0):
        methods = {"upols": 0, "upola": 1}
        if method not in methods:
            raise ValueError(f"method must be 'upols' or 'upola', got {method!r}")
        o = _matrix_opts(options)
        h = ctypes.c_void_p()
        _native.check(_native.load().neo_hip_matrix_create(int(inputs), int(outputs), int(block_size), int(partitions),
                                                           int(device), methods[method], ctypes.byref(o),
                                                           ctypes.byref(h)))
        self._h = h
        self.inputs, self.outputs, self.block_size, self.partitions = int(inputs), int(outputs), int(block_size), int(partitions)
        self.method, self.device = method, device

    # -- setup ------------------------------------------------------------
    def filter(self, partitions, routes=None) -> None:
        """routes None: dense partitions [O][I][P][B+1]; else [nroutes][P][B+1] with routes a list
        of (out, in). complex64 host array or CUDA tensor. Resets all state."""
        ro, ri = _routes(routes, self.inputs, self.outputs)
        H, p, dev, _ = _matrix_filter_arg(partitions, (len(ro), self.partitions, self.block_size + 1))
        _native.check(_native.load().neo_hip_matrix_set_filter(self._h, p, _ptr(ro), _ptr(ri), len(ro), dev))

    def set_impulse(self, ir, routes=None, normalize: bool = True) -> None:
        """ir [O][I][L] (routes None) or [nroutes][L] float32: normalize_impulse over all routes'
        rows (optional), then uniform_partition on the device."""
        ro, ri = _routes(routes, self.inputs, self.outputs)
        a, p, dev, _ = _matrix_impulse_arg(ir, len(ro))
        _native.check(_native.load().neo_hip_matrix_set_impulse(self._h, p, a.shape[-1], _ptr(ro), _ptr(ri), len(ro),
                                                                int(normalize), dev))

    def reset(self) -> None:
        """Clears all state; a running fade (update_filter) completes: the new filter is the filter."""
        _native.check(_native.load().neo_hip_matrix_reset(self._h))

    # -- live updates -------------------------------------------------------
    FADE_CURVES = {"linear": 0, "cosine": 1}

    def update_filter(self, partitions, fade_blocks: int = 1, curve: str = "linear", stream: int = 0) -> None:
        """Live update (neo_hip_matrix_update_filter): crossfade to `partitions` over the next
        fade_blocks blocks and KEEP ALL STATE; filter() remains the resetting call. partitions
        [nroutes][P][B+1] (dense: [O][I][P][B+1]) in the route order of the last filter() /
        set_impulse(): the route list does not change. Sample n of the fade is
        y_A + g[n] (y_B - y_A) with g = matrix_fade_gains(block_size, fade_blocks, curve); curve
        "linear" or "cosine". A CUDA tensor: asynchronous on torch's current stream (or `stream`),
        which must be the stream process() runs on; an ndarray: complete on return."""
        shape = (self.info()["routes"], self.partitions, self.block_size + 1)
        c = _fade_curve(curve)
        lib = _native.load()
        if not shape[0]:  # no filter set: the library's refusal
            _native.check(lib.neo_hip_matrix_update_filter(self._h, _ptr(np.zeros(1, np.complex64)), 0, int(fade_blocks), c, None))
        H, p, dev, current = _matrix_filter_arg(partitions, shape)
        _native.check(lib.neo_hip_matrix_update_filter(self._h, p, dev, int(fade_blocks), c,
                                                       ctypes.c_void_p(stream or current or None)))

    def update_impulse(self, ir, normalize: bool = True, fade_blocks: int = 1, curve: str = "linear",
                       stream: int = 0) -> None:
        """update_filter from impulse responses [nroutes][L] (dense: [O][I][L]) float32:
        normalize_impulse over all routes' rows (optional), then uniform_partition on the device
        into the second bank (neo_hip_matrix_update_impulse). Keeps all state."""
        nroutes = self.info()["routes"]
        c = _fade_curve(curve)
        lib = _native.load()
        if not nroutes:  # no filter set: the library's refusal
            _native.check(lib.neo_hip_matrix_update_filter(self._h, _ptr(np.zeros(1, np.complex64)), 0, int(fade_blocks), c, None))
        a, p, dev, current = _matrix_impulse_arg(ir, nroutes)
        _native.check(lib.neo_hip_matrix_update_impulse(self._h, p, a.shape[-1], int(normalize), dev, int(fade_blocks), c,
                                                        ctypes.c_void_p(stream or current or None)))

    def fade_info(self) -> dict:
        """remaining_blocks of the running fade (0: none), its fade_blocks (0: none) and bank_bytes,
        the second filter bank (0 until the first update after a filter; then info()["filter_bytes"])."""
        r, f, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_matrix_fade_info(self._h, ctypes.byref(r), ctypes.byref(f), ctypes.byref(n)))
        return {"remaining_blocks": r.value, "fade_blocks": f.value, "bank_bytes": n.value}

    def set_batch(self, enable: bool, split_workgroups: int = 0) -> None:
        """Batched passes (neo_hip_matrix_set_batch): process() cuts a call into passes of up to 32
        blocks that share one walk over every route's filter, then single steps. Turning it on grows
        the inputs' rings to P + 31 rows and keeps the stream; split_workgroups 0 = automatic."""
        _native.check(_native.load().neo_hip_matrix_set_batch(self._h, int(bool(enable)), int(split_workgroups)))

    def batch_info(self) -> dict:
        """blocks_per_pass (32 or 1), splits per output of a pass (0 without a filter or with
        batching off) and the rows of every input's ring."""
        b, s, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _native.check(_native.load().neo_hip_matrix_batch_info(self._h, ctypes.byref(b), ctypes.byref(s), ctypes.byref(r)))
        return {"blocks_per_pass": b.value, "splits": s.value, "ring_rows": r.value}

    def set_offline(self, enable: bool, windows_per_pass: int = 0) -> None:
        """Offline windows (neo_hip_matrix_set_offline): process() runs passes of 256 blocks (two
        windows; windows_per_pass 1: 128) while that many are left, by 256-point transforms along the
        block axis: per input the forward ones, per output the inverse ones, per route ceil(P / 128)
        spectrum products. The rest of a call goes as without it. Turning it on grows the inputs'
        rings to 128 (ceil(P / 128) + 2) + 1 rows and keeps the stream."""
        _native.check(_native.load().neo_hip_matrix_set_offline(self._h, int(bool(enable)), int(windows_per_pass)))

    def offline_info(self) -> dict:
        """blocks_per_pass (256 or 128; 0 with offline windows off), segments = ceil(P / 128), the
        rows of every input's ring and the bytes of the segment spectra (0 until they are allocated)."""
        b, g, r, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _native.check(_native.load().neo_hip_matrix_offline_info(self._h, ctypes.byref(b), ctypes.byref(g),
                                                                 ctypes.byref(r), ctypes.byref(n)))
        return {"blocks_per_pass": b.value, "segments": g.value, "ring_rows": r.value, "spectra_bytes": n.value}

    def set_levels(self, enable: bool, windows=None, split_workgroups: int = 0) -> None:
        """Window levels (neo_hip_matrix_set_levels): long filters one block per call. A single step
        then reads only the head, partitions [0, 2 windows[0]), on every block; each level reads its
        band of partitions once per window of its length, one window ahead, in equal parts spread
        over the window's blocks (matrix_level_plan has the plan). windows None: (8, 32);
        split_workgroups: the workgroup target of a part, 0 = automatic. May be turned on or off at
        any time between calls; blocks that ran another way (batched or offline passes, a fade, the
        mode off) are made up for by priming at the next level step, with the same bits."""
        w, wp, nw = _windows(windows)
        _native.check(_native.load().neo_hip_matrix_set_levels(self._h, int(bool(enable)), wp, nw, int(split_workgroups)))

    def levels_info(self) -> dict:
        """enabled, head (partitions of the ordinary step), levels (a list of window, first, last,
        splits; empty without a filter or with partitions <= head: the ordinary step runs), ring_rows,
        primed (the slabs are current), partial_bytes and head_bank_bytes as planned."""
        d = _native.MatrixLevelsDesc()
        _native.check(_native.load().neo_hip_matrix_levels_info(self._h, ctypes.byref(d)))
        levels = [{"window": d.window[l], "first": d.first[l], "last": d.last[l], "splits": d.splits[l]}
                  for l in range(d.levels)]
        return {"enabled": bool(d.enabled), "head": d.head, "levels": levels, "ring_rows": d.ring_rows,
                "primed": bool(d.primed), "partial_bytes": d.partial_bytes, "head_bank_bytes": d.head_bank_bytes}

    # -- processing ---------------------------------------------------------
    def process(self, x, stream: int = 0):
        """x [I][n B] -> y [O][n B]: float32 ndarray (synchronous) or CUDA tensor (asynchronous on
        `stream`, default torch's current stream)."""
        lib = _native.load()
        if _is_torch(x) and x.is_cuda:
            import torch

            if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 2 or x.shape[0] != self.inputs:
                raise ValueError("x must be a contiguous float32 tensor [inputs][n * block_size]")
            n = x.shape[1]
            if n % self.block_size:
                raise ValueError("matrix convolvers take whole blocks")
            y = torch.empty((self.outputs, n), dtype=torch.float32, device=x.device)
            s = stream or torch.cuda.current_stream(x.device).cuda_stream
            _native.check(lib.neo_hip_matrix_process(self._h, ctypes.c_void_p(x.data_ptr()), n,
                                                     ctypes.c_void_p(y.data_ptr()), n, n // self.block_size, 1,
                                                     ctypes.c_void_p(s)))
            return y
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float32)))
        if a.shape[0] != self.inputs or a.shape[1] % self.block_size:
            raise ValueError("x must be [inputs][n * block_size]")
        n = a.shape[1]
        y = np.empty((self.outputs, n), dtype=np.float32)
        _native.check(lib.neo_hip_matrix_process(self._h, _ptr(a), n, _ptr(y), n, n // self.block_size, 0, None))
        return y

    def process_device(self, in_ptr: int, ld_in: int, out_ptr: int, ld_out: int, nblocks: int = 1,
                       stream: int = 0) -> None:
        """nblocks steps on device pointers: input i at in_ptr + 4 i ld_in, output o at out_ptr + 4 o ld_out."""
        _native.check(_native.load().neo_hip_matrix_process(self._h, ctypes.c_void_p(in_ptr), int(ld_in),
                                                            ctypes.c_void_p(out_ptr), int(ld_out), int(nblocks), 1,
                                                            ctypes.c_void_p(stream)))

    def info(self) -> dict:
        d = _native.MatrixDesc()
        _native.check(_native.load().neo_hip_matrix_info(self._h, ctypes.byref(d)))
        return {n: getattr(d, n) for n, _ in _native.MatrixDesc._fields_}

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.load().neo_hip_matrix_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def matrix_convolve(signal, ir, block_size: int, routes=None, method: str = "upols", device: int = 0,
                    batch: bool = False, offline: bool = False):
    """One shot: signal [I][n], ir [O][I][L] (routes None) or [nroutes][L] with routes a list of
    (out, in) and the output count max(out) + 1 -> [O][n padded to whole blocks]; the impulse is
    normalized over all routes, as dense_convolve normalizes over channels. batch=True runs the
    blocks in batched passes (MatrixConvolver.set_batch): the same results up to summation order.
    offline=True runs windows of 128 blocks as offline passes (MatrixConvolver.set_offline) and the
    rest of the call in batched passes: the same results up to rounding.
    A float32 CUDA tensor as signal (ir a tensor on the same device or an array) stays on the
    device and gives a tensor."""
    on_device = _is_torch(signal) and signal.is_cuda
    if on_device:
        import torch

        if signal.dtype != torch.float32 or signal.dim() != 2:
            raise ValueError("a device signal must be a float32 tensor [inputs][n]")
        x = signal.contiguous()
        a = ir if _is_torch(ir) and ir.is_cuda else np.asarray(ir, dtype=np.float32)
        device = x.device.index or 0
    else:
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(signal, dtype=np.float32)))
        a = np.asarray(ir, dtype=np.float32)
    I = x.shape[0]
    if routes is None:
        if a.ndim != 3 or a.shape[1] != I:
            raise ValueError("ir must be [outputs][inputs][L] without a route list")
        O = a.shape[0]
    else:
        routes = [(int(o), int(i)) for o, i in routes]
        O = max(o for o, _ in routes) + 1
    B = int(block_size)
    n = x.shape[1]
    pad = (-n) % B
    if pad and on_device:
        x = torch.nn.functional.pad(x, (0, pad)).contiguous()
    elif pad:
        x = np.concatenate([x, np.zeros((I, pad), np.float32)], axis=1)
    conv = MatrixConvolver(I, O, B, num_partitions(a.shape[-1], B), method=method, device=device)
    try:
        conv.set_impulse(a.contiguous() if _is_torch(a) else a, routes)
        if batch or offline:
            conv.set_batch(True)
        if offline:
            conv.set_offline(True)
        return conv.process(x)
    finally:
        conv.close()
