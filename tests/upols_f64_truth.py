"""float64 numpy truth for the double-precision UPOLS / UPOLA convolvers, stated two ways, and the
problems both test files share (tests/test_upols_f64.py shows on the CPU that the two statements
agree within 1e-13 at every shape; tests/test_upols_f64_gpu.py holds the device to 1e-12 against them).

  blockwise   the algorithm block by block with np.fft.rfft / irfft: 2B window (overlap-save: slide,
              last B samples; overlap-add: block | zeros, first B + tail), delay line of P spectra,
              Y = sum_p H[p] X[(w - p) mod P], irfft
  whole       np.convolve of each channel's whole signal with its impulse response, first n samples
"""
import numpy as np

TOL = 1e-12          # the project's f64 bar, peak-normalised (tests/test_fft_gpu.py)
TRUTH_AGREE = 1e-13  # the two numpy statements against each other

# values against truth: B x P x C, P + 5 blocks so the ring of P rows wraps
VALUE_SHAPES = [(C, B, P) for B in (16, 128, 512) for P in (1, 3, 9, 70) for C in (1, 3)]
BIG_SHAPE = (1, 4096, 3)  # 6 blocks
BIG_BLOCKS = 6


def nblocks(P):
    return P + 5


def partition(ir, B):
    """[C][L] float64 -> [C][P][B+1] complex128: rfft_2B of each zero-padded B-sample partition."""
    ir = np.atleast_2d(np.asarray(ir, dtype=np.float64))
    C, L = ir.shape
    P = max(1, -(-L // B))
    pad = np.zeros((C, P * B))
    pad[:, :L] = ir
    seg = np.zeros((C, P, 2 * B))
    seg[:, :, :B] = pad.reshape(C, P, B)
    return np.fft.rfft(seg, axis=-1)


def normalize(ir):
    """A normalized copy: every channel scaled by min_c 1/sqrt(sum ir[c]^2) (zero energy counts as 1)."""
    ir = np.atleast_2d(np.asarray(ir, dtype=np.float64))
    e = (ir * ir).sum(axis=1)
    f = np.where(e == 0.0, 1.0, 1.0 / np.sqrt(np.where(e == 0.0, 1.0, e)))
    return ir * f.min()


def blockwise(x, H, method="upols"):
    """x [C][nb B] float64 through the filter H [C][P][B+1] complex128, block by block."""
    C, P, bins = H.shape
    B = bins - 1
    nb = x.shape[1] // B
    assert x.shape == (C, nb * B)
    fdl = np.zeros((C, P, bins), dtype=np.complex128)
    window = np.zeros((C, 2 * B))
    tail = np.zeros((C, B))
    y = np.empty_like(x)
    w = 0
    for t in range(nb):
        blk = x[:, t * B:(t + 1) * B]
        if method == "upols":
            window[:, :B] = window[:, B:]
            window[:, B:] = blk
        else:
            window[:, :B] = blk
            window[:, B:] = 0.0
        fdl[:, w] = np.fft.rfft(window, axis=-1)
        acc = np.zeros((C, bins), dtype=np.complex128)
        for p in range(P):
            acc += H[:, p] * fdl[:, (w - p) % P]
        out = np.fft.irfft(acc, n=2 * B, axis=-1)
        if method == "upols":
            y[:, t * B:(t + 1) * B] = out[:, B:]
        else:
            y[:, t * B:(t + 1) * B] = out[:, :B] + tail
            tail = out[:, B:].copy()
        w = (w + 1) % P
    return y


def whole(x, ir):
    """np.convolve of every channel's whole signal with its impulse response, first n samples."""
    return np.stack([np.convolve(x[c], ir[c])[:x.shape[1]] for c in range(x.shape[0])])


_cache = {}


def problem(C, B, P, nb=None):
    """(ir [C][L], H [C][P][B+1], x [C][nb B]) of a shape, made once and read-only; L = P B - 3 (> 0
    for every B >= 16), so the last partition is zero-padded. One channel is channel 0 of the
    three-channel problem of the same (B, P): the whole-signal truth is computed once per (B, P)."""
    nb = nblocks(P) if nb is None else nb
    key = (B, P, nb)
    if key not in _cache:
        rng = np.random.default_rng(6400 + 131 * B + P)
        ir = rng.standard_normal((3, P * B - 3))
        x = rng.standard_normal((3, nb * B))
        H = partition(ir, B)
        for a in (ir, x, H):
            a.setflags(write=False)
        _cache[key] = (ir, H, x)
    ir, H, x = _cache[key]
    return ir[:C], H[:C], x[:C]


def truth(C, B, P, method, nb=None, statement="blockwise"):
    """The expected output [C][nb B] of problem(C, B, P, nb), made once and read-only."""
    nb = nblocks(P) if nb is None else nb
    key = (B, P, nb, statement, method if statement == "blockwise" else "")
    if key not in _cache:
        ir, H, x = problem(3, B, P, nb)
        y = blockwise(x, H, method) if statement == "blockwise" else whole(x, ir)
        y.setflags(write=False)
        _cache[key] = y
    return _cache[key][:C]


def peak_err(y, ref):
    return float(np.abs(np.asarray(y) - np.asarray(ref)).max()) / max(float(np.abs(ref).max()), 1e-300)


def float_rule(C, P, split_workgroups):
    """The float plain step's two-launch split (upols_plan.hpp): (S, rows)."""
    target = split_workgroups or 1024
    min_rows = 1 if split_workgroups else 8
    S = max(1, min(-(-target // C), -(-P // min_rows), 64))
    rows = -(-P // S)
    return -(-P // rows), rows


def forced_split(C):
    """split_workgroups that asks for four splits per channel: P = 9 then gives rows 3 (three equal
    splits after the rule's second step), P = 70 rows 18, 18, 18, 16."""
    return 4 * C
