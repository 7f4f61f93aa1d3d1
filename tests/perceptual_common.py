"""What tests/test_perceptual.py and tests/test_perceptual_gpu.py share: the shapes, the inputs
and the perceptual predicate of include/neo_hip.h (neo_hip_perceptual) restated in numpy float64.

The restatement is independent of the library: it evaluates the A-weighting formula itself, takes
the per-channel maximum itself and never calls into neo. Comparisons against it allow a
disagreement only for elements whose float64 level lies within DELTA of the deciding value (the
threshold for a mask, an integer for a histogram bucket), and cap how many such elements there
may be, so that a quirk of an input cannot turn into leniency.

DELTA = 1e-3 dB: levels are at most 150 in magnitude, float32 carries 2^-23 relative (1.8e-5 at
150), and the handful of float operations of the definition (a product, a sum, log10, two more
products, a sum) stay below 1e-4 in all; 1e-3 leaves a factor ten.

DELTA_HIST = 2.5e-4 dB for the histogram buckets. There EVERY integer is a deciding value, so of
levels spread over many dB a fraction 2 delta lies within delta of one: 0.2 % at 1e-3, twice the
cap of 0.1 % whatever the code under test does. The band is therefore narrower for histograms
(which asks more of the code, not less): 2 DELTA_HIST = 0.05 %, half the cap, and still five
times the float error budget (log10f at 2 ulp of |log10 x| <= 7.2 is 1e-6, times 20 times 0.5 is
1e-5; the argument's few ulp 3e-6; the rounded weight 8e-6; the last sum at 150 8e-6: 5e-5)."""
import numpy as np

#        C  B     P
SHAPES = [(2, 16, 7), (1, 32, 37), (3, 128, 9), (2, 512, 70), (1, 1024, 20), (1, 4096, 3)]
BLOCKS = {(2, 16, 7): 60, (1, 32, 37): 80, (3, 128, 9): 50, (2, 512, 70): 120, (1, 1024, 20): 60, (1, 4096, 3): 40}
THRESHOLDS = (-20.0, -40.0, -60.0, -80.0)
WEIGHTINGS = ("none", "a")
SAMPLE_RATE = 48000.0
DELTA = 1e-3
DELTA_HIST = 2.5e-4
CAP = 1e-3  # at most 0.1 % of the elements may lie in a band
BUCKETS = 144


def low_bins(B):
    return (0, 2, B)


def impulse(C, B, P):
    """Exponentially decaying noise [C][B P] float32 (60 dB over its length). With C >= 2 channel 1
    is scaled by 1e-3 (a global maximum would give another mask than the per-channel one); at
    (3, 128, 9) channel 2 is all zero and channel 0 ends after 5 partitions (zero rows: the floor
    branch)."""
    rng = np.random.default_rng(7000 + 13 * B + P)
    L = B * P
    ir = rng.standard_normal((C, L)) * 10.0 ** (-3.0 * np.arange(L) / L)
    if C >= 2:
        ir[1] *= 1e-3
    if (C, B, P) == (3, 128, 9):
        ir[2] = 0.0
        ir[0, 5 * B:] = 0.0
    return ir.astype(np.float32)


def host_spectra(ir, B):
    """uniform_partition with numpy.fft: rfft of every B-sample partition zero-padded to 2 B."""
    C, L = ir.shape
    P = L // B
    return np.fft.rfft(ir.reshape(C, P, B).astype(np.float64), n=2 * B, axis=2).astype(np.complex64)


def a_weighting64(f):
    c = np.array([12194.217, 20.598997, 107.65265, 737.86223], np.float64) ** 2
    f2 = np.asarray(f, np.float64) ** 2
    with np.errstate(divide="ignore"):
        return 2.0 + 20.0 * (np.log10(c[0]) + 2.0 * np.log10(f2) - np.log10(f2 + c[0]) - np.log10(f2 + c[1])
                             - 0.5 * np.log10(f2 + c[2]) - 0.5 * np.log10(f2 + c[3]))


def weights64(B, sample_rate, low, weighting):
    k = np.arange(B + 1)
    w = a_weighting64(k * sample_rate / (2.0 * B)) if weighting == "a" else np.zeros(B + 1)
    w = np.array(w, np.float64)
    w[:low] = 100.0
    return w


def levels64(parts, w):
    """dB [C][P][B+1] float64 of complex64 spectra, and which elements take a value that every
    arithmetic computes without rounding (the floor -72 plus an integer weight)."""
    re, im = parts.real.astype(np.float64), parts.imag.astype(np.float64)
    power = re * re + im * im
    m = power.max(axis=(1, 2), keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = power * (1.0 / m)
        raw = 20.0 * np.log10(x)
    pos = x > 0  # false for 0 and for NaN (an all-zero channel's 0 * inf)
    lv = np.where(pos, np.maximum(-144.0, np.where(pos, raw, 0.0)), -144.0) * 0.5 + w
    on_floor = ~pos | (raw < -144.0 - DELTA)
    exact = on_floor & (w == np.round(w))
    return lv, exact


def tile_levels64(lv, exact):
    C, P, bins = lv.shape
    B = bins - 1
    t = lv[:, :, :B].reshape(C, P, B // 16, 16).max(axis=3)
    t[:, :, 0] = np.maximum(t[:, :, 0], lv[:, :, B])
    # a tile's level is exact if no inexact column comes within DELTA of its maximum
    cols = np.where(exact, -np.inf, lv)
    ti = cols[:, :, :B].reshape(C, P, B // 16, 16).max(axis=3)
    ti[:, :, 0] = np.maximum(ti[:, :, 0], cols[:, :, B])
    return t, ti < t - DELTA


def bucket(lv):
    v = np.maximum(0.0, -np.asarray(lv, np.float64))
    return np.minimum(BUCKETS - 1, np.floor(np.minimum(v, 1e6))).astype(np.int64)


def hist_bounds(lv, exact):
    """Per channel the counts every correct histogram of the levels lv [C][...] lies between, and
    the band elements (inexact levels within DELTA_HIST of a bucket boundary)."""
    C = lv.shape[0]
    lo_b, hi_b = bucket(lv + DELTA_HIST), bucket(lv - DELTA_HIST)  # a higher level is a lower bucket
    band = (lo_b != hi_b) & ~exact
    lower = np.zeros((C, BUCKETS), np.int64)
    upper = np.zeros((C, BUCKETS), np.int64)
    sure = bucket(lv)
    for c in range(C):
        lower[c] = np.bincount(sure[c][~band[c]].ravel(), minlength=BUCKETS)
        upper[c] = lower[c] + np.bincount(lo_b[c][band[c]].ravel(), minlength=BUCKETS) \
            + np.bincount(hi_b[c][band[c]].ravel(), minlength=BUCKETS)
    return lower, upper, band


def check_mask(got, lv, exact, theta, what):
    """got may differ from lv > theta only inside the band, and the band holds at most CAP."""
    want = lv > theta
    band = (np.abs(lv - theta) <= DELTA) & ~exact
    nband = int(band.sum())
    bad = (np.asarray(got, bool) != want) & ~band
    print(f"{what}: kept {int(want.sum())} of {want.size}, band {nband}, disagree {int((got != want).sum())}")
    assert nband <= CAP * want.size, (what, nband, want.size)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    return nband


def check_hist(got, lv, exact, total_per_channel, nbins, what):
    """got [C][144] lies between the bounds of hist_bounds, sums to total_per_channel, and the band
    (of columns or of tiles) holds at most CAP of the case's nbins columns."""
    lower, upper, band = hist_bounds(lv, exact)
    got = np.asarray(got)
    nband = int(band.sum())
    print(f"{what}: band {nband} of {lv.size}")
    assert np.array_equal(got.sum(axis=1), np.full(lv.shape[0], total_per_channel)), what
    assert nband <= CAP * nbins, (what, nband, nbins)
    assert np.all(got >= lower) and np.all(got <= upper), (what, np.argwhere((got < lower) | (got > upper))[:5].tolist())
    return nband
