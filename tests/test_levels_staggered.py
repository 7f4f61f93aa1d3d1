"""Staggered level windows (neo_hip_upols_opts.windows = 2; levels_plan.hpp plan_levels_stag,
slice_part, prime_round), restated in float64 numpy from the plan export
(neo_hip_upols_stagger_plan) and checked against the direct block-axis convolution -- no GPU.

A level of window T >= 4 G, and the far level, is cut into T / G classes of channels. Class k is
computed whole in the background launch of every group g = k mod T / G, for its window that starts
at block s = (g + 2) G; the far level runs phase 2 of class k there and phase 1 two groups earlier.
The launch of group g is guaranteed only the FDL rows before (g - 1) G (odd g: it waits for the
blocks before the previous group) or (g - 2) G (even g: it only follows its odd predecessor), and
the blocks wait for it at the next even group. The replay runs every background role at a random
point between its launch's issue and the block that waits for it, asserts every FDL row a role
reads against the launch's guarantee, asserts that the buffer a role rewrites is no longer read by
any block that may still be in flight, and compares every output block with the direct sum.
Columns stand for channels here (a class is a range of columns)."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "neo-dsp_amd"))

FT, FN = 128, 256  # far window, transform length
K = 32             # columns (channels)


def splan(P, G, Kw=0, C=K, B=64):
    import neo

    return neo.convolution.stagger_plan(C, B, P, G, Kw)


class StagSim:
    """float64 replay of the staggered schedule; sp: the plan (stagger_plan), Kw: far window group"""

    def __init__(self, H, sp, Kw, seed=0, early=0):
        self.H, self.sp, self.Kw, self.G = H, sp, max(1, Kw), sp["step_group"]
        self.early = early  # mutation: the even groups' classes start their windows `early` groups sooner
        self.P = H.shape[0]
        self.R = max(self.P + 31, 512, FT * ((self.P + FT - 1) // FT + 2) + 1)  # upols.hip: the offline ring
        self.ring = np.zeros((self.R, K), complex)
        self.rowt = np.full(self.R, -10 ** 9)  # absolute block held by each ring row
        self.t, self.t0, self.n = 0, 0, -1
        self.rng = np.random.default_rng(seed)
        self.pending = []  # background launches in stream order: [roles left, due block n]
        self.slab = [np.zeros((2, T, K), complex) for T in sp["T"]]
        self.F, ns = sp["far_a"], sp["nseg"]
        if ns:
            seg = np.zeros((ns, FN, K), complex)
            for s in range(ns):
                lo = self.F + FT * s
                hi = min(self.P, lo + FT)
                seg[s, : hi - lo] = H[lo:hi]
            self.HF = np.fft.fft(seg, axis=1)
            self.XF = np.zeros((ns, FN, K), complex)
            self.ff = np.zeros((2, FT, K), complex)
            self.acc = np.zeros((self.Kw, FN, K), complex)

    # -- the classes: (first column, end column, group residue, window start mod T)
    def classes(self, key):
        return self.sp["classes"][key]

    def phi(self, T, k):
        """windows of class k start where (n + phi) mod T = 0 (stag_phi)"""
        return (-(k + 2 - (self.early if k % 2 == 0 else 0)) * self.G) % T

    # -- rows
    def rows(self, tabs, limit, strict=True):
        """ring rows of the absolute blocks tabs, all before `limit` (the launch's guarantee)"""
        tabs = np.asarray(tabs)
        assert tabs.max() < limit, (int(tabs.max()), limit)
        r = (self.w_of(tabs)) % self.R
        if strict:  # the row still holds that block (or nothing: before the stream began)
            held = self.rowt[r]
            assert np.all((held == tabs) | ((tabs < 0) & (held < 0))), "ring row overwritten"
        return r

    def w_of(self, tabs):
        return tabs  # ring row of absolute block t is t mod R (the write position starts at 0)

    # -- roles
    def toep(self, l, s_abs, k0, k1, buf, limit):
        T, a, b = self.sp["T"][l], self.sp["a"][l], self.sp["b"][l]
        ps = np.arange(a, b)
        for j in range(T):
            r = self.rows(s_abs + j - ps, limit)
            self.slab[l][buf, j, k0:k1] = (self.H[a:b, k0:k1] * self.ring[r, k0:k1]).sum(0)

    def cls(self, k):
        return (k // 4) % self.Kw

    def first(self, c):
        return 1 + ((c - 1) % self.Kw)

    def far1(self, wn, k0, k1, nfresh, mode=0, cls=0):
        ns, Kw = self.sp["nseg"], self.Kw
        for k in range(k0, k1):
            c = self.cls(k) if mode else 0
            if mode and c != cls:
                if self.first(c) <= wn:
                    continue
                nw = 1
            else:
                nw = Kw if mode else 1
            for j in range(nw):
                acc = np.zeros(FN, complex)
                for s in range(max(min(nfresh, ns), j + 1), ns):
                    acc += self.XF[(wn - (s - j) - 1) % ns, :, k] * self.HF[s, :, k]
                self.acc[(wn + j) % Kw, :, k] = acc

    def far2a(self, s_abs, wn, k0, k1, nfresh, limit):
        ns = self.sp["nseg"]
        for s in range(min(nfresh, ns)):
            tabs = s_abs - self.F - (s + 1) * FT + np.arange(FN)
            # rows that meet only the zero padding past P may have left the ring
            r = self.rows(tabs, limit, strict=False)
            need = tabs > s_abs - self.P  # block s + j meets rows after s + j - P
            held = self.rowt[r][need]
            assert np.all((held == tabs[need]) | ((tabs[need] < 0) & (held < 0))), "ring row overwritten"
            self.XF[(wn - s - 1) % ns, :, k0:k1] = np.fft.fft(self.ring[r, k0:k1], axis=0)

    def far2b(self, wn, k0, k1, nfresh, grp=False):
        ns, Kw = self.sp["nseg"], self.Kw
        acc = self.acc[wn % Kw, :, k0:k1].copy()
        for s in range(min(nfresh, ns)):
            acc += self.XF[(wn - s - 1) % ns, :, k0:k1] * self.HF[s, :, k0:k1]
        if grp:
            for k in range(k0, k1):
                c = self.cls(k)
                j = (wn - c) % Kw if wn >= self.first(c) else 0
                for s in range(1, min(j, ns - 1) + 1):
                    acc[:, k - k0] += self.XF[(wn - s - 1) % ns, :, k] * self.HF[s, :, k]
        self.ff[wn & 1, :, k0:k1] = np.fft.ifft(acc, axis=0)[FT:]

    # -- the schedule
    def bg_roles(self, n0, limit, replay=False):
        """the background launch of group g = n0 / G (slice_part); limit: rows before block n = limit"""
        sp, G, t0 = self.sp, self.G, self.t0
        g = n0 // G
        lead = 2 - (self.early if g % 2 == 0 else 0)
        out = []
        for l, T in enumerate(sp["T"]):
            if T < 2 * G:
                continue  # in the block launches
            if not sp["staggered"][l]:
                if replay:
                    continue
                m0 = n0 + self.aphi[l]  # aligned: part j of the next window, equal parts
                j, W = (m0 % T) // G, m0 // T + 1
                if j >= 1:
                    k0, k1 = (j - 1) * K // (T // G - 1), j * K // (T // G - 1)
                    out.append(lambda l=l, T=T, W=W, k0=k0, k1=k1: self.toep(
                        l, t0 + W * T - self.aphi[l], k0, k1, W & 1, t0 + limit))
                continue
            s = n0 + lead * G
            if s <= 0:
                continue
            k0, k1, k, _ = self.classes(l)[g % (T // G)]
            W = (s + self.phi(T, k)) // T
            if k1 > k0:
                # the buffer rewritten held window W - 2, whose blocks end at s - T: all of them done
                assert s - T <= limit or W < 2, "slab buffer still read by blocks in flight"
                out.append(lambda l=l, s=s, k0=k0, k1=k1, W=W: self.toep(l, t0 + s, k0, k1, W & 1, t0 + limit))
        if sp["nseg"]:
            nc, Kw = FT // G, self.Kw
            s1, s2 = n0 + 2 * G + lead * G, n0 + lead * G
            if s1 > 0:
                k0, k1, k, _ = self.classes("far")[(g + 2) % nc]
                W = (s1 + self.phi(FT, k)) // FT
                if k1 > k0:
                    out.append(lambda k0=k0, k1=k1, W=W: self.far1(W, k0, k1, 1, 0 if Kw == 1 else (2 if W < Kw else 1),
                                                                  W % Kw))
            if s2 > 0:
                k0, k1, k, _ = self.classes("far")[g % nc]
                W = (s2 + self.phi(FT, k)) // FT
                if k1 > k0:
                    assert s2 - FT <= limit or W < 2, "far field buffer still read by blocks in flight"

                    def far2c(k0=k0, k1=k1, W=W, s2=s2):
                        self.far2a(t0 + s2, W, k0, k1, 1, t0 + limit)
                        self.far2b(W, k0, k1, 1, Kw > 1)
                    out.append(far2c)
        return [out[i] for i in self.rng.permutation(len(out))]

    def block_roles(self, n):
        """the levels of T < 2 G, 1 / T of the next window per step (block_levels)"""
        sp, out, t0 = self.sp, [], self.t0
        for l, T in enumerate(sp["T"]):
            if T >= 2 * self.G:
                break
            st, W = n % T, n // T + 1
            k0, k1 = st * K // T, (st + 1) * K // T
            if k1 > k0:
                out.append(lambda l=l, T=T, W=W, k0=k0, k1=k1: self.toep(l, t0 + W * T, k0, k1, W & 1, t0 + n + 1))
        return out

    def join(self):
        while self.pending:
            for r in self.pending.pop(0)[0]:
                r()

    def plain(self, x):
        self.join()
        self.ring[self.t % self.R] = x
        self.rowt[self.t % self.R] = self.t
        y = (self.H * self.ring[(self.t - np.arange(self.P)) % self.R]).sum(0)
        self.t += 1
        self.n = -1
        return y

    def prime(self):
        """prime_round (levels_plan.hpp): window 0 of every class began phi steps ago; then the
        launches of the groups -3 .. -1 as they would have run"""
        self.join()
        sp, G, t0 = self.sp, self.G, self.t
        self.t0 = t0
        self.aphi = [T // 2 if (not sp["staggered"][l]) and 4 * G <= T <= 32 else 0 for l, T in enumerate(sp["T"])]
        for l, T in enumerate(sp["T"]):
            if sp["staggered"][l]:
                for k0, k1, k, off in self.classes(l):
                    assert self.early or (T - self.phi(T, k)) % T == off  # the export's window offsets
                    if k1 > k0:
                        self.toep(l, t0 - self.phi(T, k), k0, k1, 0, t0)
            else:
                self.toep(l, t0 - self.aphi[l], 0, K, 0, t0)
                if self.aphi[l]:
                    self.toep(l, t0 + T - self.aphi[l], 0, K, 1, t0)
        if sp["nseg"]:
            ns = sp["nseg"]
            for k0, k1, k, off in self.classes("far"):
                assert self.early or (FT - self.phi(FT, k)) % FT == off
                if k1 > k0:
                    self.far1(0, k0, k1, ns)
                    self.far2a(t0 - self.phi(FT, k), 0, k0, k1, ns, t0)
                    self.far2b(0, k0, k1, ns)
        for g in (-3, -2, -1):
            for r in self.bg_roles(g * G, 0, replay=True):
                r()
        self.n = 0

    def step(self, x):
        if self.n < 0:
            self.prime()
        n, sp, G, t0 = self.n, self.sp, self.G, self.t0
        y = [None]

        def block_read():
            a0 = sp["a0"]
            r = (self.H[1:a0] * self.ring[(self.t - np.arange(1, a0)) % self.R]).sum(0)
            for l, T in enumerate(sp["T"]):
                if sp["staggered"][l]:
                    for k0, k1, k, _ in self.classes(l):
                        m = n + self.phi(T, k)
                        r[k0:k1] += self.slab[l][(m // T) & 1, m % T, k0:k1]
                else:
                    m = n + self.aphi[l]
                    r = r + self.slab[l][(m // T) & 1, m % T]
            if sp["nseg"]:
                for k0, k1, k, _ in self.classes("far"):
                    m = n + self.phi(FT, k)
                    r[k0:k1] += self.ff[(m // FT) & 1, m % FT, k0:k1]
            y[0] = r + self.H[0] * x

        def block_write():
            self.ring[self.t % self.R] = x
            self.rowt[self.t % self.R] = self.t

        jobs = self.block_roles(n) + [block_read, block_write]
        jobs = [jobs[i] for i in self.rng.permutation(len(jobs))]
        if n % G == 0:
            odd = (n // G) & 1
            # odd groups wait for the blocks before n - G, even ones only follow their predecessor
            self.pending.append([self.bg_roles(n, n - G if odd else n - 2 * G), n + G if odd else n + 2 * G])
        while self.pending and self.pending[0][1] <= n:  # the even group's block waits
            for r in self.pending.pop(0)[0]:
                r()
        bgq = [r for p in self.pending for r in p[0]]
        k = int(self.rng.integers(0, len(bgq) + 1))
        slots = set(self.rng.choice(len(jobs) + k, size=k, replace=False).tolist()) if k else set()
        it, jt = iter(bgq[:k]), iter(jobs)
        jobs = [next(it) if i in slots else next(jt) for i in range(len(jobs) + k)]
        left = k
        while left:
            p = self.pending[0]
            d = min(left, len(p[0]))
            del p[0][:d]
            left -= d
            if not p[0]:
                self.pending.pop(0)
        for j in jobs:
            j()
        self.t += 1
        self.n = n + 1
        return y[0]


def run(P, G, Kw, sp=None, early=0, seed=None, nb=None):
    sp = sp or splan(P, G, Kw)
    seed = P + 10 * G + Kw if seed is None else seed
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((P, K)) + 1j * rng.standard_normal((P, K))
    Kw_eff = Kw if sp["nseg"] >= 2 else 1
    sim = StagSim(H, sp, Kw_eff, seed=seed, early=early)
    nb = nb or (2 * P + 3 * FT + 60)  # every class's first regular window, the ring's wrap (R < 2 P + 300)
    X = rng.standard_normal((nb, K)) + 1j * rng.standard_normal((nb, K))
    worst = 0.0
    for t in range(nb):
        # history before the levels start, and plain steps in mid-stream (join + re-prime), off the group grid
        y = sim.plain(X[t]) if (t < 37 or nb // 2 + 1 <= t < nb // 2 + 4) else sim.step(X[t])
        m = min(P, t + 1)
        ref = (H[:m] * X[t - np.arange(m)]).sum(0)
        worst = max(worst, float(np.abs(y - ref).max() / (np.abs(ref).max() + 1e-300)))
    return worst


CASES = [(60, 4, 1), (150, 4, 1), (300, 4, 2), (450, 4, 3), (700, 4, 2), (938, 4, 3), (1100, 4, 4), (1875, 4, 4),
         (300, 2, 1), (700, 2, 3), (938, 2, 2), (150, 8, 1), (450, 8, 2), (1100, 8, 4), (938, 8, 1), (700, 8, 4)]


@pytest.mark.parametrize("P,G,Kw", CASES)
def test_staggered_schedule_matches_direct(P, G, Kw):
    assert run(P, G, Kw) < 1e-12


@pytest.mark.parametrize("P,G,Kw", [(450, 4, 3), (938, 4, 2), (700, 2, 1), (1100, 8, 4)])
def test_staggered_schedule_arbitrary_cuts(P, G, Kw):
    """any class cuts give the same outputs, classes without a channel included"""
    sp = splan(P, G, Kw)
    rng = np.random.default_rng(P)
    for key, cl in sp["classes"].items():
        n = len(cl)
        cuts = sorted(rng.integers(0, K + 1, size=n - 1).tolist())
        if n > 3:
            cuts[1] = cuts[0]  # an empty class
            cuts[-1] = K      # and an empty last one
        cuts = [0] + sorted(cuts) + [K]
        sp["classes"][key] = [(cuts[j], cuts[j + 1], cl[j][2], cl[j][3]) for j in range(n)]
    assert run(P, G, Kw, sp=sp) < 1e-12


@pytest.mark.parametrize("P,G", [(450, 4), (938, 4), (700, 2)])
def test_band_one_partition_earlier_fails(P, G):
    """the rule is tight: a staggered band starting one partition earlier reads a row past the
    launch's guarantee"""
    sp = splan(P, G, 2)
    l = sp["staggered"].index(True)
    sp["a"][l] -= 1
    sp["b"][l - 1] -= 1
    with pytest.raises(AssertionError):
        run(P, G, 2, sp=sp, nb=400)


@pytest.mark.parametrize("P,G", [(450, 4), (1875, 4), (1875, 2)])
def test_far_band_one_partition_earlier_fails(P, G):
    """where the far level starts at its earliest, 128 + 4 G (elsewhere the plan puts it later to
    save a segment, with slack)"""
    sp = splan(P, G, 2)
    assert sp["far_a"] == FT + 4 * G
    sp["far_a"] -= 1
    sp["b"][-1] -= 1
    with pytest.raises(AssertionError):
        run(P, G, 2, sp=sp, nb=600)


@pytest.mark.parametrize("P,G", [(450, 4), (938, 4)])
def test_window_one_group_earlier_fails(P, G):
    """a class of an even group may not own the window starting at (g + 1) G: the blocks there do
    not wait for its launch"""
    sp = splan(P, G, 2)
    bad = False
    try:
        bad = run(P, G, 2, sp=sp, early=1, nb=500) > 1e-9
    except AssertionError:
        bad = True
    assert bad


# -- the plan --------------------------------------------------------------------------------

def bench_rows(lp, far_a, nseg, Kw):
    """rows of 8 B per channel column and step by bench.py's algorithmic_bytes formulas: the block
    role 23, a Toeplitz level (2 (b - a) + 2 T - 1) / T, the stored far level"""
    rows = 23.0
    for T, a, b in zip(lp["T"], lp["a"], lp["b"]):
        rows += (2.0 * (b - a) + 2 * T - 1) / T
    if nseg:
        rows += (256.0 * 2 * (nseg - 1) / Kw + 256 + 256.0 * (3 + Kw - 1) + 128 + 256) / FT
    return rows


@pytest.mark.parametrize("G", [2, 4, 8])
def test_staggered_plan_bands(G):
    for P in [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 255, 256, 257, 383, 384, 385, 938, 1875, 4000]:
        sp = splan(P, G)
        cover = [(0, sp["a0"])] + list(zip(sp["a"], sp["b"]))
        if sp["nseg"]:
            F = sp["far_a"]
            cover.append((F, F + FT * sp["nseg"]))
            assert F + FT * (sp["nseg"] - 1) < P <= F + FT * sp["nseg"]
            assert FT + 4 * G <= F <= FT + 4 * G + 127
        for (lo, hi), (lo2, _) in zip(cover, cover[1:]):
            assert hi == lo2, (P, cover)
        assert cover[-1][1] >= P
        for T, a, b, st in zip(sp["T"], sp["a"], sp["b"], sp["staggered"]):
            assert a >= (T + 4 * G if st else 2 * T) and st == (T >= 4 * G)
            assert b - a <= (192 if T == 32 else 2 * T)  # the kernels' tiles
        for key, cl in sp["classes"].items():
            T = FT if key == "far" else sp["T"][key]
            assert len(cl) == T // G and cl[0][0] == 0 and cl[-1][1] == K
            assert all(c[1] == d[0] for c, d in zip(cl, cl[1:]))
            assert [c[3] for c in cl] == [((k + 2) * G) % T for k in range(len(cl))]


def test_staggered_plan_bytes_and_balance():
    import neo

    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    import bench

    for C, B, P in [(2048, 512, 938), (256, 512, 938), (256, 256, 1875)]:
        sp = neo.convolution.stagger_plan(C, B, P, 4, 0)
        loads = np.array(sp["loads"])
        assert len(loads) == 32 and abs(loads / loads.mean() - 1).max() < 0.01, loads / loads.mean()
    sp = neo.convolution.stagger_plan(2048, 512, 938, 4, 0)
    lp = neo.convolution.level_plan(938)
    Kw = bench.far_group(lp["nseg"], 2048 * 512 // 16)
    aligned = bench_rows(lp, 256, lp["nseg"], Kw)
    Ks = bench.far_group(sp["nseg"], 2048 * 512 // 16)
    stag = bench_rows(sp, sp["far_a"], sp["nseg"], Ks)
    assert abs(aligned - 76.2) < 0.2  # the figure of DESIGN 5 (639.2 MB at c5full)
    assert stag <= 0.92 * aligned, (stag, aligned)


def test_aligned_exports_unchanged():
    import neo

    lp = neo.convolution.level_plan(938)
    assert lp == {"a0": 8, "T": [4, 8, 16, 32], "a": [8, 16, 32, 64], "b": [16, 32, 64, 256], "nseg": 6}
    assert neo.convolution.level_plan(300) == {"a0": 8, "T": [4, 8, 16, 32], "a": [8, 16, 32, 64],
                                                "b": [16, 32, 64, 256], "nseg": 1}
    # the whole aligned part plan as the library gave it before the staggered plan was added
    pp = neo.convolution.part_plan(4, 256, 300, 4)
    assert pp["phi"] == [0, 0, 8, 16] and pp["cycle"] == 32
    assert pp["cuts"] == {
        1: [[0, 64]] * 16,
        2: [[0, 4, 64, 64], [0, 10, 54, 64], [0, 0, 64, 64], [0, 10, 54, 64], [0, 0, 64, 64], [0, 10, 54, 64],
              [0, 0, 60, 64], [0, 0, 52, 64]],
        3: [[0, 16, 46, 58, 70, 82, 112, 128]] * 3 + [[0, 11, 37, 51, 72, 92, 117, 128]]}
    assert pp["loads"] == [
        1233088.0, 1201408.0, 1223104.0, 1141568.0, 1237504.0, 1203200.0, 1218688.0, 1210368.0, 1238784.0, 1210368.0,
        1218688.0, 1203200.0, 1138688.0, 1203200.0, 1218688.0, 1210368.0, 1238784.0, 1210368.0, 1218688.0, 1203200.0,
        1138688.0, 1203200.0, 1218688.0, 1210368.0, 1238784.0, 1210368.0, 1218688.0, 1203200.0, 1122816.0, 1256256.0,
        1137024.0, 1227904.0]
