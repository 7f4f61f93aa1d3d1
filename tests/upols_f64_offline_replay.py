"""A float64 numpy replay of the offline windows of the double-precision UPOLS / UPOLA convolvers
(csrc/upols_f64_offline.hip), written from the rule and shared by tests/test_upols_f64_offline.py (the
replay against tests/upols_f64_truth.py on the CPU) and tests/test_upols_f64_offline_gpu.py (the shapes
and call sequences). Not the device code: numpy's fft along the block axis, unpacked rows of B + 1
bins, one Python loop per launch. The plain step and the batched pass are the batch replay's.

A window is 128 consecutive blocks at write position w. Block j's spectrum is the fresh row N[j] of a
scratch. Window row e is N[e] for e >= 0, the ring row (w + e) mod P as it stood before the pass for
-P < e < 0, and zero for e <= -P. With nseg = ceil(P / 128), per channel and bin
    Y[j] = sample 128 + j of IDFT256( sum_{q < nseg} DFT256(rows -128 (q+1) .. -128 q + 127) HF[q] )
HF[q] = DFT256 along the partitions of filter rows 128 q .. 128 q + 127, zero past P, zero padded to
256. The last min(128, P) fresh rows then enter the ring, w moves on by 128 mod P."""
import numpy as np

import upols_f64_batch_replay as RB

W, F = 128, 256
SCRATCH, RING, ZERO = 0, 1, 2

# (C, B, P, blocks): the GPU tests' value shapes
VALUE_SHAPES = [(1, 16, 1, 128), (3, 16, 3, 256), (3, 16, 127, 256), (1, 16, 128, 256), (3, 16, 129, 384),
                (3, 128, 200, 384), (1, 512, 129, 256), (3, 16, 257, 640), (1, 4096, 3, 128)]


def segments(P):
    return -(-P // W)


def offline_src(e, w, P):
    """(kind, row) of window row e: the definition the index function of the plan header must equal."""
    if e >= 0:
        return (SCRATCH, e)
    if e <= -P:
        return (ZERO, 0)
    return (RING, (w + e) % P)


def plan_rule(C, B, P, ola):
    """The byte counts of the plan, restated: rows of 16 B bytes per channel."""
    nseg, row = segments(P), 16 * C * B
    tails = 8 * C * W * B if ola else 0
    loaded = W + min(W * nseg, P - 1)  # the fresh rows and the ring rows that are not zero
    return {"nseg": nseg, "spectra_bytes": row * nseg * F, "scratch_bytes": row * W, "y_bytes": row * W,
            "tail_bytes": tails, "extra_bytes": 2 * row * W + tails,
            "pass_bytes": row * (W + loaded + F * nseg + 2 * W + 2 * min(W, P)) + 8 * C * B * (W * (6 if ola else 3) + 1)}


class Replay(RB.Replay):
    """The batch replay's handle (ring of P rows, w, prev / tail; plain step, batched pass) with the
    window pass as a third way on."""

    def run_window(self, x):
        B, P, w, C = self.B, self.P, self.w, self.C
        assert self.ring.shape[1] == P
        blk = [x[:, j * B:(j + 1) * B] for j in range(W)]
        # launch 1: the scratch of fresh rows; the ring is not written
        N = [self._window(self.prev if j == 0 else blk[j - 1], blk[j]) for j in range(W)]
        zero = np.zeros((C, B + 1), dtype=np.complex128)

        def row(e):
            kind, r = offline_src(e, w, P)
            return zero if kind == ZERO else N[r] if kind == SCRATCH else self.ring[:, r]

        # launch 2: the pairs from the newest back, the products in the order q = 0, 1, ..
        acc = np.zeros((C, F, B + 1), dtype=np.complex128)
        for q in range(segments(P)):
            pair = np.stack([row(e) for e in range(-W * (q + 1), -W * q + W)], axis=1)
            seg = np.zeros((C, F, B + 1), dtype=np.complex128)
            k = min(P, W * (q + 1)) - W * q
            seg[:, :k] = self.H[:, W * q:W * q + k]
            acc += np.fft.fft(pair, axis=1) * np.fft.fft(seg, axis=1)
        Y = np.fft.ifft(acc, axis=1)[:, W:]
        # launch 3: c2r per block, the commit after the products, prev
        out, tails = np.empty((C, W * B)), []
        for j in range(W):
            y = np.fft.irfft(Y[:, j], n=2 * B, axis=-1)
            out[:, j * B:(j + 1) * B] = y[:, :B] if self.ola else y[:, B:]
            tails.append(y[:, B:].copy())
        written = []
        for j in range(W):
            r = RB.commit_row(j, W, P, w)
            if r >= 0:
                self.ring[:, r] = N[j]
                written.append(r)
        assert len(set(written)) == len(written) == min(W, P)
        # launch 4 (overlap-add): the tail chain
        if self.ola:
            for j in range(W):
                out[:, j * B:(j + 1) * B] += self.prev if j == 0 else tails[j - 1]
            self.prev = tails[-1]
        else:
            self.prev = blk[-1].copy()
        self.w = (w + W) % P
        return out

    def process(self, x, T=1, rows=None, offline=True):
        """A process call: whole windows while 128 blocks are left, then the batch replay's call
        (passes of T blocks if T > 1, then plain steps)."""
        B = self.B
        nb = x.shape[1] // B
        y = np.empty_like(x)
        done = 0
        while offline and done + W <= nb:
            y[:, done * B:(done + W) * B] = self.run_window(x[:, done * B:(done + W) * B])
            done += W
        if done < nb:
            y[:, done * B:] = super().process(x[:, done * B:], T, rows if rows is not None else self.P)
        return y
