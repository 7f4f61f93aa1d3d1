"""A float64 numpy replay of the batched passes of the double-precision UPOLS / UPOLA convolvers
(csrc/upols_f64_batch.hip), written from the definition of a pass and shared by
tests/test_upols_f64_batch.py (the replay against tests/upols_f64_truth.py on the CPU) and
tests/test_upols_f64_batch_gpu.py (the call sequence). Not the device code: numpy's rfft / irfft,
unpacked rows of B + 1 bins, one Python loop per launch.

A pass is T blocks at write position w. Block j's spectrum is the fresh row N[j] of a scratch; block
j at partition p takes window row e = j - p: N[e] when e >= 0, else ring row (w + e) mod P as it
stood before the pass. The ring takes the last min(T, P) fresh rows after the MAC."""
import numpy as np

import upols_f64_truth as T64


def window_src(e, w, P):
    """(scratch, row) of window row e: the definition the index function of the plan header must equal."""
    return (1, e) if e >= 0 else (0, (w + e) % P)


def commit_row(j, T, P, w):
    """The ring row block j of a pass commits its fresh row to, -1 for none: the last min(T, P) blocks."""
    return (w + j) % P if j >= T - min(T, P) else -1


def batch_rule(C, B, P, T, split_workgroups=0):
    """(S, rows) of a pass's MAC: an explicit workgroup target takes the plain step's splits as they
    are; automatic: ~1024 workgroups over C x S x ceil(B / 256), >= T rows per split, <= 64 splits."""
    if split_workgroups:
        return T64.float_rule(C, P, split_workgroups)
    per_split = C * -(-B // 256)
    S = max(1, min(-(-1024 // per_split), 64, P // T))
    rows = -(-P // S)
    return -(-P // rows), rows


class Replay:
    """The state of one handle (ring, write position, previous block, tail) and its two ways on."""

    def __init__(self, H, method):
        self.H, self.ola = H, method == "upola"
        self.C, self.P, bins = H.shape
        self.B = bins - 1
        self.ring = np.zeros(H.shape, dtype=np.complex128)
        self.prev = np.zeros((self.C, self.B))  # overlap-save: the previous block; overlap-add: the tail
        self.w = 0

    def _window(self, before, blk):
        win = np.zeros((self.C, 2 * self.B))
        if self.ola:
            win[:, :self.B] = blk
        else:
            win[:, :self.B], win[:, self.B:] = before, blk
        return np.fft.rfft(win, axis=-1)

    def step(self, blk):
        """One plain step, as tests/upols_f64_truth.py blockwise states it."""
        B, P = self.B, self.P
        self.ring[:, self.w] = self._window(self.prev, blk)
        acc = np.zeros((self.C, B + 1), dtype=np.complex128)
        for p in range(P):
            acc += self.H[:, p] * self.ring[:, (self.w - p) % P]
        y = np.fft.irfft(acc, n=2 * B, axis=-1)
        if self.ola:
            out, self.prev = y[:, :B] + self.prev, y[:, B:].copy()
        else:
            out, self.prev = y[:, B:], blk.copy()
        self.w = (self.w + 1) % P
        return out

    def run_pass(self, x, T, rows):
        """T blocks x [C][T B] as one pass whose MAC splits hold `rows` partitions."""
        B, P, w = self.B, self.P, self.w
        blk = [x[:, j * B:(j + 1) * B] for j in range(T)]
        # launch 1: the scratch of fresh rows; the ring is not written
        N = [self._window(self.prev if j == 0 else blk[j - 1], blk[j]) for j in range(T)]

        def row(e):
            scratch, r = window_src(e, w, P)
            return N[r] if scratch else self.ring[:, r]

        # launch 2: per split a sliding window of T rows, one row entering per partition
        slabs = []
        for p0 in range(0, P, rows):
            win = [row(j - p0) for j in range(T)]
            acc = [np.zeros((self.C, B + 1), dtype=np.complex128) for _ in range(T)]
            for p in range(p0, min(P, p0 + rows)):
                for j in range(T):
                    acc[j] += self.H[:, p] * win[j]
                entering = row(-(p + 1)) if p + 1 < P else None
                win = [entering] + win[:-1]
            slabs.append(acc)
        # launch 3: slabs in order, c2r, commit after the MAC, prev
        out, tails = np.empty((self.C, T * B)), []
        for j in range(T):
            total = slabs[0][j].copy()
            for s in slabs[1:]:
                total += s[j]
            y = np.fft.irfft(total, n=2 * B, axis=-1)
            out[:, j * B:(j + 1) * B] = y[:, :B] if self.ola else y[:, B:]
            tails.append(y[:, B:].copy())
        written = []
        for j in range(T):
            r = commit_row(j, T, P, w)
            if r >= 0:
                self.ring[:, r] = N[j]
                written.append(r)
        assert len(set(written)) == len(written) == min(T, P)
        # launch 4 (overlap-add): the tail chain
        if self.ola:
            for j in range(T):
                out[:, j * B:(j + 1) * B] += self.prev if j == 0 else tails[j - 1]
            self.prev = tails[-1]
        else:
            self.prev = blk[-1].copy()
        self.w = (w + T) % P
        return out

    def process(self, x, T=1, rows=None):
        """A process call: whole passes of T blocks (T = 1: none), then plain steps."""
        B = self.B
        nb = x.shape[1] // B
        y = np.empty_like(x)
        done = 0
        while T > 1 and done + T <= nb:
            y[:, done * B:(done + T) * B] = self.run_pass(x[:, done * B:(done + T) * B], T, rows)
            done += T
        for t in range(done, nb):
            y[:, t * B:(t + 1) * B] = self.step(x[:, t * B:(t + 1) * B])
        return y


def sequence(T):
    """The interleaving both test files run: (blocks, batched) per call."""
    return [(3, False), (T + 5, True), (2, False), (2 * T, True)]
