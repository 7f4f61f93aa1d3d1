"""Seeded call scripts over every way the four handle families run a block (dense float32, sparse,
matrix, double precision), the runner that plays one on a handle and the float64 model of what
the handle must return. A plain module like group_script.py: test_call_script.py (no GPU) and
test_call_script_gpu.py import it.

A Script is a shape, a method, handle options, its filters (filter 0 is the one the fresh handle is
given) and a list of events
    ("blocks", n, how)           n input blocks; how "step": one call per block, "call": one call over all n
    ("batch", on) ("offline", on)  set_batch / set_offline
    ("ahead", on)                dense set_ahead (streaming levels)
    ("levels", on)               matrix set_levels (window levels, the default windows 8 and 32)
    ("update", f, F, curve)      update_filter to filter f over F blocks, "linear" or "cosine"
    ("refused_update", f)        the same call while a fade has blocks left: it raises, nothing changes
    ("filter", f)                the resetting call
    ("reset",)
A sparse filter is its partitions and its mask; an update changes both.

walk(script)   the state rules of include/neo_hip.h alone, no arithmetic: which banks every block
               mixes, the fade's remaining blocks after every event, the epochs (stretches between
               state-clearing events) and where every event and fade sits. The coverage conditions
               of test_call_script.py are conditions on this.
model(script)  numpy float64 only; it never calls the library or the oracle. Block by block in the
               frequency domain, as upols_f64_truth.blockwise: X_t = rfft of the 2B window (overlap-
               save: previous block | block; overlap-add: block | zeros), Y_t = sum_p H[p] X_{t-p}
               over the blocks since the last clearing event, irfft; last B samples (overlap-save)
               or first B plus the tail of Y_{t-1} (overlap-add). H are the values the handle is
               given (complex64 promoted, complex128 for the double family, parts * mask for sparse),
               a matrix output the sum over its routes. Sample n of a fade is y_A + g[n] (y_B - y_A),
               t = n / (F B), g = t (linear) or 0.5 - 0.5 cos(pi t) (cosine), both banks fed the whole
               history since the last clearing event.
run(neo, torch, script)  plays the script on a fresh handle, in place on a CUDA tensor on the current
               stream, filters as host arrays; returns the output and fade_info()["remaining_blocks"]
               after every event.
make_script(family, shape_id, seed)  draws the events from np.random.default_rng(seed): only legal
               sequences (an update only with no fade blocks left, except in refused_update). The
               scenes a seed list must hold (test_call_script.py's coverage conditions) are placed
               deterministically, one set per seed % 4, between the random stretches; SEEDS has one
               seed of every residue per shape.

"Wrapped" in the coverage conditions means that at least P blocks ran since the last clearing event:
every row of the P-row delay line has been written (a mode's longer ring holds P live rows as well).
The call-length classes are stated for every T the library uses (8, 16 or 32 blocks per pass):
"< T" is 2 .. 7 blocks, "a multiple of T plus a rest" is 32 q + r with 1 <= r <= 7."""
import numpy as np

FAMILIES = ("dense", "sparse", "matrix", "f64")
CURVES = ("linear", "cosine")
NFILTERS = 3
SAMPLE_RATE = 48000.0
MASK_DB = (-40.0, -20.0)  # filter f takes MASK_DB[f % 2]: an update changes the mask as well

# the "lower" list of tests/test_matrix_gpu.py's ROUTE_LISTS (lower-triangular: banded), cut to the shape
LOWER = [(o, i) for o in range(4) for i in range(o + 1)]

SHAPES = {
    "dense": [
        dict(dims=(2, 64, 70), method="upols", options={}),
        dict(dims=(2, 32, 300), method="upols", options={"far_level": 1}),
        dict(dims=(3, 64, 450), method="upols", options={"step_group": 4, "windows": 1}),
        dict(dims=(2, 64, 700), method="upola", options={"step_group": 2, "windows": 2}),
        dict(dims=(2, 64, 420), method="upols", options={"step_group": 4, "far_level": 2}),
        dict(dims=(2, 32, 37), method="upols", options={"levels": 0, "fused": 0}),
        dict(dims=(2, 32, 37), method="upols", options={"levels": 0, "fused": 1}),
    ],
    "sparse": [dict(dims=d, method=m, options={"fused": f})
               for d in ((2, 32, 37), (2, 512, 70)) for m in ("upols", "upola") for f in (0, 1)],
    "matrix": [dict(dims=d, method=m, options={})
               for d in ((2, 2, 32, 130), (3, 5, 128, 37)) for m in ("upols", "upola")],
    "f64": [dict(dims=d, method=m, options={})
            for d in ((2, 16, 130), (1, 128, 9)) for m in ("upols", "upola")],
}
# four seeds per shape, one of every residue mod 4 (the scene sets of make_script)
_SEEDS = {
    "dense": [(0, 5, 10, 15), (52, 57, 42, 47), (84, 89, 94, 99), (136, 121, 126, 131), (168, 173, 178, 163),
              (200, 205, 210, 215), (252, 257, 242, 247)],
    "sparse": [(1000, 1005, 1010, 1015), (1052, 1057, 1042, 1047), (1084, 1089, 1094, 1099), (1136, 1121, 1126, 1131),
               (1168, 1173, 1178, 1163), (1200, 1205, 1210, 1215), (1252, 1257, 1242, 1247), (1284, 1289, 1294, 1299)],
    "matrix": [(2000, 2005, 2010, 2015), (2052, 2057, 2042, 2047), (2084, 2089, 2094, 2099), (2136, 2121, 2126, 2131)],
    "f64": [(3000, 3005, 3010, 3015), (3052, 3057, 3042, 3047), (3084, 3089, 3094, 3099), (3136, 3121, 3126, 3131)],
}
SEEDS = {(fam, k): seeds for fam in FAMILIES for k, seeds in enumerate(_SEEDS[fam])}


def shape_name(family, k):
    sh = SHAPES[family][k]
    opts = "".join(f"-{a}{b}" for a, b in sorted(sh["options"].items()))
    return f"{family}-{'x'.join(str(d) for d in sh['dims'])}-{sh['method']}{opts}"


class Script:
    def __init__(self, family, shape_id, method, dims, options, events, seed=None, name=None):
        assert family in FAMILIES and method in ("upols", "upola")
        self.family, self.shape_id, self.method, self.dims, self.options = family, shape_id, method, tuple(dims), dict(options)
        self.events, self.seed = list(events), seed
        self.name = name or f"{shape_name(family, shape_id)}-seed{seed}"
        self.B, self.P = self.dims[-2], self.dims[-1]
        self.inputs = self.dims[0]
        self.outputs = self.dims[1] if family == "matrix" else self.dims[0]
        self.routes = [(o, i) for o, i in LOWER if o < self.outputs and i < self.inputs] if family == "matrix" else None
        self.nblocks = sum(ev[1] for ev in self.events if ev[0] == "blocks")

    # -- what the handle is given: made once per shape (filters) and per script (signal), read-only --
    def filters(self):
        return _filters(self.family, self.dims)[0]

    def masks(self):
        """sparse: the masks [NFILTERS][C][P][B+1] uint8 (neo.perceptual_mask_host, on the host)"""
        assert self.family == "sparse"
        key = ("mask", self.dims)
        if key not in _cache:
            import neo

            out = []
            for f, H in enumerate(self.filters()):
                m = neo.perceptual_mask_host(H, neo.PerceptualSparsity(SAMPLE_RATE, MASK_DB[f % 2], 0, "a"))
                m = np.ascontiguousarray(np.asarray(m) != 0, dtype=np.uint8)
                m.setflags(write=False)
                out.append(m)
            _cache[key] = out
        return _cache[key]

    def effective_filters(self):
        """complex128: the values the handle computes with"""
        H = [np.asarray(h, dtype=np.complex128) for h in self.filters()]
        if self.family == "sparse":
            H = [h * m for h, m in zip(H, self.masks())]
        return H

    def signal(self):
        key = ("x", self.name)
        if key not in _cache:
            rng = np.random.default_rng([77, FAMILIES.index(self.family), self.shape_id, self.seed or 0, self.nblocks])
            x = rng.uniform(-1.0, 1.0, (self.inputs, self.nblocks * self.B))
            x = x.astype(np.float64 if self.family == "f64" else np.float32)
            x.setflags(write=False)
            _cache[key] = x
        return _cache[key]

    def prefix(self):
        """the events before the first mode-changing event, and the blocks they hold"""
        k = next((k for k, ev in enumerate(self.events) if ev[0] in MODE_EVENTS), len(self.events))
        return k, sum(ev[1] for ev in self.events[:k] if ev[0] == "blocks")


MODE_EVENTS = ("batch", "offline", "ahead", "levels")
_cache = {}


def _filters(family, dims):
    """NFILTERS filters of a shape and their impulse responses: exponentially decaying noise (60 dB
    over its length, so that the sparse masks drop the late partitions' weak bins), every row
    scaled to unit energy, partitioned by numpy's rfft in float64 and rounded once to the handle's
    type. The last partition is zero-padded (L = P B - 3)."""
    key = ("H", family, dims)
    if key not in _cache:
        B, P = dims[-2], dims[-1]
        rows = len([1 for o, i in LOWER if o < dims[1] and i < dims[0]]) if family == "matrix" else dims[0]
        L = P * B - 3
        rng = np.random.default_rng([55, FAMILIES.index(family)] + list(dims))
        Hs, irs = [], []
        for _ in range(NFILTERS):
            ir = rng.standard_normal((rows, L)) * 10.0 ** (-3.0 * np.arange(L) / L)
            ir /= np.sqrt((ir * ir).sum(axis=1, keepdims=True))
            if family != "f64":
                ir = ir.astype(np.float32).astype(np.float64)
            pad = np.zeros((rows, P * B))
            pad[:, :L] = ir
            seg = np.zeros((rows, P, 2 * B))
            seg[:, :, :B] = pad.reshape(rows, P, B)
            H = np.fft.rfft(seg, axis=-1).astype(np.complex128 if family == "f64" else np.complex64)
            H.setflags(write=False)
            ir.setflags(write=False)
            Hs.append(H)
            irs.append(ir)
        _cache[key] = (Hs, irs)
    return _cache[key]


# ------------------------------------------------------------------------------------- state rules
class Walk:
    """blocks[t] = (epoch, a, b, k, F, curve): block t mixes banks a and b at block k of a fade of F
    (b None: bank a alone). remaining[e]: the fade's blocks left after event e. epochs: [start, end)
    block ranges between clearing events (empty ones dropped). at[e]: before event e, the block
    index `block`, the blocks `since` the last clearing event and the fade blocks `left`.
    fades: per update its event, `start` (block), `since` (blocks since the clearing event at its
    first block), F, and `end`: the block after its last one if it ran out, None if it was cut."""

    def __init__(self):
        self.blocks, self.remaining, self.epochs, self.at, self.fades = [], [], [], [], []


def walk(script):
    w = Walk()
    cur, fade = 0, None  # fade: [b, F, curve, done, record]
    start = 0

    def clear():
        nonlocal start
        if len(w.blocks) > start:
            w.epochs.append((start, len(w.blocks)))
        start = len(w.blocks)

    for e, ev in enumerate(script.events):
        t = len(w.blocks)
        w.at.append({"block": t, "since": t - start, "left": fade[1] - fade[3] if fade else 0})
        if ev[0] == "blocks":
            assert ev[1] >= 1 and ev[2] in ("step", "call"), ev
            for _ in range(ev[1]):
                if fade:
                    w.blocks.append((len(w.epochs), cur, fade[0], fade[3], fade[1], fade[2]))
                    fade[3] += 1
                    if fade[3] == fade[1]:
                        fade[4]["end"] = len(w.blocks)
                        cur, fade = fade[0], None
                else:
                    w.blocks.append((len(w.epochs), cur, None, 0, 0, None))
        elif ev[0] == "update":
            _, f, F, curve = ev
            assert fade is None, "an update with fade blocks left is not legal: use refused_update"
            assert script.family != "f64" and 0 <= f < NFILTERS and F >= 1 and curve in CURVES, ev
            rec = {"event": e, "start": t, "since": t - start, "F": F, "end": None}
            w.fades.append(rec)
            fade = [f, F, curve, 0, rec]
        elif ev[0] == "refused_update":
            assert fade is not None, "refused_update needs a running fade"
        elif ev[0] == "filter":
            cur, fade = ev[1], None
            clear()
        elif ev[0] == "reset":
            if fade:
                cur, fade = fade[0], None
            clear()
        elif ev[0] in MODE_EVENTS:
            pass  # mode switches keep a running fade and change no value
        else:
            raise ValueError(ev[0])
        w.remaining.append(fade[1] - fade[3] if fade else 0)
    clear()
    return w


def gains(B, F, k, curve):
    """g[n] of block k of a fade of F blocks, float64"""
    t = (k * B + np.arange(B, dtype=np.float64)) / (F * B)
    return t if curve == "linear" else 0.5 - 0.5 * np.cos(np.pi * t)


# ------------------------------------------------------------------------------------------ model
class Model:
    def __init__(self, y, walked):
        self.y, self.walk, self.remaining, self.epochs = y, walked, walked.remaining, walked.epochs


def _spectra(x, B, ola):
    """X [rows][n][B+1] of an epoch's input x [rows][n B] float64"""
    rows, n = x.shape[0], x.shape[1] // B
    blk = x.reshape(rows, n, B)
    win = np.zeros((rows, n, 2 * B))
    if ola:
        win[:, :, :B] = blk
    else:
        win[:, :, B:] = blk
        win[:, 1:, :B] = blk[:, :-1]
    return np.fft.rfft(win, axis=-1)


def model(script):
    """The expected output [outputs][nblocks B] float64 and the walk, made once per script."""
    key = ("model", script.name)
    if key in _cache:
        return _cache[key]
    w = walk(script)
    B, P, ola = script.B, script.P, script.method == "upola"
    H = script.effective_filters()
    x = np.asarray(script.signal(), dtype=np.float64)
    y = np.zeros((script.outputs, script.nblocks * B))
    if script.family == "matrix":
        r_in = np.array([i for _, i in script.routes])
        r_out = np.array([o for o, _ in script.routes])
    for a, b in w.epochs:
        X = _spectra(x[:, a * B:b * B], B, ola)
        if script.family == "matrix":
            X = X[r_in]  # one row per route
        Y = {}  # (filter, block in the epoch) -> irfft(Y_t) [outputs][2B]

        def out(f, t):
            if (f, t) not in Y:
                m = min(P, t + 1)
                acc = (H[f][:, :m] * X[:, t - m + 1:t + 1][:, ::-1]).sum(axis=1)
                if script.family == "matrix":
                    per = acc
                    acc = np.zeros((script.outputs, B + 1), dtype=np.complex128)
                    np.add.at(acc, r_out, per)
                Y[(f, t)] = np.fft.irfft(acc, n=2 * B, axis=-1)
            return Y[(f, t)]

        def bank(f, t):
            if not ola:
                return out(f, t)[:, B:]
            return out(f, t)[:, :B] + (out(f, t - 1)[:, B:] if t else 0.0)

        for t in range(b - a):
            _, fa, fb, k, F, curve = w.blocks[a + t]
            ya = bank(fa, t)
            if fb is not None:
                ya = ya + gains(B, F, k, curve) * (bank(fb, t) - ya)
            y[:, (a + t) * B:(a + t + 1) * B] = ya
            for key2 in [q for q in Y if q[1] < t]:
                del Y[key2]
    y.setflags(write=False)
    _cache[key] = Model(y, w)
    return _cache[key]


def script_error(y, m):
    """max over channels and epochs of max|y - truth| / that channel's truth peak in that epoch;
    epochs shorter than 4 blocks take the whole run's peak of the channel."""
    y = np.asarray(y, dtype=np.float64)
    B = m.y.shape[1] // len(m.walk.blocks)
    assert y.shape == m.y.shape, (y.shape, m.y.shape)
    whole = np.abs(m.y).max(axis=1)
    worst = 0.0
    for a, b in m.epochs:
        s = slice(a * B, b * B)
        peak = np.abs(m.y[:, s]).max(axis=1) if b - a >= 4 else whole
        err = np.abs(y[:, s] - m.y[:, s]).max(axis=1) / np.maximum(peak, 1e-300)
        worst = max(worst, float(err.max()))
    return worst


# ----------------------------------------------------------------------------------------- runner
def make_handle(neo, script):
    d, fam = script.dims, script.family
    if fam == "dense":
        conv = neo.UpolsConvolver(*d, method=script.method, options=script.options)
        conv.filter(script.filters()[0])
    elif fam == "sparse":
        conv = neo.SparseUpolsConvolver(*d, method=script.method, options=script.options)
        conv.filter(script.filters()[0], script.masks()[0])
    elif fam == "matrix":
        conv = neo.MatrixConvolver(*d, method=script.method, options=script.options)
        conv.filter(script.filters()[0], script.routes)
    else:
        conv = neo.UpolsConvolver64(*d, method=script.method)
        conv.filter(script.filters()[0])
    return conv


def run(neo, torch, script, events=None):
    """Plays the script (or its first `events` events) on a fresh handle. Returns the output
    [outputs][blocks played * B], fade_info()["remaining_blocks"] after every event (0 for the
    double family, which has no fades) and how many refused updates raised NeoHipError."""
    fam, B = script.family, script.B
    evs = script.events if events is None else script.events[:events]
    x = script.signal()
    n = x.shape[1]
    rows = max(script.inputs, script.outputs)
    t = torch.zeros((rows, n), dtype=torch.float64 if fam == "f64" else torch.float32, device="cuda")
    t[:script.inputs] = torch.from_numpy(np.array(x)).cuda()
    item = t.element_size()
    s = torch.cuda.current_stream().cuda_stream
    conv = make_handle(neo, script)
    H = script.filters()
    remaining, refused, done = [], 0, 0

    def update(f, F=2, curve="linear"):
        if fam == "sparse":
            conv.update_filter(H[f], script.masks()[f], fade_blocks=F, curve=curve)
        else:
            conv.update_filter(H[f], fade_blocks=F, curve=curve)

    def blocks(k):
        p = t.data_ptr() + item * done * B
        if fam == "dense" or fam == "sparse":
            if k == 1:
                conv.process_device(p, n, p, n, s)
            else:
                conv.process_blocks_ptr(p, p, n, k, s)
        elif fam == "matrix":
            conv.process_device(p, n, p, n, k, s)
        else:
            conv.process_device(p, n, p, n, k * B, s)

    try:
        for ev in evs:
            if ev[0] == "blocks":
                if ev[2] == "step":
                    for _ in range(ev[1]):
                        blocks(1)
                        done += 1
                else:
                    blocks(ev[1])
                    done += ev[1]
            elif ev[0] == "batch":
                conv.set_batch(ev[1])
            elif ev[0] == "offline":
                conv.set_offline(ev[1])
            elif ev[0] == "ahead":
                conv.set_ahead(ev[1])
            elif ev[0] == "levels":
                conv.set_levels(ev[1])
            elif ev[0] == "update":
                update(*ev[1:])
            elif ev[0] == "refused_update":
                try:
                    update(ev[1])
                except neo._native.NeoHipError:
                    refused += 1
                else:
                    raise AssertionError(f"{script.name}: an update with fade blocks left was accepted")
            elif ev[0] == "filter":
                if fam == "sparse":
                    conv.filter(H[ev[1]], script.masks()[ev[1]])
                elif fam == "matrix":
                    conv.filter(H[ev[1]], script.routes)
                else:
                    conv.filter(H[ev[1]])
            elif ev[0] == "reset":
                conv.reset()
            else:
                raise ValueError(ev[0])
            remaining.append(conv.fade_info()["remaining_blocks"] if fam != "f64" else 0)
        torch.cuda.synchronize()
        y = t[:script.outputs, :done * B].cpu().numpy()
    finally:
        conv.close()
    return y, remaining, refused


# -------------------------------------------------------------------------------------- generator
def capabilities(family, shape_id):
    """What the shape's handle can be asked: fades, its mode events with the handle's defaults, the
    mode that turns the streaming (window) levels on, whether it has offline windows, and the
    script's block budget."""
    sh = SHAPES[family][shape_id]
    B, P = sh["dims"][-2], sh["dims"][-1]
    if family == "dense":
        streaming = sh["options"].get("levels", -1) != 0
        modes = {"batch": True}
        if P >= 128:
            modes["offline"] = True  # (the library refuses offline windows below 128 partitions)
        if streaming:
            modes["ahead"] = True
        return dict(fades=True, modes=modes, levels="ahead" if streaming else None, offline=P >= 128, budget=900)
    if family == "sparse":
        return dict(fades=True, modes={"batch": False}, levels=None, offline=False, budget=150 if B == 512 else 900)
    if family == "matrix":
        return dict(fades=True, modes={"batch": False, "offline": False, "levels": False}, levels="levels", offline=True,
                    budget=900 if B <= 32 else 700)
    return dict(fades=False, modes={"batch": False, "offline": False}, levels=None, offline=True, budget=900)


class _Gen:
    def __init__(self, family, shape_id, seed):
        self.cap = capabilities(family, shape_id)
        self.P = SHAPES[family][shape_id]["dims"][-1]
        self.rng = np.random.default_rng(seed)
        self.ev, self.n, self.since, self.left, self.cur = [], 0, 0, 0, 0
        self.modes = dict(self.cap["modes"])
        self.budget = self.cap["budget"]

    def blocks(self, n, how):
        if n <= 0:
            return
        self.ev.append(("blocks", int(n), how))
        self.n += n
        self.since += n
        if self.left:
            if n >= self.left:
                self.cur, self.left = self.nxt, 0
            else:
                self.left -= n

    def mode(self, name, on):
        if name in self.modes:
            self.ev.append((name, bool(on)))
            self.modes[name] = bool(on)

    def other(self):
        busy = (self.cur, self.nxt) if self.left else (self.cur,)
        return int(self.rng.choice([f for f in range(NFILTERS) if f not in busy]))

    def finish_fade(self):
        if self.left:
            self.blocks(self.left, "step")

    def update(self, F, curve=None):
        if not self.cap["fades"]:
            return
        self.finish_fade()
        self.nxt = self.other()
        self.ev.append(("update", self.nxt, int(F), curve or CURVES[int(self.rng.integers(2))]))
        self.left = int(F)

    def refused(self):
        if self.cap["fades"] and self.left:
            self.ev.append(("refused_update", self.other()))

    def clear(self, kind):
        if kind == "reset":
            self.ev.append(("reset",))
            if self.left:
                self.cur = self.nxt
        else:
            self.cur = self.other()
            self.ev.append(("filter", self.cur))
        self.left, self.since = 0, 0

    def levels_on(self):
        """single steps then run the streaming (window) levels"""
        if self.cap["levels"] and not self.modes[self.cap["levels"]]:
            self.mode(self.cap["levels"], True)

    def offline_on(self):
        """a call of >= 128 blocks then runs offline windows (dense: they take batching as well)"""
        for name in ("batch", "offline"):
            if name in self.modes and not self.modes[name]:
                self.mode(name, True)

    def to_phase(self, ph, mod=32):
        self.finish_fade()
        self.blocks((ph - self.since) % mod, "step")

    def fade_in_steps(self, F, after=3, curve=None):
        self.levels_on()
        self.update(F, curve)
        self.blocks(F + after, "step")

    def filler(self, until_since=None, until_n=None):
        """random legal scenes without a clearing event until `since` or the block count is reached"""
        r = self.rng
        while (until_since is not None and self.since < until_since) or (until_n is not None and self.n < until_n):
            room = until_since - self.since if until_since is not None else until_n - self.n
            k = int(r.integers(6))
            if k == 0:
                self.blocks(min(room, int(r.integers(1, 24))), "step")
            elif k == 1:
                self.blocks(min(room, int(r.integers(2, 8))), "call")
            elif k == 2:
                self.blocks(min(room, 32 * int(r.integers(1, 3)) + int(r.integers(1, 8))), "call")
            elif k == 3 and self.cap["fades"]:
                self.update(int(r.integers(1, 13)))
                self.blocks(min(room, int(r.integers(1, 16))), "step" if r.integers(2) else "call")
            elif k == 4 and self.cap["fades"] and self.left:
                self.refused()
                self.blocks(1, "step")
            else:
                name = list(self.modes)[int(r.integers(len(self.modes)))]
                self.mode(name, not self.modes[name])
                self.blocks(min(room, int(r.integers(1, 10))), "step" if r.integers(2) else "call")


def make_script(family, shape_id, seed):
    sh = SHAPES[family][shape_id]
    g = _Gen(family, shape_id, seed)
    r, P, v = g.rng, g.P, seed % 4
    small = g.budget < 300
    phases = [int(p) for p in r.permutation([p for p in range(32) if p % 4 == v])]
    rest = int(r.integers(1, 8))
    if family == "matrix" and v != 3:
        g.blocks(int(r.integers(3, 10)), "step")  # plain steps first: the levels prime in mid-stream
        g.levels_on()
    if v == 0:
        # an update before block P, a fade longer than a window, an update right after a fade's last block
        g.to_phase(phases[0])
        g.fade_in_steps(int(r.integers(33, 48)) if not small else int(r.integers(5, 12)), after=int(r.integers(0, 3)))
        g.fade_in_steps(3, after=4)
        if not small:
            g.to_phase(phases[1])
            g.fade_in_steps(int(r.integers(1, 9)), after=2)
            g.offline_on()
            g.blocks(256 + 128 + int(r.integers(1, 40)), "call")
        g.filler(until_since=P)
        # the offline toggles with the ring wrapped (dense below 128 partitions, sparse: batching's)
        if g.cap["offline"]:
            g.offline_on()
            g.mode("offline", False)
            g.blocks(128 + rest, "call")
            g.mode("offline", True)
            g.blocks(128, "call")
        else:
            g.mode("batch", not g.modes["batch"])
            g.blocks(32 + rest, "call")
            g.mode("batch", not g.modes["batch"])
            g.blocks(32 + rest, "call")
    elif v == 1:
        # a fade that ends on a window boundary; the batch and level toggles with the ring wrapped
        if not small:
            g.to_phase(phases[0])
            g.fade_in_steps(int(r.integers(1, 9)))
        F = int(r.integers(2, 12))
        g.to_phase(-F)
        g.fade_in_steps(F, after=5)
        if not small:
            g.to_phase(phases[1])
            g.fade_in_steps(int(r.integers(1, 9)))
            g.offline_on()
            g.blocks(256, "call")
        g.filler(until_since=P)
        g.mode("batch", not g.modes["batch"])
        g.blocks(32 + rest, "call")
        g.mode("batch", not g.modes["batch"])
        g.blocks((32 if small else 64) + rest, "call")
        if g.cap["levels"]:
            g.levels_on()
            g.blocks(5, "step")
            g.mode(g.cap["levels"], False)
            g.blocks(4, "step")
            g.update(4)
            g.blocks(7, "step")
            g.mode(g.cap["levels"], True)
            g.blocks(40, "step")
    elif v == 2:
        # clearing events with fade blocks left, a reset before the ring has filled, a refused update, calls
        # that span a whole fade, an offline call that starts inside a fade, a fade across a multiple of 128
        g.blocks(int(r.integers(3, 12)), "step")
        g.update(6)
        g.blocks(2, "step")
        g.clear("reset")
        g.to_phase(phases[0])
        g.fade_in_steps(int(r.integers(1, 9)))
        g.update(5)
        g.blocks(2, "step")
        g.refused()
        g.blocks(6, "step")
        g.update(4)
        g.blocks(32 + rest, "call")
        g.update(7)
        g.blocks(3, "call")
        g.clear("filter")
        g.blocks(int(r.integers(5, 20)), "step")
        if small:
            g.mode("batch", not g.modes["batch"])
            g.blocks(32 + rest, "call")
        else:
            g.offline_on()
            g.update(5)
            g.blocks(5 + 128 + rest, "call")
            g.to_phase(-int(r.integers(2, 6)), 128)
            g.fade_in_steps(8, after=6)
            g.to_phase(phases[1])
            g.fade_in_steps(int(r.integers(1, 9)))
    else:
        # mostly random: stretches between clearing events drawn at random, with and without fade blocks left
        g.blocks(int(r.integers(2, 8)), "call")
        g.clear("reset")
        for k in range(2):
            g.filler(until_since=int(r.integers(10, 30) if small else r.integers(20, 60)))
            if not small:
                g.to_phase(phases[k])
            g.fade_in_steps(int(r.integers(1, 9)), after=int(r.integers(0, 4)))
            if r.integers(2):
                g.update(int(r.integers(2, 9)))
                g.blocks(1, "step")
            g.clear("reset" if k else "filter")
        if not small:
            g.offline_on()
            g.blocks(128, "call")
    g.filler(until_n=g.budget)
    return Script(family, shape_id, sh["method"], sh["dims"], sh["options"], g.ev, seed=seed)


# Minimal failing scripts found by the seeds, kept as named regression cases: name -> Script.
REGRESSIONS = {}


def all_scripts():
    """(family, shape id, seed) of every committed script"""
    return [(fam, k, seed) for fam in FAMILIES for k in range(len(SHAPES[fam])) for seed in SEEDS[(fam, k)]]


_scripts = {}


def script(family, shape_id, seed):
    key = (family, shape_id, seed)
    if key not in _scripts:
        _scripts[key] = make_script(family, shape_id, seed)
    return _scripts[key]
