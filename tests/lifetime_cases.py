"""Case tables and runners of tests/test_lifetime_gpu.py: one script per case, run `serial` (a
device-wide synchronize after every call) or `held` (the caller's side stream held back by
stream_holds.hold, no host synchronization from the hold to the reuse step).

Every runner returns (outputs, truths, problems, host seconds): the outputs by name as arrays, for
the serial run the expected value of every output (the oracle's or the float64 numpy statement's)
with its tolerance, the list of what went wrong on the way (a hold that was too short, a call
marked J that returned before the queued work was done, a reuse step that reserved device memory)
and the host time from the first queued call to the return of the call under test. A plain
module: the test module imports it, nothing here is collected."""
import time

import numpy as np

F32_TOL = 1e-5   # the project's float32 bar, of the peak
F64_TOL = 1e-12  # upols_f64_truth.TOL

B = 64
FADE = 3  # fade_blocks of every update


class Ctx:
    """The steps of the issue's script that every kind shares."""

    def __init__(self, neo, torch, mode, hold_us):
        import stream_holds

        self.neo, self.torch, self.mode, self.hold_us, self.holds = neo, torch, mode, hold_us, stream_holds
        self.held = mode == "held"
        self.side = torch.cuda.Stream()  # torch's current stream stays the default stream
        self.problems = []
        self.host_s = 0.0
        self.done = None
        if self.held:
            stream_holds.calibrate()  # (synchronizes: before anything is queued)

    @property
    def s(self):
        return self.side.cuda_stream

    def sync(self):
        """after every call of the serial run; nothing in the held run"""
        if not self.held:
            self.torch.cuda.synchronize()

    def start(self, stream=None):
        """inputs are there, then the hold; the host clock starts at the first queued call"""
        self.torch.cuda.synchronize()
        if self.held:
            self.holds.hold(self.side if stream is None else stream, self.hold_us)
        self.t0 = time.perf_counter()

    def queued(self, stream=None):
        """after the last queued call: the event the J calls must have waited for"""
        self.done = self.torch.cuda.Event()
        self.done.record(self.side if stream is None else stream)
        if self.held and self.done.query():
            self.problems.append(f"the hold of {self.hold_us:.0f} us was too short: the queued work had finished "
                                 "before the call under test, the case proves nothing")

    def under_test(self, what, fn, joins):
        fn()
        self.host_s = max(self.host_s, time.perf_counter() - self.t0)
        if self.held and joins and not self.done.query():
            self.problems.append(f"J: {what} returned before the work queued on the side stream was done")
        self.sync()

    def reuse(self, fn):
        """the second object's bring-up and blocks: out of the ranges just freed, no new chunk"""
        before = self.neo.memory_info()["reserved"]
        out = fn()
        after = self.neo.memory_info()["reserved"]
        if after != before:
            self.problems.append(f"the reuse step reserved device memory: {before} -> {after} bytes")
        return out

    def finish(self):
        self.torch.cuda.synchronize()


def _host(t):
    return t.cpu().numpy()


def _mix(yA, yB, g, first, blocks):
    """y_A + g (y_B - y_A) over `blocks` blocks from block `first`, y_B after them"""
    out = np.array(yB, dtype=np.float64)
    a, b = first * B, (first + blocks) * B
    out[:, a:b] = yA[:, a:b] + g.astype(np.float64)[None, :] * (yB[:, a:b].astype(np.float64) - yA[:, a:b])
    out[:, :a] = yA[:, :a]
    return out


_cache = {}


def _cached(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ------------------------------------------------------------------------------- dense convolvers
# handle: P, options, streaming (set_batch(False)), blocks of queued work, one call for all of them
DENSE_HANDLES = {
    "a": (9, {}, True, 6, False),                   # the plain step
    "b": (300, {"step_group": 4}, True, 140, False),  # streaming levels, background stream and events
    "c": (300, {}, False, 291, True),               # an offline pass of 256, a pass of 32, three steps
}
DENSE_J = ["close", "filter", "set_impulse", "reset", "update_filter"]
DENSE_SETTERS = [("b", "set_ahead"), ("c", "set_batch"), ("c", "set_offline")]
# blocks stepped on the side stream after the call (an update: the fade's and two past it)
DENSE_AFTER = {"close": 0, "filter": 4, "set_impulse": 4, "reset": 4, "update_filter": FADE + 2, "set_ahead": 16,
               "set_batch": 8, "set_offline": 8}
DENSE_CASES = ([(h, m, c) for h in DENSE_HANDLES for m in ("upols", "upola") for c in DENSE_J] +
               [(h, m, c) for h, c in DENSE_SETTERS for m in ("upols", "upola")])
C = 2


def dense_problem(oracle, P, nb):
    def make():
        irs = [np.stack([oracle.noise(7100 + 13 * P + 7 * k + c, B * P) for c in range(C)]) for k in range(2)]
        parts = [oracle.uniform_partition(oracle.normalize_impulse(ir), B) for ir in irs]
        sig = np.stack([oracle.noise(7150 + 13 * P + c, B * nb) for c in range(C)])
        return irs[0], irs[1], parts[0], parts[1], sig
    return _cached(("dense", P, nb), make)


def _conv_ref(oracle, key, sig, parts, method):
    return _cached(("ref",) + key, lambda: oracle.dense_convolve(np.ascontiguousarray(sig), parts, method=method))


def _steps(conv, x, y, first, n, stream, one_call=False):
    """blocks [first, first + n) of x into y: one block per process_device call (launch_step), or
    all of them in one process_blocks call (process_samples)"""
    ld = x.shape[1]
    o = 4 * B * first
    if one_call:
        conv.process_blocks_ptr(x.data_ptr() + o, y.data_ptr() + o, ld, n, stream)
    else:
        for t in range(n):
            conv.process_device(x.data_ptr() + o + 4 * B * t, ld, y.data_ptr() + o + 4 * B * t, ld, stream)


def _second_dense(ctx, make, parts, x, mask=None):
    """step 7: a second object of the same kind and shape, the other filter, two blocks on the
    default stream"""
    torch = ctx.torch
    y2 = torch.full((x.shape[0], 2 * B), 7.0, device="cuda")

    def go():
        conv = make()
        conv.filter(parts) if mask is None else conv.filter(parts, mask)
        conv.set_batch(False)
        for t in range(2):
            conv.process_device(x.data_ptr() + 4 * B * t, x.shape[1], y2.data_ptr() + 4 * B * t, 2 * B, 0)
            ctx.sync()
        return conv
    return ctx.reuse(go), y2


def run_dense(neo, torch, oracle, case, mode, hold_us):
    handle, method, call = case
    P, opts, streaming, Q, one_call = DENSE_HANDLES[handle]
    K = DENSE_AFTER[call]
    ir1, ir2, H1, H2, sig = dense_problem(oracle, P, Q + 16)
    sig = sig[:, :(Q + K) * B] if K else sig[:, :Q * B]
    make = lambda: neo.UpolsConvolver(C, B, P, method=method, options=opts)  # noqa: E731
    conv = make()
    conv.filter(H1)
    if streaming:
        conv.set_batch(False)
    x = torch.from_numpy(sig.copy()).cuda()
    y = torch.full_like(x, 7.0)
    ctx = Ctx(neo, torch, mode, hold_us)
    ctx.start()
    if one_call:
        _steps(conv, x, y, 0, Q, ctx.s, True)
        ctx.sync()
    else:
        for t in range(Q):
            if handle == "a":
                _steps(conv, x, y, t, 1, ctx.s)
            else:
                _steps(conv, x, y, t, 1, ctx.s, True)  # the same block through neo_hip_upols_process_blocks
            ctx.sync()
    ctx.queued()
    fn, joins = {
        "close": (conv.close, True),
        "filter": (lambda: conv.filter(H2), True),
        "set_impulse": (lambda: conv.set_impulse(ir2), True),
        "reset": (conv.reset, True),
        "update_filter": (lambda: conv.update_filter(H2, fade_blocks=FADE, stream=0), True),
        "set_ahead": (lambda: conv.set_ahead(False), False),
        "set_batch": (lambda: conv.set_batch(False), False),
        "set_offline": (lambda: conv.set_offline(False), False),
    }[call]
    ctx.under_test(f"{call}()", fn, joins)
    second, y2 = _second_dense(ctx, make, H2, x)
    if call == "set_ahead":  # plain steps, then the levels again (they prime at the first step)
        for t in range(8):
            _steps(conv, x, y, Q + t, 1, ctx.s, True)
            ctx.sync()
        conv.set_ahead(True)
        for t in range(8, 16):
            _steps(conv, x, y, Q + t, 1, ctx.s, True)
            ctx.sync()
    elif one_call and K:
        _steps(conv, x, y, Q, K, ctx.s, True)
        ctx.sync()
    else:
        for t in range(K):
            _steps(conv, x, y, Q + t, 1, ctx.s, handle != "a")
            ctx.sync()
    ctx.finish()
    got = _host(y)
    outs = {"queued": got[:, :Q * B], "second": _host(y2)}
    if K:
        outs["after"] = got[:, Q * B:]
    second.close()
    conv.close()
    truths = {}
    if mode == "serial":
        key = (P, method)
        truths["queued"] = _conv_ref(oracle, key + ("q", Q), sig[:, :Q * B], H1, method)
        truths["second"] = _conv_ref(oracle, key + ("second",), sig[:, :2 * B], H2, method)
        tail = sig[:, Q * B:]
        if call in ("filter", "set_impulse"):  # the state is rebuilt
            truths["after"] = _conv_ref(oracle, key + ("fresh2", Q, K), tail, H2, method)
        elif call == "reset":
            truths["after"] = _conv_ref(oracle, key + ("fresh1", Q, K), tail, H1, method)
        elif call == "update_filter":
            yA = _conv_ref(oracle, key + ("A", Q, K), sig, H1, method)
            yB = _conv_ref(oracle, key + ("B", Q, K), sig, H2, method)
            truths["after"] = _mix(yA, yB, neo.fade_gains(B, FADE), Q, FADE)[:, Q * B:]
        elif K:
            truths["after"] = _conv_ref(oracle, key + ("A", Q, K), sig, H1, method)[:, Q * B:]
        truths = {k: (v, F32_TOL) for k, v in truths.items()}
    return outs, truths, ctx.problems, ctx.host_s


# ------------------------------------------------------------------------------ sparse convolvers
SPARSE_P, SPARSE_Q = 20, 6
SPARSE_CASES = [(m, c) for m in ("upols", "upola") for c in ("close", "filter", "update_reset")]


def sparse_masks():
    """about 0.5 and 0.1 of the tiles: the lower half of the partitions against the lower half of
    the bins of every fifth partition (the banks differ in size: they are reallocated)"""
    m1 = np.zeros((C, SPARSE_P, B + 1), bool)
    m1[:, :SPARSE_P // 2] = True
    m2 = np.zeros_like(m1)
    m2[:, ::5, :B // 2] = True
    return m1, m2


def run_sparse(neo, torch, oracle, case, mode, hold_us):
    method, call = case
    P, Q = SPARSE_P, SPARSE_Q
    nb = Q + FADE + 2 + 4
    _, _, H1, H2, sig = dense_problem(oracle, P, nb)
    m1, m2 = sparse_masks()
    H1m, H2m = (H1 * m1).astype(np.complex64), (H2 * m2).astype(np.complex64)
    make = lambda: neo.SparseUpolsConvolver(C, B, P, method=method)  # noqa: E731
    conv = make()
    conv.filter(H1, m1)
    x = torch.from_numpy(sig.copy()).cuda()
    y = torch.full_like(x, 7.0)
    ctx = Ctx(neo, torch, mode, hold_us)

    def go(first, n):
        for t in range(n):
            _steps(conv, x, y, first + t, 1, ctx.s)
            ctx.sync()

    ctx.start()
    go(0, Q)
    ctx.queued()
    pos = Q
    if call == "close":
        ctx.under_test("close()", conv.close, True)
    elif call == "filter":
        ctx.under_test("filter()", lambda: conv.filter(H2, m2), True)
    else:
        ctx.under_test("update_filter()", lambda: conv.update_filter(H2, m2, fade_blocks=FADE, stream=0), True)
        ctx.start()  # (the update joined the side stream: a second hold for the reset)
        go(Q, FADE + 2)
        pos = Q + FADE + 2
        ctx.queued()
        ctx.under_test("reset() after the update", conv.reset, True)  # the retired bank's tiles go back
    second, y2 = _second_dense(ctx, make, H2, x, m2)
    K = 0 if call == "close" else 4
    go(pos, K)
    ctx.finish()
    got = _host(y)
    outs = {"queued": got[:, :pos * B], "second": _host(y2)}
    if K:
        outs["after"] = got[:, pos * B:(pos + K) * B]
    second.close()
    conv.close()
    truths = {}
    if mode == "serial":
        key = ("sparse", method)
        truths["second"] = _conv_ref(oracle, key + ("second",), sig[:, :2 * B], H2m, method)
        if call == "update_reset":
            yA = _conv_ref(oracle, key + ("A",), sig[:, :pos * B], H1m, method)
            yB = _conv_ref(oracle, key + ("B",), sig[:, :pos * B], H2m, method)
            truths["queued"] = _mix(yA, yB, neo.fade_gains(B, FADE), Q, FADE)
        else:
            truths["queued"] = _conv_ref(oracle, key + ("q",), sig[:, :Q * B], H1m, method)
        if K:  # filter() and reset() rebuild the state; both leave H2 under mask2
            truths["after"] = _conv_ref(oracle, key + ("fresh", pos), sig[:, pos * B:(pos + K) * B], H2m, method)
        truths = {k: (v, F32_TOL) for k, v in truths.items()}
    return outs, truths, ctx.problems, ctx.host_s


# ------------------------------------------------------------------- double-precision convolvers
F64_P, F64_Q, F64_T = 9, 19, 8  # one call of 8 + 8 + 3 blocks
F64_CASES = [(m, c) for m in ("upols", "upola") for c in ("close", "filter", "reset", "set_batch")]


def f64_problem():
    import upols_f64_truth as T

    def make():
        rng = np.random.default_rng(7300)
        ir = rng.standard_normal((2, C, F64_P * B - 3))
        x = rng.standard_normal((C, (F64_Q + 11) * B))
        return T.partition(ir[0], B), T.partition(ir[1], B), x
    return _cached(("f64",), make)


def run_f64(neo, torch, oracle, case, mode, hold_us):
    import upols_f64_truth as T

    method, call = case
    P, Q = F64_P, F64_Q
    K = {"close": 0, "set_batch": 11}.get(call, 4)
    H1, H2, sig = f64_problem()
    sig = sig[:, :(Q + K) * B]

    def make():
        c = neo.UpolsConvolver64(C, B, P, method=method)
        c.set_batch(F64_T)
        return c
    conv = make()
    conv.filter(H1)
    x = torch.from_numpy(sig.copy()).cuda()
    y = torch.full_like(x, 7.0)
    ld = x.shape[1]
    ctx = Ctx(neo, torch, mode, hold_us)

    def go(c, src, dst, first, n, stream):
        o = 8 * B * first
        c.process_device(src.data_ptr() + o, src.shape[1], dst.data_ptr() + o, dst.shape[1], n * B, stream)
        ctx.sync()

    ctx.start()
    go(conv, x, y, 0, Q, ctx.s)
    ctx.queued()
    fn = {"close": conv.close, "filter": lambda: conv.filter(H2), "reset": conv.reset,
          "set_batch": lambda: conv.set_batch(False)}[call]  # batch_free64 after setup_join64
    ctx.under_test(f"{call}()", fn, True)
    if call == "set_batch":
        conv.set_batch(F64_T)
    y2 = torch.full((C, 2 * B), 7.0, dtype=torch.float64, device="cuda")

    def bring_up():
        c = make()
        c.filter(H2)
        for t in range(2):
            go(c, x, y2, t, 1, 0)
        return c
    second = ctx.reuse(bring_up)
    if K:
        go(conv, x, y, Q, K, ctx.s)
    ctx.finish()
    got = _host(y)
    outs = {"queued": got[:, :Q * B], "second": _host(y2)}
    if K:
        outs["after"] = got[:, Q * B:]
    second.close()
    conv.close()
    truths = {}
    if mode == "serial":
        bw = lambda key, s, H: _cached(("f64ref", method) + key, lambda: T.blockwise(np.ascontiguousarray(s), H, method))  # noqa: E731
        truths["queued"] = bw(("q",), sig[:, :Q * B], H1)
        truths["second"] = bw(("second",), sig[:, :2 * B], H2)
        tail = sig[:, Q * B:]
        if call == "filter":
            truths["after"] = bw(("fresh2", K), tail, H2)
        elif call == "reset":
            truths["after"] = bw(("fresh1", K), tail, H1)
        elif K:
            truths["after"] = bw(("A", K), sig, H1)[:, Q * B:]
        assert ld == sig.shape[1]
        truths = {k: (v, F64_TOL) for k, v in truths.items()}
    return outs, truths, ctx.problems, ctx.host_s


# ------------------------------------------------------------------------------ matrix convolvers
MATRIX_Q = 6
MATRIX_CALLS = [(9, "close"), (9, "filter"), (9, "update_filter"), (9, "set_batch"), (130, "set_offline"),
                (130, "set_levels")]
MATRIX_CASES = [(m, P, c) for m in ("upols", "upola") for P, c in MATRIX_CALLS]
ROUTES = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (out, in): the dense [O][I] order


def matrix_problem(oracle, P, nb):
    def make():
        ir = [np.stack([oracle.noise(7500 + 17 * P + 5 * k + r, B * P) for r in range(4)]) for k in range(2)]
        parts = [oracle.uniform_partition(oracle.normalize_impulse(a), B) for a in ir]
        sig = np.stack([oracle.noise(7560 + 17 * P + i, B * nb) for i in range(2)])
        return parts[0], parts[1], sig
    return _cached(("matrix", P, nb), make)


def _matrix_ref(oracle, key, sig, parts, method):
    def make():
        per = oracle.dense_convolve(np.ascontiguousarray(sig[[i for _, i in ROUTES]]), parts, method=method).astype(np.float64)
        return np.stack([per[0] + per[1], per[2] + per[3]])
    return _cached(("mref",) + key, make)


def run_matrix(neo, torch, oracle, case, mode, hold_us):
    method, P, call = case
    Q = MATRIX_Q
    K = 0 if call == "close" else 8
    H1, H2, sig = matrix_problem(oracle, P, Q + 8)
    sig = sig[:, :(Q + K) * B]
    shape = (2, 2, P, B + 1)
    make = lambda: neo.MatrixConvolver(2, 2, B, P, method=method)  # noqa: E731
    conv = make()
    conv.filter(H1.reshape(shape))
    x = torch.from_numpy(sig.copy()).cuda()
    y = torch.full_like(x, 7.0)
    ctx = Ctx(neo, torch, mode, hold_us)

    def go(c, dst, first, n, stream, one_call=False):
        o = 4 * B * first
        if one_call:
            c.process_device(x.data_ptr() + o, x.shape[1], dst.data_ptr() + o, dst.shape[1], n, stream)
            ctx.sync()
            return
        for t in range(n):
            c.process_device(x.data_ptr() + o + 4 * B * t, x.shape[1], dst.data_ptr() + o + 4 * B * t, dst.shape[1], 1, stream)
            ctx.sync()

    ctx.start()
    go(conv, y, 0, Q, ctx.s)
    ctx.queued()
    fn = {"close": conv.close, "filter": lambda: conv.filter(H2.reshape(shape)),
          "update_filter": lambda: conv.update_filter(H2, fade_blocks=FADE, stream=0),
          "set_batch": lambda: conv.set_batch(True), "set_offline": lambda: conv.set_offline(True),
          "set_levels": lambda: conv.set_levels(True)}[call]
    ctx.under_test(f"{call}()", fn, True)
    y2 = torch.full((2, 2 * B), 7.0, device="cuda")

    def bring_up():
        c = make()
        c.filter(H2.reshape(shape))
        go(c, y2, 0, 2, 0)
        return c
    second = ctx.reuse(bring_up)
    if K:  # the passes the new mode cuts a call into read the re-laid ring; level steps come one per call
        go(conv, y, Q, K, ctx.s, one_call=call in ("set_batch", "set_offline"))
    ctx.finish()
    got = _host(y)
    outs = {"queued": got[:, :Q * B], "second": _host(y2)}
    if K:
        outs["after"] = got[:, Q * B:]
    second.close()
    conv.close()
    truths = {}
    if mode == "serial":
        key = (P, method)
        truths["queued"] = _matrix_ref(oracle, key + ("q",), sig[:, :Q * B], H1, method)
        truths["second"] = _matrix_ref(oracle, key + ("second",), sig[:, :2 * B], H2, method)
        if call == "filter":
            truths["after"] = _matrix_ref(oracle, key + ("fresh2",), sig[:, Q * B:], H2, method)
        elif call == "update_filter":
            yA, yB = (_matrix_ref(oracle, key + (n,), sig, H, method) for n, H in (("A", H1), ("B", H2)))
            truths["after"] = _mix(yA, yB, neo.fade_gains(B, FADE), Q, FADE)[:, Q * B:]
        elif K:
            truths["after"] = _matrix_ref(oracle, key + ("A",), sig, H1, method)[:, Q * B:]
        truths = {k: (v, F32_TOL) for k, v in truths.items()}
    return outs, truths, ctx.problems, ctx.host_s


# --------------------------------------------------------------------------------- overlap stages
OVERLAP_F, OVERLAP_Q = 40, 3
OVERLAP_CASES = ["save", "add"]


def run_overlap(neo, torch, oracle, kind, mode, hold_us):
    F, Q = OVERLAP_F, OVERLAP_Q
    sig = _cached(("overlap",), lambda: np.stack([oracle.noise(7700 + c, B * (Q + 2)) for c in range(C)]))
    make = lambda: neo.OverlapStage(kind, C, B, F)  # noqa: E731
    st = make()
    bins = st.transform_size() // 2 + 1
    x = torch.from_numpy(sig.copy()).cuda()
    y = torch.full_like(x, 7.0)
    spec = torch.zeros((Q + 2, C, bins), dtype=torch.complex64, device="cuda")
    ctx = Ctx(neo, torch, mode, hold_us)

    def go(stage, t, stream):
        blk = slice(t * B, (t + 1) * B)
        stage.forward(x[:, blk], spec[t], stream=stream)
        ctx.sync()
        stage.inverse(spec[t], y[:, blk], stream=stream)
        ctx.sync()

    ctx.start()
    for t in range(Q):
        go(st, t, ctx.s)
    ctx.queued()
    ctx.under_test("close()", st.close, True)

    def bring_up():  # other data: the blocks after the first stage's
        stage = make()
        for t in range(Q, Q + 2):
            go(stage, t, 0)
        return stage
    second = ctx.reuse(bring_up)
    ctx.finish()
    got = _host(y)
    outs = {"queued": got[:, :Q * B], "second": got[:, Q * B:], "spectra": _host(spec)}
    second.close()
    truths = {}
    if mode == "serial":
        ref = lambda s: np.stack([oracle.overlap_stage(kind, np.ascontiguousarray(s[c]), B, F) for c in range(C)])  # noqa: E731
        truths = {"queued": (ref(sig[:, :Q * B]), F32_TOL), "second": (ref(sig[:, Q * B:]), F32_TOL)}
    return outs, truths, ctx.problems, ctx.host_s


# -------------------------------------------------------------------------------------- FFT plans
FFT_CASES = [(0, 13, 2), (16, 13, 2), (1, 14, 1)]  # kind, order, batch: the multi-pass plans that own scratch


def run_fft(neo, torch, oracle, case, mode, hold_us):
    kind, order, batch = case
    n = 1 << order
    if kind == 1:
        xs = [oracle.noise(7800 + k, batch * n).reshape(batch, n) for k in range(2)]
        ref, tol, out_shape, out_dtype = oracle.rfft, F32_TOL, (batch, n // 2 + 1), torch.complex64
    elif kind == 0:
        xs = [oracle.noise(7810 + k, 2 * batch * n).view(np.complex64).reshape(batch, n) for k in range(2)]
        ref, tol, out_shape, out_dtype = oracle.fft, F32_TOL, (batch, n), torch.complex64
    else:
        rng = np.random.default_rng(7820)
        xs = [rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n)) for _ in range(2)]
        ref, tol, out_shape, out_dtype = oracle.fft_f64, F64_TOL, (batch, n), torch.complex128
    dx = [torch.from_numpy(a.copy()).cuda() for a in xs]
    out = [torch.zeros(out_shape, dtype=out_dtype, device="cuda") for _ in range(2)]
    plan = neo.fft.FFTPlan(kind, order, batch)
    ctx = Ctx(neo, torch, mode, hold_us)
    ctx.start()
    plan.execute_device(dx[0].data_ptr(), out[0].data_ptr(), -1, ctx.s)
    ctx.sync()
    ctx.queued()
    ctx.under_test("close()", plan.close, True)

    def bring_up():
        p = neo.fft.FFTPlan(kind, order, batch)
        p.execute_device(dx[1].data_ptr(), out[1].data_ptr(), -1, 0)
        ctx.sync()
        return p
    second = ctx.reuse(bring_up)
    ctx.finish()
    outs = {"queued": _host(out[0]), "second": _host(out[1])}
    second.close()
    truths = {}
    if mode == "serial":
        truths = {"queued": (ref(xs[0]), tol), "second": (ref(xs[1]), tol)}
    return outs, truths, ctx.problems, ctx.host_s


# ---------------------------------------------------------------------------- stream_set overflow
OVERFLOW_STREAMS = 17  # stream_set::kMax + 1


def run_overflow(neo, torch, oracle, case, mode, hold_us):
    """17 streams step one block each on a plain handle, every one ordered after the one before by
    an event, the first held: the 17th note finds the set full, joins the sixteen remembered
    streams and starts over with the 17th. Then that stream is held, steps once more, and close()
    has to wait for it."""
    P, N = 9, OVERFLOW_STREAMS
    _, _, H1, H2, sig = dense_problem(oracle, P, DENSE_HANDLES["a"][3] + 16)
    sig = sig[:, :(N + 1) * B]
    method = "upols"
    make = lambda: neo.UpolsConvolver(C, B, P, method=method)  # noqa: E731
    conv = make()
    conv.filter(H1)
    conv.set_batch(False)
    x = torch.from_numpy(sig.copy()).cuda()
    y = torch.full_like(x, 7.0)
    streams = [torch.cuda.Stream() for _ in range(N)]
    ctx = Ctx(neo, torch, mode, hold_us)
    ctx.start(streams[0])
    prev = None
    for t in range(N - 1):
        if prev is not None:
            streams[t].wait_event(prev)
        _steps(conv, x, y, t, 1, streams[t].cuda_stream)
        prev = torch.cuda.Event()
        prev.record(streams[t])
        ctx.sync()
    ctx.queued(streams[N - 2])
    streams[N - 1].wait_event(prev)
    ctx.under_test("the 17th stream's step (the full set is joined)",
                   lambda: _steps(conv, x, y, N - 1, 1, streams[N - 1].cuda_stream), True)
    ctx.start(streams[N - 1])
    _steps(conv, x, y, N, 1, streams[N - 1].cuda_stream)
    ctx.sync()
    ctx.queued(streams[N - 1])
    ctx.under_test("close() after the set started over", conv.close, True)
    second, y2 = _second_dense(ctx, make, H2, x)
    ctx.finish()
    outs = {"queued": _host(y), "second": _host(y2)}
    second.close()
    truths = {}
    if mode == "serial":
        truths = {"queued": (_conv_ref(oracle, (P, method, "q", N + 1), sig, H1, method), F32_TOL),
                  "second": (_conv_ref(oracle, (P, method, "second"), sig[:, :2 * B], H2, method), F32_TOL)}
    return outs, truths, ctx.problems, ctx.host_s


# ------------------------------------------------------------------------------------ every case
def _id(*parts):
    return "-".join(str(p) for p in parts)


CASES = ([(_id("dense", *c), run_dense, c) for c in DENSE_CASES] +
         [(_id("sparse", *c), run_sparse, c) for c in SPARSE_CASES] +
         [(_id("f64", *c), run_f64, c) for c in F64_CASES] +
         [(_id("matrix", c[0], f"P{c[1]}", c[2]), run_matrix, c) for c in MATRIX_CASES] +
         [(_id("overlap", c), run_overlap, c) for c in OVERLAP_CASES] +
         [(_id("fft", *c), run_fft, c) for c in FFT_CASES] +
         [("stream-set-overflow", run_overflow, None)])
