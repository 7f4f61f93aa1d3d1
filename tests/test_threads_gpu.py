"""The thread and stream contract of include/neo_hip.h ("Threads and streams"), held on the device.

Every test follows one recipe: the expected outputs are computed serially first, with the same
calls on fresh objects, and pinned to the oracle at the project's bar (peak-normalized 1e-5;
1e-12 for the double plans; the float64 restatement of perceptual_common for the perceptual
predicate); then the same calls run from eight host threads at once (or on two streams) and every
result must equal its serial one bit for bit. Bit equality between repeated runs is the project's
own claim (the reset, sparse, group and latency-mode tests assert it between handles), so a
difference here means that a call saw another call's data or state.

What is contended: the device-memory pool and its one mutex (dmem.hip), the four shared blocking
streams per device (the fifth live handle shares a stream with the first), the shared twiddle
tables, the per-thread null_join event, the page-lock table of the groups (upols_group.hip) and the
Python plan cache (neo/fft/_plan.py), which hands ONE plan to every thread that transforms the same
shape: neo_hip_fft_execute_host stages through the plan's single pair of device buffers, and a
multi-pass plan (inner order above 12) has one set of scratch buffers for all its executes. The
library serialises both (the plan's mutex, and an event between executes on different streams;
fft.hip).

Not here, on purpose: latency mode (set_persistent). A resident spinning kernel per handle plus
spinning host threads is a poor thing to multiply on a shared machine, and nothing above needs it.

run_threads and same_bits are the harness; tests/test_threads.py shows without a GPU that they
bite."""
import functools
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import perceptual_common as pc
from conftest import peak_err
from test_io_contract_gpu import _maker, _per_block, assert_same_bits, problem

pytestmark = pytest.mark.gpu
TOL = 1e-5
TOL64 = 1e-12  # complex<double> plans, as in test_fft_gpu.py
N_THREADS = 8  # fixed: nothing here is sized by os.cpu_count()
JOIN_TIMEOUT = 120.0
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")


# ------------------------------------------------------------------ the harness (no GPU needed)
def run_threads(workers, n_threads=None, timeout=JOIN_TIMEOUT):
    """Run the workers at the same time, one thread each, released together by a barrier; returns
    their return values in order and re-raises the first worker's exception (by index). `workers`:
    a list of callables taking nothing, or one callable that is called with its thread index in
    range(n_threads). A worker still running `timeout` seconds after the start fails the call
    (the threads are daemons: a stuck one does not keep the interpreter alive)."""
    if callable(workers):
        workers = [functools.partial(workers, i) for i in range(n_threads)]
    n = len(workers) if n_threads is None else n_threads
    assert len(workers) == n and 1 <= n <= N_THREADS, (len(workers), n)
    barrier = threading.Barrier(n)
    results, errors = [None] * n, [None] * n

    def body(i):
        try:
            barrier.wait(timeout)
            results[i] = workers[i]()
        except BaseException as e:  # noqa: BLE001 (handed to the caller's thread)
            errors[i] = e

    threads = [threading.Thread(target=body, args=(i,), daemon=True, name=f"worker-{i}") for i in range(n)]
    deadline = time.monotonic() + timeout
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    stuck = [t.name for t in threads if t.is_alive()]
    if stuck:
        raise AssertionError(f"still running after {timeout:g} s: {', '.join(stuck)}")
    for e in errors:
        if e is not None:
            raise e
    return results


def same_bits(got, want, what):
    """Arrays of any dtype equal bit for bit (shape and dtype too); names the first element that
    differs. float32 [C][n] goes through assert_same_bits (channel and column named)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype == np.float32 and got.ndim == 2:
        assert_same_bits(got, want, what)
        return
    size = got.dtype.itemsize
    bad = (got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8)).reshape(-1, size).any(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at flat index {i}: "
                             f"{got.reshape(-1)[i]!r} != {want.reshape(-1)[i]!r}")


def check_results(results, want, what):
    """results[i] (one array, or a list of arrays from repeated rounds) against want[i], bit for
    bit; the worker's index is named."""
    assert len(results) == len(want), what
    for i, (r, w) in enumerate(zip(results, want)):
        for k, a in enumerate(r if isinstance(r, (list, tuple)) else [r]):
            same_bits(a, w, f"{what}: worker {i}, round {k}")


# ------------------------------------------------------------------ FFT
def _cnoise(oracle, seed, shape, dtype=np.complex64):
    n = int(np.prod(shape))
    return oracle.noise(seed, 2 * n).view(np.complex64).reshape(shape).astype(dtype)


def _rnoise(oracle, seed, shape):
    return oracle.noise(seed, int(np.prod(shape))).reshape(shape)


#          make input                                        the call                                      the oracle                                   bar
FACADE = {
    "fft-c64": (lambda o, s: _cnoise(o, s, (4, 1024)), lambda neo, x: neo.fft.fft(x), lambda o, x: o.fft(x, -1), TOL),
    "ifft-c64": (lambda o, s: _cnoise(o, s, (4, 1024)), lambda neo, x: neo.fft.ifft(x, norm="forward"),
                 lambda o, x: o.fft(x, +1), TOL),
    "rfft-f32": (lambda o, s: _rnoise(o, s, (4, 1024)), lambda neo, x: neo.fft.rfft(x), lambda o, x: o.rfft(x), TOL),
    "irfft-c64": (lambda o, s: _cnoise(o, s, (4, 513)), lambda neo, x: neo.fft.irfft(x, 1024, norm="forward"),
                  lambda o, x: o.irfft(x, 1024), TOL),
    "fft-c128": (lambda o, s: _cnoise(o, s, (2, 256), np.complex128), lambda neo, x: neo.fft.fft(x),
                 lambda o, x: o.fft_f64(x, -1), TOL64),
    "fft-c64-order13": (lambda o, s: _cnoise(o, s, (2, 8192)), lambda neo, x: neo.fft.fft(x), lambda o, x: o.fft(x, -1),
                        TOL),
}


@pytest.mark.parametrize("kind", list(FACADE))
def test_fft_facade_from_threads(neo_gpu, oracle, kind):
    """neo.fft is re-entrant: 8 threads x 100 calls on the SAME shape (so the same cached plan and
    its one pair of staging buffers; order 13 also its scratch), each thread its own data. Every
    one of the 800 results equals the thread's serial result bit for bit."""
    make, call, ref, tol = FACADE[kind]
    xs = [make(oracle, 9100 + 17 * i) for i in range(N_THREADS)]
    serial = [call(neo_gpu, x) for x in xs]
    for x, y in zip(xs, serial):
        err = peak_err(y, ref(oracle, x))
        assert err <= tol, (kind, err)
    for a in xs + serial:
        a.setflags(write=False)

    def worker(i):
        for r in range(100):
            same_bits(call(neo_gpu, xs[i]), serial[i], f"{kind}: thread {i}, call {r}")
        return 100

    assert run_threads(worker, N_THREADS) == [100] * N_THREADS


def test_one_plan_many_threads_c_abi(neo_gpu, oracle):
    """One plan executed from several threads (neo_hip.h): an LDS-path plan (order 10, batch 4) and
    the smallest multi-pass plan (order 13, batch 2), both shared by 8 threads that call
    neo_hip_fft_execute_host directly, 100 rounds each on their own arrays."""
    C2C = neo_gpu._native.C2C
    shapes = {10: (4, 1024), 13: (2, 8192)}
    xs = {o: [_cnoise(oracle, 9300 + 31 * i + o, shp) for i in range(N_THREADS)] for o, shp in shapes.items()}
    serial = {}
    for o, shp in shapes.items():
        plan = neo_gpu.fft.FFTPlan(C2C, o, shp[0])
        serial[o] = []
        for x in xs[o]:
            y = np.empty_like(x)
            plan.execute_host(x, y, -1)
            assert peak_err(y, oracle.fft(x, -1)) <= TOL
            serial[o].append(y)
        plan.close()
    plans = {o: neo_gpu.fft.FFTPlan(C2C, o, shp[0]) for o, shp in shapes.items()}

    def worker(i):
        out = {o: np.empty_like(xs[o][i]) for o in shapes}
        for r in range(100):
            for o in shapes:
                out[o].fill(0)
                plans[o].execute_host(xs[o][i], out[o], -1)
                same_bits(out[o], serial[o][i], f"order {o}: thread {i}, round {r}")
        return 100

    try:
        assert run_threads(worker, N_THREADS) == [100] * N_THREADS
    finally:
        for p in plans.values():
            p.close()


def _device_bits(torch, t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


@pytest.mark.parametrize("kind,order,batch", [("c2c", 13, 256), ("r2c", 14, 256)])
def test_one_multipass_plan_two_streams(neo_gpu, oracle, kind, order, batch):
    """One multi-pass plan executed on two streams with no host synchronisation in between: 20
    rounds of "input a on s1, input b on s2", one synchronisation at the end, all 40 outputs equal
    to the serial ones bit for bit. The c2c plan of order 13 ping-pongs through two scratch buffers,
    the r2c plan of order 14 (inner order 13) through three.

    Before the plan kept an event between its executes, nothing ordered them: run_c2c_global
    (fft.hip) writes pass i of every execute into the plan's d_scratch[i & 1], and the r2c path its
    inner transform into d_scratch[2], whichever stream the execute is on, so the first pass of the
    execute on s2 overwrote d_scratch[0] while the second pass of the execute on s1 was still
    reading it. Nobody has measured how often that race is lost on an MI355X (it needs the two
    streams' kernels to overlap); that it is a race is read from the code, not from a failing run."""
    torch = pytest.importorskip("torch")
    n = 1 << order
    K = neo_gpu._native.C2C if kind == "c2c" else neo_gpu._native.R2C
    if kind == "c2c":
        xs = [_cnoise(oracle, 9500 + k, (batch, n)) for k in range(2)]
        refs = [oracle.fft(x, -1) for x in xs]
        out_shape, out_dtype = (batch, n), torch.complex64
    else:
        xs = [_rnoise(oracle, 9600 + k, (batch, n)) for k in range(2)]
        refs = [oracle.rfft(x) for x in xs]
        out_shape, out_dtype = (batch, n // 2 + 1), torch.complex64
    dx = [torch.from_numpy(x).cuda() for x in xs]
    want = []
    plan = neo_gpu.fft.FFTPlan(K, order, batch)  # serial: a fresh plan, one stream, a sync after every execute
    for k in range(2):
        o = torch.empty(out_shape, dtype=out_dtype, device="cuda")
        plan.execute_device(dx[k].data_ptr(), o.data_ptr(), -1, 0)
        torch.cuda.synchronize()
        err = peak_err(o.cpu().numpy(), refs[k])
        assert err <= TOL, (kind, k, err)
        want.append(_device_bits(torch, o))
    plan.close()

    plan = neo_gpu.fft.FFTPlan(K, order, batch)
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros(out_shape, dtype=out_dtype, device="cuda") for _ in range(40)]
    torch.cuda.synchronize()  # inputs and zeroed outputs are there before the streams start
    for r in range(20):
        for k in range(2):
            plan.execute_device(dx[k].data_ptr(), outs[2 * r + k].data_ptr(), -1, s[k].cuda_stream)
    torch.cuda.synchronize()
    plan.close()
    for j, o in enumerate(outs):
        if not torch.equal(_device_bits(torch, o), want[j % 2]):
            same_bits(o.cpu().numpy(), want[j % 2].cpu().numpy().view(np.complex64).reshape(out_shape),
                      f"{kind} order {order}: round {j // 2}, stream {j % 2}")
            raise AssertionError(f"{kind} order {order}: round {j // 2}, stream {j % 2} differs")


# ------------------------------------------------------------------ convolvers, one per thread
def _device_run(torch, make, drive, sig, finish=None):
    """create -> filter -> run on a device copy of sig (null stream) -> close"""
    conv = make()
    t = torch.from_numpy(np.array(sig, dtype=np.float32)).cuda()
    n = sig.shape[1]
    drive(conv, t.data_ptr(), n, t.data_ptr(), n)
    if finish:
        finish(conv)
    torch.cuda.synchronize()
    out = t.cpu().numpy()
    conv.close()
    return out


def _convolver_jobs(neo, oracle, torch):
    """[(name, job, reference)]: job() brings a handle up, runs the path and tears it down;
    every path at its smallest shape."""
    from test_sparse_gpu import masks
    from test_upols_gpu import _v2_reference

    jobs = []

    # plain step, the launch pair and the fused kernel, device buffers
    C, B, P, nb = 2, 64, 12, 40
    parts, sig, ref = problem(oracle, C, B, P, nb)

    def plain(parts=parts, sig=sig, C=C, B=B, P=P, nb=nb):
        outs = []
        for fused in (0, 1):
            def setup(conv):
                assert not conv.ahead_info()[0]
            make = _maker(neo, C, B, P, parts, options={"levels": 0, "fused": fused}, setup=setup)
            outs.append(_device_run(torch, make, _per_block(B, nb), sig))
        return np.concatenate(outs)
    jobs.append(("plain step", plain, np.concatenate([ref, ref])))

    # host buffers: pinned staging from the shared pinned chunks, five blocks per call
    C, B, P, nb = 2, 128, 9, 30
    parts, sig, ref = problem(oracle, C, B, P, nb)

    def host(parts=parts, sig=sig, C=C, B=B, P=P, nb=nb):
        conv = _maker(neo, C, B, P, parts)()
        out = np.concatenate([conv.process(np.ascontiguousarray(sig[:, a:a + 5 * B]))
                              for a in range(0, nb * B, 5 * B)], axis=1)
        conv.close()
        return out
    jobs.append(("host process", host, ref))

    # streaming levels: Toeplitz levels in one launch per step; the far level stored, its slices on
    # the background stream (step groups of 4); the far level recomputed
    for name, C, B, P, nb, opts, form, sg in (("toeplitz levels", 2, 32, 70, 200, {"step_group": 1}, 0, 1),
                                              ("far level stored", 2, 16, 257, 654, {"far_level": 1, "step_group": 4}, 1, 4),
                                              ("far level recomputed", 2, 32, 257, 654,
                                               {"far_level": 2, "step_group": 1}, 2, 1)):
        parts, sig, ref = problem(oracle, C, B, P, nb)

        def levels(parts=parts, sig=sig, C=C, B=B, P=P, nb=nb, opts=opts, form=form, sg=sg):
            def setup(conv):
                assert conv.ahead_info()[0] and conv.step_group() == sg and conv.far_form() == form
            make = _maker(neo, C, B, P, parts, options=dict(opts, levels=1), setup=setup)
            return _device_run(torch, make, _per_block(B, nb), sig, finish=lambda conv: conv.join_background(None))
        jobs.append((name, levels, ref))

    # batched passes of falling size, then single blocks: one process_blocks call
    C, B, P, nb = 2, 16, 7, 37
    parts, sig, ref = problem(oracle, C, B, P, nb)

    def batched(parts=parts, sig=sig, C=C, B=B, P=P):
        conv = _maker(neo, C, B, P, parts)()
        assert conv.batch_info()[0] > 1
        t = torch.from_numpy(np.array(sig)).cuda()
        conv.process_blocks(t)
        torch.cuda.synchronize()
        out = t.cpu().numpy()
        conv.close()
        return out
    jobs.append(("batched process_blocks", batched, ref))

    # upola_v2, ragged sample counts (host I/O), the pieces of test_upola_v2_pieces_vs_oracle
    C, B, L = 2, 64, 64
    ir = np.stack([oracle.noise(180 + c, L) for c in range(C)])
    v2parts = oracle.uniform_partition(oracle.normalize_impulse(ir), B)
    N = B * 9
    v2sig = np.stack([oracle.noise(190 + c, N) for c in range(C)])
    cuts = sorted({0, 1, B // 2 + 1, B + B // 2 + 1, 3 * B + 1, 4 * B + 1, 4 * B + 2, 6 * B, 8 * B, N})

    def v2(C=C, B=B):
        conv = neo.UpolsConvolver(C, B, v2parts.shape[1], method="upola_v2")
        conv.filter(v2parts)
        out = np.concatenate([conv.process(np.ascontiguousarray(v2sig[:, a:b])) for a, b in zip(cuts[:-1], cuts[1:])],
                             axis=1)
        conv.close()
        return out
    jobs.append(("upola_v2 pieces", v2, _v2_reference(oracle, v2parts, v2sig, cuts)))

    # sparse step on tile-compacted filters
    C, B, P, nb = 2, 16, 7, 60
    parts, sig, _ = problem(oracle, C, B, P, nb)
    mask = masks(C, B, P)["bernoulli-0.5"]

    def sparse(parts=parts, sig=sig, C=C, B=B, P=P, nb=nb, mask=mask):
        def make():
            conv = neo.SparseUpolsConvolver(C, B, P)
            conv.filter(parts, mask)
            return conv
        return _device_run(torch, make, _per_block(B, nb), sig)
    jobs.append(("sparse step", sparse, oracle.dense_convolve(sig, (parts * mask).astype(np.complex64))))
    return jobs


def test_distinct_convolvers_from_threads(neo_gpu, oracle):
    """Distinct handles need no locking by the caller: eight threads, each owning another step path,
    three rounds of create -> filter -> run -> close each, so that bring-up and teardown in one
    thread overlap running kernels of the others, pool ranges change owners and (more than four
    handles alive) the shared streams are shared across threads. Every round of every path equals
    that path's serial run bit for bit."""
    torch = pytest.importorskip("torch")
    jobs = _convolver_jobs(neo_gpu, oracle, torch)
    assert len(jobs) == N_THREADS
    want = []
    for name, job, ref in jobs:
        y = job()
        err = peak_err(y, ref)
        print(f"{name}: serial vs oracle {err:.3g}")
        assert err <= TOL, (name, err)
        want.append(y)
    results = run_threads([functools.partial(lambda job: [job() for _ in range(3)], job) for _, job, _ in jobs])
    for (name, _, _), r, w in zip(jobs, results, want):
        check_results([r], [w], name)


def test_distinct_multi_device_convolvers_from_threads(neo_gpu, oracle):
    """Two multi-device convolvers in two threads (three and two shards on device 0, so each call
    fans out over shard threads of its own inside the library as well): three rounds of create ->
    filter -> three process calls of four blocks -> close, bit-equal to the serial run."""
    B, P, nb = 128, 10, 12
    shapes = [(7, [0, 0, 0]), (5, [0, 0])]
    probs = [problem(oracle, C, B, P, nb) for C, _ in shapes]

    def job(k):
        C, devices = shapes[k]
        parts, sig, _ = probs[k]
        m = neo_gpu.UpolsMultiConvolver(C, B, P, devices)
        m.filter(parts)
        out = np.concatenate([m.process(sig[:, a:a + 4 * B]) for a in range(0, nb * B, 4 * B)], axis=1)
        m.close()
        return out

    want = []
    for k in range(2):
        y = job(k)
        err = peak_err(y, probs[k][2])
        assert err <= TOL, (k, err)
        want.append(y)
    results = run_threads(lambda k: [job(k) for _ in range(3)], 2)
    check_results(results, want, "multi-device convolver")


# ------------------------------------------------------------------ one-shot entry points
def _one_shot_jobs(neo, oracle):
    """[(name, job, check)]: job() -> array; check(array) holds the serial result to the oracle"""
    jobs = []

    def bar(ref):
        def check(y):
            err = peak_err(y, ref)
            assert err <= TOL, err
        return check

    ir = np.stack([oracle.noise(9700 + c, 1000) for c in range(2)])
    jobs.append(("uniform_partition", lambda: neo.uniform_partition(ir, 128), bar(oracle.uniform_partition(ir, 128))))

    ir17 = np.stack([oracle.noise(9720 + c, 4801) for c in range(17)])
    jobs.append(("normalize_impulse", lambda: neo.normalize_impulse(ir17.copy()), bar(oracle.normalize_impulse(ir17))))

    sig, patch = oracle.noise(9740, 555), oracle.noise(9741, 10)
    jobs.append(("fft_convolve", lambda: neo.fft_convolve(sig, patch), bar(oracle.fft_convolve(sig, patch))))
    jobs.append(("direct_convolve", lambda: neo.direct_convolve(sig, patch), bar(oracle.direct_convolve(sig, patch))))

    x = np.stack([oracle.noise(9760 + c, 5000) for c in range(2)])
    jobs.append(("stft", lambda: neo.fft.stft(x, 300, 512, 100), bar(oracle.stft(x, 300, 512, 100, oracle.hann(512)))))

    C, B, P = pc.SHAPES[2]
    parts = neo.uniform_partition(neo.normalize_impulse(pc.impulse(C, B, P)), B)  # the device's own partitions
    sp = neo.PerceptualSparsity(pc.SAMPLE_RATE, -40.0, 2, "a")
    lv, exact = pc.levels64(parts, pc.weights64(B, pc.SAMPLE_RATE, 2, "a"))
    tl, texact = pc.tile_levels64(lv, exact)

    def check_hist(h):
        pc.check_hist(h[0], lv, exact, P * (B + 1), lv.size, "bins")
        pc.check_hist(h[1], tl, texact, P * (B // 16), lv.size, "tiles")

    jobs.append(("perceptual_mask", lambda: neo.perceptual_mask(parts, sp),
                 lambda m: pc.check_mask(m, lv, exact, -40.0, "mask")))

    def hist():
        h = neo.perceptual_histogram(parts, sp)
        return np.stack([h["bins"], h["tiles"]])
    jobs.append(("perceptual_histogram", hist, check_hist))

    Cs, Bs, F, nb = 2, 128, 129, 12
    n = oracle.overlap_transform_size(Bs, F)
    G = np.fft.rfft(np.concatenate([oracle.noise(9780, F), np.zeros(n - F, np.float32)]).astype(np.float64)
                    ).astype(np.complex64)
    xs = np.stack([oracle.noise(9790 + c, Bs * nb) for c in range(Cs)])

    def overlap():
        stage = neo.OverlapStage("save", Cs, Bs, F)
        out = xs.copy()
        for t in range(nb):
            blk = np.ascontiguousarray(out[:, t * Bs:(t + 1) * Bs])
            spec = stage.forward(blk)
            spec *= G
            stage.inverse(spec, blk)
            out[:, t * Bs:(t + 1) * Bs] = blk
        stage.close()
        return out
    jobs.append(("overlap stage", overlap, bar(np.stack([oracle.overlap_stage("save", xs[c], Bs, F, G) for c in range(Cs)]))))
    return jobs


def test_one_shots_from_threads(neo_gpu, oracle):
    """The one-shot entry points are re-entrant: each of eight threads loops 30 times over its own
    one (each allocates, launches on a shared stream and frees), and every result equals the serial
    one bit for bit."""
    jobs = _one_shot_jobs(neo_gpu, oracle)
    assert len(jobs) == N_THREADS
    want = []
    for name, job, check in jobs:
        y = job()
        check(y)
        want.append(y)

    def worker(i):
        name, job, _ = jobs[i]
        for r in range(30):
            same_bits(job(), want[i], f"{name}: call {r}")
        return 30

    assert run_threads(worker, N_THREADS) == [30] * N_THREADS


# ------------------------------------------------------------------ groups
def _page_aligned(rows, cols):
    """a zeroed C-contiguous float32 [rows][cols] array that starts a 4 KiB page and shares none"""
    words = rows * cols
    raw = np.zeros((words + 1023) // 1024 * 1024 + 2048, np.float32)
    skip = (-raw.ctypes.data % 4096) // 4
    a = raw[skip:skip + words].reshape(rows, cols)
    assert a.ctypes.data % 4096 == 0 and a.flags.c_contiguous and a.base is not None  # the view keeps raw alive
    return a


@pytest.mark.parametrize("shared_range", [False, True])
@pytest.mark.parametrize("P", [7, 70])
def test_two_groups_from_threads(neo_gpu, oracle, P, shared_range):
    """A group is for one thread at a time, but two groups may run in two threads: each its own
    UpolsGroup(16, P) with four members and its own registered frame, 12 frames in the plugin's
    pattern. With shared_range group 1 also registers group 0's frame (an owner registers its
    buffer with the group of every shape it holds): the page-lock table counts the range, so
    group 1's unregister at close does not take the lock away under group 0's in-place reads. Only
    group 0's members live in that range. The two frames lie in pages of their own (an allocator may
    put two 256-byte arrays into one page; whose page lock that is when the ranges' registrations
    end at different times is the driver's business, not this test's).

    P = 70: the members run the streaming levels, the groups coalesce after three frames (one
    launch per frame on the shared handle, the frame read in place) and both report `coalesced`.
    P = 7 (plain step): a group only coalesces members that run the streaming levels
    (call_independent, upols_group.hip: 64 partitions and up), so these two stay in independent
    mode, every member on its own handle on its group's stream, and report that."""
    B, M, nf = 16, 4, 12
    parts, sigs = [], []
    for k in range(2):
        ir = np.stack([oracle.noise(9800 + 10 * k + c, B * P) for c in range(M)])
        parts.append(oracle.uniform_partition(oracle.normalize_impulse(ir), B))
        sigs.append(np.stack([oracle.noise(9850 + 10 * k + c, B * nf) for c in range(M)]))
    frames = [_page_aligned(M, B) for _ in range(2)]

    def job(k, also=None):
        g = neo_gpu.UpolsGroup(B, P)
        ids = [g.join() for _ in range(M)]
        for i, c in zip(ids, range(M)):
            g.filter(i, parts[k][c])
        frame = frames[k]
        g.register(frame)
        if also is not None:
            g.register(also)
        out = np.empty_like(sigs[k])
        for f in range(nf):
            frame[:] = sigs[k][:, f * B:(f + 1) * B]
            for c in range(M):
                g(ids[c], frame[c])
            out[:, f * B:(f + 1) * B] = frame
        st = g.stats()
        g.close()
        return out, st

    want = []
    for k in range(2):
        y, st = job(k)
        assert st["coalesced"] == (P >= 64), st
        err = peak_err(y, oracle.dense_convolve(sigs[k], parts[k]))
        assert err <= TOL, (k, err)
        want.append(y)
    results = run_threads([functools.partial(job, 0), functools.partial(job, 1, frames[0] if shared_range else None)])
    for k, (y, st) in enumerate(results):
        assert st["coalesced"] == (P >= 64), (k, st)
    check_results([y for y, _ in results], want, "group")


# ------------------------------------------------------------------ the C++ header API
def test_cpp_threads_on_gpu():
    """tests/cpp/test_threads.cpp: eight std::threads, each with its own fft_plan (order 10) and
    upols_multichannel, all sharing one fft_plan of order 13; 100 rounds against serial results by
    memcmp."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "liboracle.so"])
    subprocess.check_call(["make", "-s", "-C", CPP, "bin/test_threads"])
    r = subprocess.run([os.path.join(CPP, "bin", "test_threads")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "thread test passed" in r.stdout
