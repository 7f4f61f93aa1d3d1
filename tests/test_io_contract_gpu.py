"""The I/O contract of the convolver's process calls (include/neo_hip.h): channel c is read at
in + c*ld_in and written at out + c*ld_out, in == out is allowed, the input is left as it was
and nothing outside [c*ld_out, c*ld_out + n) is written. The value tests of this suite run in
place on contiguous buffers; here every step path also runs with separate, padded buffers of
different strides (B) and in place inside one padded buffer (B'), and must give the bits of the
contiguous in-place run (A), which is pinned to the oracle.

The buffers are arenas of C + 2 rows of ld words filled with a sentinel bit pattern: the channels
live in rows 1..C, rows 0 and C + 1 are guards, so an access up to one channel stride before or
after the channels stays inside the allocation and shows up as a changed sentinel (a write) or
as a NaN in the output (a read: the input sentinel is a quiet NaN), never as a fault."""
import numpy as np
import pytest

from conftest import peak_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
IN_FILL = 0x7FC0BEEF   # a quiet NaN with a payload: a padding or guard word that reaches a sum poisons it
OUT_FILL = 0x7FD1CAFE  # another one, so a copy of input padding into output padding shows too
PAD_IN, PAD_OUT = 36, 4  # ld_in = n + 36, ld_out = n + 4: multiples of 4 that differ


# ------------------------------------------------------------------ the harness (numpy only)
def _host_arena(C, ld, fill_bits, x=None):
    a = np.full((C + 2, ld), fill_bits, dtype=np.int32)
    if x is not None:
        a.view(np.float32)[1:C + 1, :x.shape[1]] = x
    return a


def _where(bad, C, n, side):
    r, c = (int(v) for v in np.argwhere(bad)[0])
    region = "guard row" if r in (0, C + 1) else "padding" if c >= n else "payload"
    return f"row {r}, column {c} ({side} {region})"


def check_regions(out_after, C, n, out_fill, in_before=None, in_after=None):
    """Host copies of the arenas as int32 [C + 2][ld] (bit patterns, so NaNs compare):
    (a) the input arena equals its copy from before the call bit for bit, (b) every word of the
    output arena outside columns [0, n) of rows 1..C still holds the sentinel; returns (c) the
    output payload [C][n] as float32. Raises with the first offending (row, column, region)."""
    for a in (out_after, in_before, in_after):
        assert a is None or (a.dtype == np.int32 and a.ndim == 2 and a.shape[0] == C + 2 and a.shape[1] >= n)
    if in_before is not None:
        bad = in_after != in_before
        if bad.any():
            raise AssertionError("the call changed its input at " + _where(bad, C, n, "input"))
    bad = out_after != np.int32(out_fill)
    bad[1:C + 1, :n] = False
    if bad.any():
        raise AssertionError("the call wrote outside its output at " + _where(bad, C, n, "output"))
    return np.ascontiguousarray(out_after[1:C + 1, :n]).view(np.float32)


def assert_same_bits(got, want, what):
    """float32 [C][n] arrays equal bit for bit; names the first (channel, column) that differs."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    bad = np.ascontiguousarray(got).view(np.int32) != np.ascontiguousarray(want).view(np.int32)
    if bad.any():
        c, j = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at channel {c}, "
                             f"column {j}: {got[c, j]!r} != {want[c, j]!r}")


# ------------------------------------------------------------------ device / host buffers
def _arena(torch, C, ld, fill_bits):
    """One device tensor of C + 2 rows of ld words holding the sentinel; the library gets the
    pointer of row 1 (base + 4*ld)."""
    return torch.full((C + 2, ld), fill_bits, dtype=torch.int32, device="cuda")


class _Mem:
    """Buffers on one side (device tensors or numpy arrays) behind the same three calls."""

    def __init__(self, torch, host):
        self.torch, self.host = torch, host

    def contiguous(self, x):
        if self.host:
            a = np.ascontiguousarray(x).copy()
            return a, a.ctypes.data
        t = self.torch.from_numpy(np.array(x, dtype=np.float32)).cuda()  # a copy: x may be read-only
        return t, t.data_ptr()

    def arena(self, C, ld, fill_bits, x=None):
        """(arena, pointer of row 1); x [C][n] goes to columns [0, n) of rows 1..C"""
        if self.host:
            a = _host_arena(C, ld, fill_bits, x)
            return a, a.ctypes.data + 4 * ld
        t = _arena(self.torch, C, ld, fill_bits)
        if x is not None:
            t.view(self.torch.float32)[1:C + 1, :x.shape[1]] = self.contiguous(x)[0]
        return t, t.data_ptr() + 4 * ld

    def read(self, buf):
        return buf.copy() if self.host else buf.cpu().numpy()

    def sync(self):
        if not self.host:
            self.torch.cuda.synchronize()


def run_contract(torch, make, drive, x, ref, host=False, pads=(PAD_IN, PAD_OUT), exact=True, finish=None):
    """make() -> a fresh handle; drive(conv, in_ptr, ld_in, out_ptr, ld_out) makes the path's
    call sequence on the null stream. A: in place on a contiguous [C][n] buffer, twice (fresh
    handles; the path must be repeatable), pinned to `ref` at TOL. B: from an input arena of
    stride n + pads[0] into an output arena of stride n + pads[1]. B': in place inside one arena
    of stride n + pads[1]. B and B' pass check_regions and equal A bit for bit (strides move
    addresses only); exact=False (a path whose kernel choice follows the alignment): B and B'
    against `ref` at TOL instead, no A."""
    mem = _Mem(torch, host)
    C, n = x.shape
    ld_in, ld_out = n + pads[0], n + pads[1]

    def go(ip, li, op, lo):
        conv = make()
        drive(conv, ip, li, op, lo)
        if finish:
            finish(conv)
        mem.sync()
        conv.close()

    A = None
    if exact:
        runs = []
        for _ in range(2):
            buf, p = mem.contiguous(x)
            go(p, n, p, n)
            runs.append(mem.read(buf))
        A = runs[0]
        assert_same_bits(runs[1], A, "A is not repeatable")
        err = peak_err(A, ref)
        print(f"A vs oracle: peak err {err:.3g}")
        assert err <= TOL, err

    def judge(payload, what):
        if exact:
            assert_same_bits(payload, A, what)
        else:
            err = peak_err(payload, ref)
            print(f"{what} vs oracle: peak err {err:.3g}")
            assert err <= TOL, (what, err)

    ia, ip = mem.arena(C, ld_in, IN_FILL, x)
    oa, op = mem.arena(C, ld_out, OUT_FILL)
    before = mem.read(ia)
    go(ip, ld_in, op, ld_out)
    judge(check_regions(mem.read(oa), C, n, OUT_FILL, before, mem.read(ia)), "B (separate padded buffers)")
    pa, pp = mem.arena(C, ld_out, IN_FILL, x)
    go(pp, ld_out, pp, ld_out)
    judge(check_regions(mem.read(pa), C, n, IN_FILL), "B' (in place, padded)")


# ------------------------------------------------------------------ problems, made once
_cache = {}


def problem(oracle, C, B, P, nb, method="upols"):
    """filter [C][P][B+1], signal [C][nb B] and the oracle's dense convolution of a shape"""
    key = (C, B, P, nb)
    if key not in _cache:
        ir = np.stack([oracle.noise(8100 + 13 * c + B + P, B * P) for c in range(C)])
        parts = oracle.uniform_partition(oracle.normalize_impulse(ir), B)
        sig = np.stack([oracle.noise(8500 + 13 * c + B + P, B * nb) for c in range(C)])
        parts.setflags(write=False)
        sig.setflags(write=False)
        _cache[key] = (parts, sig)
    parts, sig = _cache[key]
    m = "upols" if method == "upols" else "upola"
    if key + (m,) not in _cache:
        ref = oracle.dense_convolve(sig, parts, method=m)
        ref.setflags(write=False)
        _cache[key + (m,)] = ref
    return parts, sig, _cache[key + (m,)]


def _maker(neo, C, B, P, parts, method="upols", options=None, setup=None):
    def make():
        conv = neo.UpolsConvolver(C, B, P, method=method, options=options)
        conv.filter(parts)
        if setup:
            setup(conv)
        return conv
    return make


def _per_block(B, nb):
    """one block per process_device call"""
    def drive(conv, ip, ld_in, op, ld_out):
        for t in range(nb):
            conv.process_device(ip + 4 * t * B, ld_in, op + 4 * t * B, ld_out, 0)
    return drive


def _samples(cuts, is_device):
    """one process_samples call per piece [cuts[i], cuts[i + 1])"""
    def drive(conv, ip, ld_in, op, ld_out):
        for a, b in zip(cuts[:-1], cuts[1:]):
            conv.process_samples_ptr(ip + 4 * a, ld_in, op + 4 * a, ld_out, b - a, is_device, 0)
    return drive


# ------------------------------------------------------------------ the paths
@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("C,B,P,nb,split", [(3, 16, 7, 20, 0), (2, 1024, 5, 12, 0), (1, 4096, 3, 5, 0),
                                            (2, 128, 50, 130, 12)])
def test_plain_step(neo_gpu, oracle, C, B, P, nb, split, fused, method):
    """k_upols_step (+ k_upols_finish with fused 0) through process_device; with 12 split
    workgroups (6 per channel) the last-arriver tail of the fused step writes `out`."""
    torch = pytest.importorskip("torch")
    parts, sig, ref = problem(oracle, C, B, P, nb, method)

    def setup(conv):
        assert not conv.ahead_info()[0]
        assert split == 0 or conv.splits == 6

    make = _maker(neo_gpu, C, B, P, parts, method, {"levels": 0, "fused": fused, "split_workgroups": split}, setup)
    run_contract(torch, make, _per_block(B, nb), sig, ref)


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb,opts,form", [(2, 32, 70, 200, {"toep_split": 1}, 0),
                                                (2, 32, 70, 200, {"toep_split": 2}, 0),
                                                (2, 32, 257, 654, {"far_level": 0}, 3),
                                                (2, 32, 257, 654, {"far_level": 1}, 1),
                                                (2, 32, 257, 654, {"far_level": 2}, 2), (1, 1024, 70, 150, {}, 0)])
def test_streaming_levels_one_launch_per_step(neo_gpu, oracle, C, B, P, nb, opts, form, method):
    """k_lvl_step: the block and the level slices in one launch, every far form"""
    torch = pytest.importorskip("torch")
    parts, sig, ref = problem(oracle, C, B, P, nb, method)

    def setup(conv):
        assert conv.ahead_info()[0] and conv.step_group() == 1 and conv.far_form() == form

    make = _maker(neo_gpu, C, B, P, parts, method, dict(opts, levels=1, step_group=1), setup)
    run_contract(torch, make, _per_block(B, nb), sig, ref)


@pytest.mark.parametrize("method,G,paced", [("upols", 2, 0), ("upols", 4, 0), ("upols", 8, 0), ("upols", 4, 1),
                                            ("upols", 4, 2), ("upola", 4, 0)])
def test_step_groups_and_paced(neo_gpu, oracle, method, G, paced):
    """the block launch on the caller's stream, the slices of G calls on the background stream
    (whole or in paced pieces); the background is joined before the buffers are read back"""
    torch = pytest.importorskip("torch")
    C, B, P, nb = 2, 32, 257, 654
    parts, sig, ref = problem(oracle, C, B, P, nb, method)

    def setup(conv):
        assert conv.ahead_info()[0] and conv.step_group() == G
        if paced:
            conv.set_paced(paced)

    make = _maker(neo_gpu, C, B, P, parts, method, {"levels": 1, "far_level": 1, "step_group": G}, setup)
    run_contract(torch, make, _per_block(B, nb), sig, ref, finish=lambda conv: conv.join_background(None))


@pytest.mark.parametrize("method", ["upols", "upola", "upola_v2"])
@pytest.mark.parametrize("C,B,P,nb", [(2, 16, 7, 37), (1, 2048, 5, 11)])
def test_batched_passes_and_leftover_blocks(neo_gpu, oracle, method, C, B, P, nb):
    """one process_samples call: batched passes of falling size, then single blocks"""
    torch = pytest.importorskip("torch")
    parts, sig, ref = problem(oracle, C, B, P, nb, method)

    def setup(conv):
        assert conv.batch_info()[0] > 1

    make = _maker(neo_gpu, C, B, P, parts, method, None, setup)
    run_contract(torch, make, _samples([0, nb * B], True), sig, ref)


@pytest.mark.parametrize("method", ["upols", "upola"])
@pytest.mark.parametrize("C,B,P,nb", [(1, 16, 129, 300), (2, 64, 128, 300)])
def test_offline_windows(neo_gpu, oracle, method, C, B, P, nb):
    """one process_samples call of 300 blocks: an offline pass of 256, the rest as usual"""
    torch = pytest.importorskip("torch")
    parts, sig, ref = problem(oracle, C, B, P, nb, method)

    def setup(conv):
        assert conv.offline_info()[0]

    make = _maker(neo_gpu, C, B, P, parts, method, None, setup)
    run_contract(torch, make, _samples([0, nb * B], True), sig, ref)


def _v2_problem(oracle):
    from test_upols_gpu import _v2_reference

    C, B, L = 3, 128, 1000
    if "v2" not in _cache:
        ir = np.stack([oracle.noise(8700 + c, L) for c in range(C)])
        parts = oracle.uniform_partition(oracle.normalize_impulse(ir), B)
        N = B * 9
        sig = np.stack([oracle.noise(8800 + c, N) for c in range(C)])
        cuts = sorted({0, 1, B // 2 + 1, B + B // 2 + 1, 3 * B + 1, 4 * B + 1, 4 * B + 2, 6 * B, 8 * B, N})
        _cache["v2"] = (C, B, parts, sig, cuts, _v2_reference(oracle, parts, sig, cuts))
    return _cache["v2"]


@pytest.mark.parametrize("host,pads,exact", [(False, (36, 4), True), (False, (37, 5), False), (True, (36, 4), True),
                                             (True, (3, 1), True)])
def test_upola_v2_pieces(neo_gpu, oracle, host, pads, exact):
    """sub-block pieces at the cuts of test_upola_v2_pieces_vs_oracle. Aligned strides take the
    kernels of the contiguous run: bit equality. Odd device strides (4-byte aligned pointers) send
    whole blocks through k_upola2_piece too, which need not round like the launch pair: those runs
    are held to the restatement at TOL. Host buffers are staged contiguously: bit equality for any
    stride."""
    torch = pytest.importorskip("torch")
    C, B, parts, sig, cuts, ref = _v2_problem(oracle)
    make = _maker(neo_gpu, C, B, parts.shape[1], parts, "upola_v2")
    run_contract(torch, make, _samples(cuts, not host), sig, ref, host=host, pads=pads, exact=exact)


def test_host_memory_strided_copies(neo_gpu, oracle):
    """process_samples on host memory (the strided copies into and out of the staging buffer):
    five calls of five blocks, ld_in = n + 3, ld_out = n + 1"""
    torch = pytest.importorskip("torch")
    C, B, P, nb = 3, 16, 7, 25
    parts, sig, ref = problem(oracle, C, B, P, nb)
    make = _maker(neo_gpu, C, B, P, parts)
    run_contract(torch, make, _samples(list(range(0, nb * B + 1, 5 * B)), False), sig, ref, host=True, pads=(3, 1))


@pytest.mark.parametrize("method,name", [("upols", "bernoulli-0.1"), ("upola", "empty-rows")])
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("C,B,P,nb", [(2, 16, 7, 60), (2, 512, 70, 120)])
def test_sparse_step(neo_gpu, oracle, C, B, P, nb, fused, method, name):
    """k_sparse_step through process_device, against the dense oracle on the masked filter"""
    torch = pytest.importorskip("torch")
    from test_sparse_gpu import masks

    parts, sig, _ = problem(oracle, C, B, P, nb)
    mask = masks(C, B, P)[name]
    key = ("sparse", C, B, P, nb, name, method)
    if key not in _cache:
        _cache[key] = oracle.dense_convolve(sig, (parts * mask).astype(np.complex64), method=method)

    def make():
        conv = neo_gpu.SparseUpolsConvolver(C, B, P, method=method, options={"fused": fused})
        conv.filter(parts, mask)
        return conv

    run_contract(torch, make, _per_block(B, nb), sig, _cache[key])


def test_multi_device_convolver(neo_gpu, oracle):
    """neo_hip_upols_multi_process_samples offsets every shard's pointers by its first channel's
    c*ld_in / c*ld_out: three shards (2, 2, 3 channels) on host arenas of different strides"""
    torch = pytest.importorskip("torch")
    C, B, P, nb = 7, 128, 10, 12
    parts, sig, ref = problem(oracle, C, B, P, nb)

    def make():
        m = neo_gpu.UpolsMultiConvolver(C, B, P, [0, 0, 0])
        m.filter(parts)
        return m

    def drive(m, ip, ld_in, op, ld_out):
        m.process_samples_ptr(ip, ld_in, op, ld_out, nb * B)

    run_contract(torch, make, drive, sig, ref, host=True)


# ------------------------------------------------------------------ latency mode
def _blocks(conv, p, ld, B, nb, stream, per_call=1):
    for i in range(0, nb, per_call):
        conv.process_blocks_ptr(p + 4 * i * B, p + 4 * i * B, ld, min(per_call, nb - i), stream)


@pytest.mark.parametrize("C,B,P,levels", [(4, 64, 100, True), (4, 512, 40, False), (1, 64, 100, True),
                                          (1, 512, 40, False)])
def test_latency_mode_stride_change(neo_gpu, oracle, C, B, P, levels):
    """The persistent kernel is launched with the caller's channel strides (k_lvl_persist with the
    streaming levels, k_plain_persist without): 10 blocks contiguous in place, 10 from a padded
    input arena into a padded output arena of another stride, 10 contiguous again. With several
    channels the kernel is relaunched exactly once at each change of stride and never otherwise;
    one channel has no stride, so nothing relaunches. All 30 blocks equal the normal step bit for
    bit (neo_hip.h). Stream syncs only: a device-wide one would wait for the resident kernel."""
    torch = pytest.importorskip("torch")
    nb = 30
    parts, sig, ref = problem(oracle, C, B, P, nb)
    n = 10 * B
    cur = torch.cuda.current_stream()
    s = cur.cuda_stream
    normal = _maker(neo_gpu, C, B, P, parts, setup=lambda c: c.set_batch(False))()
    assert normal.ahead_info()[0] == levels
    tn, pn = _Mem(torch, False).contiguous(sig)
    _blocks(normal, pn, nb * B, B, nb, s)
    normal.join_background(None)
    cur.synchronize()
    want = tn.cpu().numpy()
    normal.close()
    err = peak_err(want, ref)
    assert err <= TOL, err

    mem = _Mem(torch, False)
    t1, p1 = mem.contiguous(sig[:, :n])
    ia, ip = mem.arena(C, n + PAD_IN, IN_FILL, sig[:, n:2 * n])
    oa, op = mem.arena(C, n + PAD_OUT, OUT_FILL)
    t3, p3 = mem.contiguous(sig[:, 2 * n:])
    before = ia.cpu().numpy()
    cur.synchronize()
    pc = _maker(neo_gpu, C, B, P, parts, setup=lambda c: c.set_batch(False))()
    pc.set_persistent(True, idle_ms=3000.0)  # no idle relaunch between the phases
    launches = [pc.persistent_info()["launches"]]

    def mark():
        launches.append(pc.persistent_info()["launches"])

    _blocks(pc, p1, n, B, 1, s)
    mark()
    _blocks(pc, p1 + 4 * B, n, B, 9, s)
    mark()
    pc.process_device(ip, n + PAD_IN, op, n + PAD_OUT, s)
    mark()
    for i in range(1, 10):
        pc.process_device(ip + 4 * i * B, n + PAD_IN, op + 4 * i * B, n + PAD_OUT, s)
    mark()
    _blocks(pc, p3, n, B, 1, s)
    mark()
    _blocks(pc, p3 + 4 * B, n, B, 9, s, per_call=3)
    mark()
    pc.set_persistent(False)  # the kernel leaves before the buffers are read back
    cur.synchronize()
    steps = [b - a for a, b in zip(launches[:-1], launches[1:])]
    assert steps == ([1, 0, 1, 0, 1, 0] if C > 1 else [1, 0, 0, 0, 0, 0]), launches
    mid = check_regions(oa.cpu().numpy(), C, n, OUT_FILL, before, ia.cpu().numpy())
    got = np.concatenate([t1.cpu().numpy(), mid, t3.cpu().numpy()], axis=1)
    pc.close()
    assert_same_bits(got, want, "latency mode vs the normal step")


# ------------------------------------------------------------------ refusals
def test_refusals_do_not_advance_state(neo_gpu, oracle):
    """Every misuse of the strides and alignments is refused on the host (NeoHipError; no kernel is
    launched), and the stream then continues on the same handle as if the bad calls had not been
    made: bit-equal to a handle that never saw them. Every pointer of a refused call still lies
    inside the arena."""
    torch = pytest.importorskip("torch")
    C, B, P, nb = 2, 16, 7, 12
    parts, sig, ref = problem(oracle, C, B, P, nb)
    n, ld = nb * B, nb * B + 4
    mem = _Mem(torch, False)
    Err = neo_gpu._native.NeoHipError
    outs = []
    for bad in (False, True):
        conv = _maker(neo_gpu, C, B, P, parts)()
        a, p = mem.arena(C, ld, IN_FILL, sig)

        def refused(call, *args):
            if bad:
                with pytest.raises(Err):
                    call(*args)

        refused(conv.process_device, p + 4, ld, p, ld, 0)      # in + 4 bytes
        refused(conv.process_device, p, ld, p + 8, ld, 0)      # out + 8 bytes
        refused(conv.process_device, p, B + 2, p, ld, 0)       # ld_in = B + 2
        refused(conv.process_device, p, ld, p, B - 4, 0)       # ld_out < B
        for t in range(4):
            conv.process_device(p + 4 * t * B, ld, p + 4 * t * B, ld, 0)
        q = p + 4 * 4 * B
        refused(conv.process_blocks_ptr, q, q, ld + 1, 4, 0)   # ld & 3
        refused(conv.process_blocks_ptr, q, q, 4 * B - 4, 4, 0)  # ld < nb * B
        conv.process_blocks_ptr(q, q, ld, 4, 0)
        q = p + 4 * 8 * B
        refused(conv.process_samples_ptr, q, ld, q, ld, B + 4, True, 0)      # n % B != 0 on a upols handle
        refused(conv.process_samples_ptr, q, B, q, ld, 2 * B, True, 0)       # ld_in < n
        refused(conv.process_samples_ptr, q + 4, ld, q, ld, 2 * B, True, 0)  # unaligned device input
        conv.process_samples_ptr(q, ld, q, ld, 4 * B, True, 0)
        torch.cuda.synchronize()
        outs.append(check_regions(a.cpu().numpy(), C, n, IN_FILL))
        conv.close()
    assert peak_err(outs[0], ref) <= TOL
    assert_same_bits(outs[1], outs[0], "after refused calls")


def test_latency_mode_refuses_unaligned_io(neo_gpu, oracle):
    """latency mode takes whole 16-byte aligned blocks: the refusal comes before a record is
    written, and the blocks after it equal the normal step's bit for bit"""
    torch = pytest.importorskip("torch")
    C, B, P, nb = 2, 16, 7, 12
    parts, sig, ref = problem(oracle, C, B, P, nb)
    n, ld = nb * B, nb * B + 4
    mem = _Mem(torch, False)
    cur = torch.cuda.current_stream()
    s = cur.cuda_stream
    a0, p0 = mem.arena(C, ld, IN_FILL, sig)
    a1, p1 = mem.arena(C, ld, IN_FILL, sig)
    cur.synchronize()
    normal = _maker(neo_gpu, C, B, P, parts, setup=lambda c: c.set_batch(False))()
    _blocks(normal, p0, ld, B, nb, s)
    cur.synchronize()
    normal.close()
    pc = _maker(neo_gpu, C, B, P, parts, setup=lambda c: c.set_batch(False))()
    pc.set_persistent(True, idle_ms=3000.0)
    Err = neo_gpu._native.NeoHipError
    for k in (0, 6):
        q = p1 + 4 * k * B
        with pytest.raises(Err):
            pc.process_device(q + 4, ld, q, ld, s)
        with pytest.raises(Err):
            pc.process_samples_ptr(q, ld, q + 8, ld, B, True, s)
        with pytest.raises(Err):
            pc.process_samples_ptr(q, ld + 1, q, ld + 1, B, True, s)
        with pytest.raises(Err):
            pc.process_samples_ptr(q, ld, q, ld, B + 4, True, s)
        _blocks(pc, q, ld, B, 6, s)
    pc.set_persistent(False)
    cur.synchronize()
    want = check_regions(a0.cpu().numpy(), C, n, IN_FILL)
    got = check_regions(a1.cpu().numpy(), C, n, IN_FILL)
    pc.close()
    assert peak_err(want, ref) <= TOL
    assert_same_bits(got, want, "latency mode after refused calls")
