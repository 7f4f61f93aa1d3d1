// upols.hip — multichannel uniformly-partitioned overlap-save convolution on MI355X.
//
// Replaces C instances of neo's upols_convolver<complex<float>>
// (src/neo/convolution/dense_convolver.hpp:19-20) stepped by dense_convolve /
// DenseConvolution (extra/plugin/src/dsp/DenseConvolution.hpp:39-70). One block
// step for all channels is ONE kernel, k_upols_step, grid C x S:
//
//   - workgroup (c, s) accumulates filter partitions p in [p0, p1) of channel c:
//       acc[k] += H[c][p][k] * FDL[c][(w - p) mod R][k]
//     (fdl_index.hpp:23-36 ring order; dense_filter.hpp:30-35 / multiply_add MAC),
//     streaming 16 B per bin per partition from HBM — the roofline part;
//   - split s == 0 first runs the overlap-save r2c of [previous block | new block]
//     (overlap_save.hpp:90-103) as a packed B-point complex FFT in LDS, inserts it as
//     FDL row w (dense_fdl.hpp:27-30) and uses it for p = 0 straight from LDS;
//   - the last split of a channel to finish sums the S partial spectra in fixed order,
//     runs the c2r (fallback_rfft_plan.hpp:38-55) as a packed inverse FFT in LDS,
//     scales by 1/2B and writes the last B samples (overlap_save.hpp:104-111).
//
// Device layout (HBM), all packed rows of B complex with bin 0 = {DC, Nyquist}
// (both purely real for real signals, so the fold is exact):
//   H    [C][R][B]   filter partitions (uniform_partition.hpp layout, packed; rows >= P unused)
//   FDL  [C][R][B]   frequency-domain delay line, a ring of at least R = P + kMaxBatch - 1 rows
//                    (write position w; the extra rows let a batch of T <= kMaxBatch
//                    new blocks be inserted before any of them is consumed; the far level and
//                    the offline windows ask for more: upols_plan.hpp)
//   prev [C][B]      previous input block (first half of the overlap-save window)
//   part [C][S][B]   per-split partial spectra; arrivals [C] split counters
//
// This file: the single-block step (MAC + finish, or one launch with the last-arriver tail; one
// frame for dense and sparse handles), the upola_convolver_v2 piece kernel, the one create function
// (every kind of handle from its plan: upols_plan.hpp, all checks and shape rules, host only), the
// filter calls (set_begin, a body, set_end) and the rest of the neo_hip_upols_* C-ABI.
// Live filter updates (neo_hip_upols_update_filter / _update_impulse, include/neo_hip.h): the new
// filter goes into a second bank H2 of the handle's own layout and the next fade_blocks blocks are
// crossfaded in the time domain, no state reset. While a fade has blocks left launch_step and
// process_samples run every whole block as one fade step (fade_step: upols_fade.hip's two-bank MAC,
// then the matrix convolver's fade finish with one "output" per channel), whatever the handle's
// modes; at its end the banks swap by pointer (fade_swap). H_alloc remembers the allocation that
// holds the FDL, whichever bank is current. A sparse handle's update (neo_hip_upols_update_filter_sparse
// and the two perceptual forms; sparse_update) is the same frame with a spare sparse bank (h->sp2,
// upols_sparse.hip) and upols_sparse_fade.hip's two-bank MAC; its call waits on its stream for the
// kept-tile counts.
// upols_batch.hip: T blocks per pass (process_blocks). upols_sparse.hip: the sparse handle's
// buffers, filter and MAC. upols_setup.hip: partitioning and normalization. upols_device.hpp /
// upols_handle.hpp: what they share.
#include "matrix_fade.hpp"
#include "upols_device.hpp"
#include "upols_handle.hpp"
#include "perceptual_plan.hpp"
#include "sparse_plan.hpp"
#include "upols_step.hpp"

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

namespace neo_hip {

// the step of one workgroup: upols_step_wg (upols_step.hpp)
template<int B, bool FUSED, bool OLA, bool TAIL = false, int UNROLL = upols_cfg<B>::U>
__global__ __launch_bounds__(256, (B <= 1024 ? 8 : 2)) void k_upols_step(
    const float* __restrict__ in, int64_t ld_in, float* __restrict__ out, int64_t ld_out, float* __restrict__ prev,
    const cf* __restrict__ H, cf* __restrict__ fdl, cf* __restrict__ part, int* __restrict__ arrivals,
    const cf* __restrict__ twg, int P, int ring, int S, int rows, int w, int64_t cstride, int64_t pstride, int pc)
{
    __shared__ step_lds<B> L;
    const int c = blockIdx.x / S, s = blockIdx.x - c * S;
    (void)upols_step_wg<B, FUSED, OLA, TAIL, UNROLL>(L, c, s, in, ld_in, out, ld_out, prev, H, fdl, part, arrivals, twg,
                                                     P, ring, S, rows, w, cstride, pstride, pc);
}

// Latency mode of a handle without streaming levels (fewer than 64 partitions, or the levels off;
// blocks up to 4096: the reference benchmark's shape, extra/benchmark/src/convolution.cpp:47-55):
// the fused plain step's C x S workgroups stay resident across steps. Per step n every workgroup
// waits for step n - 1 to be complete (blk_done: every channel's tail summed its slabs, reset its
// split counter and wrote its output; split 0 wrote the FDL row and the previous block), takes the
// record (workgroup 0 polls the mailbox, ps_record) and runs its split (upols_step_wg, the input
// read and the output stored at system scope). The tail of each channel counts the channel in; the
// last one tells the host (mb->done) and the workgroups (blk_done).
struct plain_persist_args : persist_ctl {
    const cf* H;
    cf* fdl;
    cf* part;
    int* arrivals;
    float* prev;
    const cf* twg;
    int64_t ld_in, ld_out, cstride, pstride;
    int C, P, ring, S, rows, pc;
};

template<int B, bool OLA>
__global__ __launch_bounds__(256) void k_plain_persist(plain_persist_args pa)
{
    __shared__ step_lds<B> L;
    __shared__ uint64_t io[2];
    __shared__ int go;
    const int c = int(blockIdx.x) / pa.S, s = int(blockIdx.x) - c * pa.S;
    const bool lead = blockIdx.x == 0;
    unsigned long long t_seen = 0;  // thread 0 of workgroup 0: when the step's record was read
    int w = pa.w0;                  // ring row of step n
    for (int64_t n = pa.n0;; ++n, w = w + 1 == pa.ring ? 0 : w + 1) {
        if (threadIdx.x == 0) {
            bool ok = ps_wait(pa, [&] { return ps_ld(pa.flags + 0) >= n - 1; });
            if (ok) ps_acquire();  // the slabs, FDL row and previous block of step n - 1 (other workgroups')
            go = ps_record(pa, n, lead, gridDim.x > 1, ok, io, t_seen);
        }
        __syncthreads();
        if (!go) break;
        // two rows in flight at B >= 2048 (one row is 8 or 16 float4 per lane: a trip to memory per row)
        const bool tail = upols_step_wg<B, true, OLA, false, (upols_cfg<B>::VPT >= 4 ? 2 : upols_cfg<B>::U), true>(
            L, c, s, reinterpret_cast<const float*>(io[0]), pa.ld_in, reinterpret_cast<float*>(io[1]), pa.ld_out,
            pa.prev, pa.H, pa.fdl, pa.part, pa.arrivals, pa.twg, pa.P, pa.ring, pa.S, pa.rows, w, pa.cstride,
            pa.pstride, pa.pc,
#ifdef NEO_PS_PROBE
            c == 0 ? pa.tl + 2 * kPsRing + 8 * (n % kPsRing) : nullptr
#else
            nullptr
#endif
        );
        if (tail) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the output's write-through stores complete
            __syncthreads();
            if (threadIdx.x == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                int64_t* arr = pa.flags + kPsFlagArrive + n % kPsArr;
                if (__hip_atomic_fetch_add(arr, int64_t(1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pa.C - 1) {
                    ps_st(arr, 0);  // free for step n + kPsArr
                    const unsigned long long t_done = wall_clock64();
                    __hip_atomic_store(&pa.mb->done, n + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    pa.tl[2 * (n % kPsRing) + 1] = t_done;
                    ps_acquire();  // the other channels' releases, passed on by the one below
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    ps_st(pa.flags + 0, n);
                }
            }
        }
        if (lead && threadIdx.x == 0) pa.tl[2 * (n % kPsRing)] = t_seen;
    }
    if (lead && threadIdx.x == 0) __hip_atomic_store(&pa.mb->alive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

int plain_persist_launch(upols_t* h, const persist_ctl& ctl, int64_t ld_in, int64_t ld_out, bool* launched)
{
    *launched = false;
    if (h->C * h->shape.S > 256) return fail(NEO_HIP_EINVAL, "latency mode: %d x %d plain step workgroups", h->C, h->shape.S);
    plain_persist_args pa{};
    static_cast<persist_ctl&>(pa) = ctl;
    pa.H = h->H;
    pa.fdl = h->fdl;
    pa.part = h->part;
    pa.arrivals = h->arrivals;
    pa.prev = h->prev;
    pa.twg = h->tw;
    pa.ld_in = ld_in;
    pa.ld_out = ld_out;
    pa.cstride = h->shape.cstride;
    pa.pstride = h->shape.pstride;
    pa.C = h->C;
    pa.P = h->P;
    pa.ring = h->ring;
    pa.S = h->shape.S;
    pa.rows = h->shape.rows;
    pa.pc = h->shape.pc;
    const unsigned grid = unsigned(h->C) * unsigned(h->shape.S);
    bool room = false;
    NEO_UPOLS_DISPATCH_OLA(h->B, h->ola,
                           room = persist_room(h, reinterpret_cast<const void*>(&k_plain_persist<BB, OL>), int(grid));
                           if (room) hipLaunchKernelGGL((k_plain_persist<BB, OL>), dim3(grid), dim3(256), 0, h->ps_stream, pa))
    if (!room) return NEO_HIP_OK;
    *launched = true;
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

// Unfused tail (one workgroup per channel): sum the S slabs in order, c2r, write.
template<int B, bool OLA>
__global__ __launch_bounds__(256) void k_upols_finish(const cf* __restrict__ part, float* __restrict__ out,
                                                      int64_t ld_out, float* __restrict__ ovl,
                                                      const cf* __restrict__ twg, int S)
{
    using K = upols_cfg<B>;
    __shared__ __attribute__((aligned(16))) cf X[B];
    __shared__ cf fft[K::LL];
    __shared__ cf tw[K::TW1 + K::TW2];
    const int tid = threadIdx.x, c = blockIdx.x;
    for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];
    const float4* p4 = reinterpret_cast<const float4*>(part + int64_t(c) * S * B);
    for (int q = tid; q < K::Q; q += 256) {
        float4 sum = p4[q];
        int t = 1;
        for (; t + 7 < S; t += 8) {
            float4 r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] = p4[int64_t(t + u) * K::Q + q];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                sum.x += r[u].x; sum.y += r[u].y; sum.z += r[u].z; sum.w += r[u].w;
            }
        }
        for (; t < S; ++t) {
            const float4 r = p4[int64_t(t) * K::Q + q];
            sum.x += r.x; sum.y += r.y; sum.z += r.z; sum.w += r.w;
        }
        reinterpret_cast<float4*>(X)[q] = sum;
    }
    __syncthreads();
    c2r_tail<B, OLA, NEO_FINISH_E(B)>(X, fft, tw, out + int64_t(c) * ld_out,
                                                                     ovl + int64_t(c) * B, tid);
}

// upola_convolver_v2 piece (overlap_add_convolver.hpp:71-136), one workgroup per channel,
// for n samples at block position pos. The real window [C][2B] is state, exactly as in
// the reference: the irfft result is written back into it (:114), so a later piece of
// the same block transforms [earlier output | new samples | earlier output]. Steps:
//   sum_first (pos == 0): tmp = sum of the TAIL slabs (partitions p >= 1, :96-108)
//   window[pos, pos+n) = input; X = rfft(window); FDL row w = X          (:90-94)
//   acc = tmp + X * H[0]                                                 (:110-112)
//   window = irfft(acc) / 2B; out = window[pos, pos+n) + overlap[...]    (:114-118)
//   complete (pos + n == B): overlap = window[B, 2B); window = 0         (:122-131)
// Whole blocks at pos 0 take the UPOLA launch pair instead: with a zero window and
// full input the two are the same computation.
template<int B>
__global__ __launch_bounds__(256) void k_upola2_piece(
    const float* __restrict__ in, int64_t ld_in, float* __restrict__ out, int64_t ld_out, int n, int pos,
    float* __restrict__ window, float* __restrict__ ovl, cf* __restrict__ tmp, const cf* __restrict__ part, int S,
    int sum_first, const cf* __restrict__ H, cf* __restrict__ fdl, int w, const cf* __restrict__ twg, int64_t cstride,
    int64_t pstride)
{
    using K = upols_cfg<B>;
    constexpr int E = K::E, T = K::T;
    __shared__ __attribute__((aligned(16))) float wl[2 * B];  // real window, then the irfft output
    __shared__ __attribute__((aligned(16))) cf acc[B];
    __shared__ cf fft[K::LL];
    __shared__ cf tw[K::TW1 + K::TW2];
    const int tid = threadIdx.x, c = blockIdx.x;
    for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];

    cf* tmp_c = tmp + int64_t(c) * B;
    if (sum_first) {  // fixed order s = 0..S-1, like k_upols_finish
        const cf* pc = part + int64_t(c) * S * B;
        for (int k = tid; k < B; k += 256) {
            cf sum = pc[k];
            for (int t = 1; t < S; ++t) {
                const cf r = pc[int64_t(t) * B + k];
                sum.x += r.x;
                sum.y += r.y;
            }
            acc[k] = sum;
            tmp_c[k] = sum;
        }
    } else {
        for (int k = tid; k < B; k += 256) acc[k] = tmp_c[k];
    }
    float* win_c = window + int64_t(c) * 2 * B;
    const float* in_c = in + int64_t(c) * ld_in;
    for (int i = tid; i < 2 * B; i += 256) wl[i] = (i >= pos && i < pos + n) ? in_c[i - pos] : win_c[i];
    __syncthreads();

    const bool active = tid < T;
    cf v[E];
    if (active) {
#pragma unroll
        for (int m = 0; m < E; ++m) v[m] = reinterpret_cast<const cf*>(wl)[tid + m * T];
    }
    stockham<B, E, -1>(v, fft, tw, tid, active);
    if (active) {
#pragma unroll
        for (int m = 0; m < E; ++m) fft[lpad(tid + m * T)] = v[m];
    }
    __syncthreads();
    cf* row = fdl + int64_t(c) * cstride + int64_t(w) * pstride;
    const cf* h0 = H + int64_t(c) * cstride;  // partition 0
    for (int k = tid; k < B; k += 256) {
        const cf x = r2c_split<B>(fft, tw + K::TW1, k), h = h0[k], a = acc[k];
        row[k] = x;
        acc[k] = k == 0 ? cf{x.x * h.x + a.x, x.y * h.y + a.y}  // packed {DC, Nyquist}: real products
                        : cf{(x.x * h.x - x.y * h.y) + a.x, (x.x * h.y + x.y * h.x) + a.y};
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int k = tid + m * T;
            const cf a0 = acc[0];
            v[m] = k == 0 ? c2r_join<B>(cf{a0.x, 0.f}, cf{a0.y, 0.f}, tw + K::TW1, 0)
                          : c2r_join<B>(acc[k], acc[B - k], tw + K::TW1, k);
        }
    }
    stockham<B, E, +1>(v, fft, tw, tid, active);
    if (active) {
        const float scale = 1.0f / float(2 * B);  // :115
#pragma unroll
        for (int m = 0; m < E; ++m) reinterpret_cast<cf*>(wl)[tid + m * T] = {v[m].x * scale, v[m].y * scale};
    }
    __syncthreads();
    float* out_c = out + int64_t(c) * ld_out;
    float* ovl_c = ovl + int64_t(c) * B;
    for (int j = tid; j < n; j += 256) out_c[j] = wl[pos + j] + ovl_c[pos + j];
    if (pos + n == B) {
        __syncthreads();  // overlap reads above are done before it is replaced
        for (int i = tid; i < B; i += 256) ovl_c[i] = wl[B + i];
        for (int i = tid; i < 2 * B; i += 256) win_c[i] = 0.0f;
    } else {
        for (int i = tid; i < 2 * B; i += 256) win_c[i] = wl[i];
    }
}

}  // namespace neo_hip

using namespace neo_hip;


int neo_hip::setup_join(upols_t* h, bool device_input)
{
    if (int rc = h->used.join()) return rc;
    if (device_input)
        if (int rc = null_join()) return rc;
    if (int rc = lvl_join(h, h->stream)) return rc;
    NEO_HIP_CHECK(hipStreamSynchronize(h->stream));
    return NEO_HIP_OK;
}

namespace {

int reset_state(upols_t* h, hipStream_t s)
{
    if (int rc = lvl_join(h, s)) return rc;
    NEO_HIP_CHECK(hipMemsetAsync(h->fdl, 0, size_t(h->C) * h->ring * h->B * sizeof(cf), s));
    NEO_HIP_CHECK(hipMemsetAsync(h->prev, 0, size_t(h->C) * h->B * sizeof(float), s));
    NEO_HIP_CHECK(hipMemsetAsync(h->arrivals, 0, size_t(h->C) * sizeof(int), s));
    if (h->v2) {
        NEO_HIP_CHECK(hipMemsetAsync(h->window, 0, size_t(h->C) * 2 * h->B * sizeof(float), s));
        NEO_HIP_CHECK(hipMemsetAsync(h->tmp, 0, size_t(h->C) * h->B * sizeof(cf), s));
    }
    h->wpos = 0;
    h->in_pos = 0;
    h->lv_n = -1;  // streaming levels re-prime at the next step (zeroing: lvl_prime)
    h->fdl_zero = true;
    return NEO_HIP_OK;
}

void destroy(upols_t* h)
{
    if (!h) return;
    (void)persist_stop(h);
    if (h->ps_stream) (void)hipStreamDestroy(h->ps_stream);
    hfree(h->ps_mb);
    dfree(h->ps_flags);
    dfree(h->ps_tl);
    for (auto& g : h->events)
        for (auto& e : g.e) (void)hipEventDestroy(e);
    lvl_free(h);  // joins the background stream first
    // device buffers back to the pool (dmem.hip): no device-wide synchronization; the caller
    // joined every stream that used them
    dfree(h->H_alloc);  // the FDL shares H's allocation (rows [nrows, 2 nrows))
    dfree(h->H == h->H_alloc ? h->H2 : h->H);  // a live update's bank: the one that is not in that allocation
    dfree(h->part_f);
    dfree(h->ovl2);
    if (h->sparse) {  // no dense filter: the FDL is an allocation of its own
        dfree(h->fdl);
        sparse_free(h);
    }
    dfree(h->part);
    dfree(h->prev);
    dfree(h->arrivals);
    dfree(h->window);
    dfree(h->tmp);
    hfree(h->io_host);  // h->io is its device mapping
    dfree(h->samples_dev);
    dfree(h->part_b);
    dfree(h->tail);
    dfree(h->off_hf);
    dfree(h->off_y);
    dfree(h->off_tail);
    hfree(h->samples_host);
    delete h;  // h->stream is shared (a group's, or one of the device's four: dmem.hip)
}

// the end of a fade: bank B is the filter (pointers swap, no copy; overlap-add: its tails are the
// tails), and what is computed from the filter follows it (far segment spectra, offline spectra)
void fade_swap(upols_t* h)
{
    if (h->sparse) sparse_fade_swap(h);  // bitmaps, offsets, bases, tiles and counts; pc / pcb follow the new tiles
    else std::swap(h->H, h->H2);
    if (h->ola) std::swap(h->prev, h->ovl2);
    h->fade_left = h->fade_total = 0;
    lvl_filter_changed(h);
}

// One block of a running fade, whatever the handle's modes: an excursion from the streaming levels
// like the plain step's (launch_step_normal: background slices joined, the levels prime again at
// the next streaming step), both banks against the same FDL rows, the mix in the finish.
int fade_step(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s)
{
    if (int rc = lvl_join(h, s)) return rc;
    if (int rc = h->sparse ? launch_sparse_fade_mac(h, sparse_cur(h), h->sp2, in, ld_in, h->fade_S, h->fade_rows, h->wpos, false, s)
                           : launch_upols_fade_mac(h, h->H, h->H2, in, ld_in, h->fade_S, h->fade_rows, h->wpos, false, s))
        return rc;
    h->fdl_zero = false;
    const int64_t n0 = int64_t(h->fade_total - h->fade_left) * h->B;
    if (int rc = launch_matrix_fade_finish(h->part_f, out, ld_out, h->prev, h->ovl2, h->tw, h->B, h->C, h->fade_S, h->ola,
                                           false, n0, int64_t(h->fade_total) * h->B, h->fade_curve, s))
        return rc;
    advance(h, 1);
    h->lv_n = -1;
    if (--h->fade_left == 0) fade_swap(h);
    return NEO_HIP_OK;
}

int launch_step(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s)
{
    if (int rc = note_stream(h, s)) return rc;
    if (h->fade_left > 0) return fade_step(h, in, ld_in, out, ld_out, s);  // (never with the latency mode on)
    if (h->sched.persist) return persist_process(h, in, ld_in, out, ld_out, 1);  // synchronous: s is not used
    return launch_step_normal(h, in, ld_in, out, ld_out, s);
}

}  // namespace

int neo_hip::launch_finish(upols_t* h, float* out, int64_t ld_out, hipStream_t s)
{
    return launch_finish_slabs(h->C, h->B, h->shape.S, h->ola, h->part, out, ld_out, h->prev, h->tw, s);
}

int neo_hip::launch_finish_slabs(int C, int B, int S, bool ola, const cf* part, float* out, int64_t ld_out, float* ovl,
                                 const cf* tw, hipStream_t s)
{
    NEO_UPOLS_DISPATCH_OLA(B, ola, hipLaunchKernelGGL((k_upols_finish<BB, OL>), dim3(unsigned(C)), dim3(256), 0, s, part, out,
                                                      ld_out, ovl, tw, S))
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

namespace {

// the one k_upols_step launch (grid C x S): the plain step's MAC in its one-launch (FUSED) or
// MAC + finish form, or (TAIL) the v2 piece's MAC over partitions p >= 1
template<bool FUSED, bool OLA, bool TAIL>
int launch_upols_step(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s)
{
    const upols_shape& sh = h->shape;
    const unsigned grid = unsigned(h->C) * unsigned(sh.S);
    NEO_UPOLS_DISPATCH(h->B, hipLaunchKernelGGL((k_upols_step<BB, FUSED, OLA, TAIL>), dim3(grid), dim3(256), 0, s, in, ld_in,
                                                out, ld_out, h->prev, h->H, h->fdl, h->part, h->arrivals, h->tw, h->P,
                                                h->ring, sh.S, sh.rows, h->wpos, sh.cstride, sh.pstride, sh.pc))
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

}  // namespace

// One block without the streaming levels, dense or sparse: the MAC launch between the timing marks,
// the finish launch of the two-launch form, the write position one row on.
int neo_hip::launch_step_normal(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s)
{
    if (h->shape.ahead) return launch_levels(h, in, ld_in, out, ld_out, s);
    if (int rc = lvl_join(h, s)) return rc;
    upols_t::ev_group* ev = nullptr;
    if (int rc = timing_begin(h, 2, &ev)) return rc;
    if (int rc = timing_mark(ev, 0, s)) return rc;
    const bool fu = h->shape.fused, ol = h->ola;
    if (int rc = h->sparse  ? launch_sparse_mac(h, in, ld_in, out, ld_out, s)
                 : fu && ol ? launch_upols_step<true, true, false>(h, in, ld_in, out, ld_out, s)
                 : fu       ? launch_upols_step<true, false, false>(h, in, ld_in, out, ld_out, s)
                 : ol       ? launch_upols_step<false, true, false>(h, in, ld_in, out, ld_out, s)
                            : launch_upols_step<false, false, false>(h, in, ld_in, out, ld_out, s))
        return rc;
    h->fdl_zero = false;
    if (int rc = timing_mark(ev, 1, s)) return rc;
    if (!h->shape.fused)
        if (int rc = launch_finish(h, out, ld_out, s)) return rc;
    advance(h, 1);
    h->lv_n = -1;
    return NEO_HIP_OK;
}

namespace {

// One v2 piece of n samples at block position h->in_pos (n <= B - in_pos).
int launch_piece(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, int n, hipStream_t s)
{
    const int sum_first = h->in_pos == 0;
    if (int rc = lvl_join(h, s)) return rc;
    h->lv_n = -1;
    h->fdl_zero = false;
    if (sum_first)  // tail MAC over partitions p >= 1 into the split slabs
        if (int rc = launch_upols_step<false, true, true>(h, in, ld_in, out, ld_out, s)) return rc;
    NEO_UPOLS_DISPATCH(h->B, hipLaunchKernelGGL((k_upola2_piece<BB>), dim3(unsigned(h->C)), dim3(256), 0, s, in, ld_in,
                                                out, ld_out, n, h->in_pos, h->window, h->prev, h->tmp, h->part,
                                                h->shape.S, sum_first, h->H, h->fdl, h->wpos, h->tw, h->shape.cstride,
                                                h->shape.pstride))
    NEO_HIP_LAUNCH_CHECK();
    h->in_pos += n;
    if (h->in_pos == h->B) {  // block complete: next FDL row (overlap_add_convolver.hpp:131)
        h->in_pos = 0;
        advance(h, 1);
    }
    return NEO_HIP_OK;
}

// Any number of samples for every channel (channel c at in + c * ld_in). upols / upola
// handles take whole blocks only; v2 handles split the samples at block boundaries
// (overlap_add_convolver.hpp:80-134) and run whole aligned blocks through launch_step.
int process_samples(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t n, hipStream_t s)
{
    if (int rc = note_stream(h, s)) return rc;
    const int B = h->B;
    const int T = h->shape.batch ? batch_blocks(h) : 1;
    const bool a16 = io_aligned(in, out, ld_in, ld_out);
    if (h->sched.persist) {  // latency mode: every block through the persistent kernel, complete on return
        if (n % B || !a16) return fail(NEO_HIP_EINVAL, "latency mode: whole 16-byte aligned blocks");
        return persist_process(h, in, ld_in, out, ld_out, n / B);
    }
    if (!h->v2) {
        if (n % B) return fail(NEO_HIP_EINVAL, "upols/upola convolvers take whole blocks (%lld samples, block %d)",
                               (long long)n, B);
        if (!a16) return fail(NEO_HIP_EINVAL, "device I/O must be 16-byte aligned (ld multiple of 4)");
    }
    // Streaming levels: a batched pass leaves them to re-prime at the next single-block step
    // (window 0 of every level computed whole, 2 x 128 far launches), so with the levels on
    // only whole T-block batches run (the rest stream, one prime per call at most), and a
    // call of fewer than kStreamKeep batches' blocks on primed levels streams them all.
    constexpr int kStreamKeep = 4;
    const bool stream_all = h->shape.ahead && h->lv_n >= 0 && n < int64_t(kStreamKeep) * T * B;
    int64_t done = 0;
    while (done < n) {
        const float* ip = in + done;
        float* op = out + done;
        int rc;
        if (h->fade_left > 0) {  // a running fade: single fade steps to its last block, then the usual passes
            if ((rc = launch_step(h, ip, ld_in, op, ld_out, s))) return rc;
            done += B;
            continue;
        }
        // offline windows: 256 or 128 whole blocks left, every block known (batching on)
        const int64_t left = (n - done) / B;
        if (h->shape.off && h->shape.batch && !stream_all && h->in_pos == 0 && a16 && done % 4 == 0 && left >= kFarT) {
            const int wp = left >= int64_t(kFarT) * kOffMaxWP ? kOffMaxWP : 1;
            if ((rc = launch_offline(h, ip, ld_in, op, ld_out, wp, s))) return rc;
            done += int64_t(wp) * kFarT * B;
            continue;
        }
        // the largest power-of-two batch (<= T) of whole blocks left, one pass over H + FDL
        int tb = 1;
        while (!stream_all && tb * 2 <= T && n - done >= int64_t(tb) * 2 * B) tb *= 2;
        if (h->shape.ahead && tb < T) tb = 1;
        if (h->in_pos == 0 && tb > 1 && a16 && done % 4 == 0) {
            rc = launch_batch(h, ip, ld_in, op, ld_out, tb, s);
            done += int64_t(tb) * B;
        } else if (!h->v2) {
            rc = launch_step(h, ip, ld_in, op, ld_out, s);
            done += B;
        } else {
            const int k = int(std::min<int64_t>(n - done, B - h->in_pos));
            // whole block on an 8-byte grid: the UPOLA pair computes the same thing
            const bool pair = h->in_pos == 0 && k == B &&
                              !((reinterpret_cast<uintptr_t>(ip) | reinterpret_cast<uintptr_t>(op)) & 7) &&
                              !((ld_in | ld_out) & 1);
            rc = pair ? launch_step(h, ip, ld_in, op, ld_out, s) : launch_piece(h, ip, ld_in, op, ld_out, k, s);
            done += k;
        }
        if (rc) return rc;
    }
    return NEO_HIP_OK;
}

}  // namespace


namespace {

// Every kind of handle: the plan (upols_plan.hpp: checks and shape rules), the device, the stream,
// the buffers of its kind, twiddles, stream-ordered zeroing, one wait. Dense / v2: filter and FDL in
// ONE allocation (FDL = rows [nrows, 2 nrows)): the LDS-DMA batched MAC reaches both of a channel
// through a single buffer descriptor; v2 adds its window and tail accumulator. Sparse
// (sparse_convolver.hpp:12-17): the FDL ring, the step state and the bitmaps / offsets; the tiles come
// with the filter (sparse_set_filter); no dense filter, level or offline buffers. The batch
// buffers come with the first batched pass (launch_batch).
int create_convolver(int channels, int block, int partitions, int device, upols_kind kind, bool ola,
                     const neo_hip_upols_opts* opt, neo_hip_upols** out, hipStream_t borrow = nullptr)
{
    if (!out) return fail(NEO_HIP_EINVAL, "handle pointer is null");
    *out = nullptr;
    upols_shape shape;
    if (const char* why = make_upols_shape(channels, block, partitions, opt, kind, borrow != nullptr, shape))
        return fail(NEO_HIP_EINVAL, "%s", why);
    const bool sparse = kind == upols_kind::sparse, v2 = kind == upols_kind::v2;
    device_guard g(device);
    if (g.rc) return g.rc;
    auto* h = new upols_t{};
    h->shape = std::move(shape);
    auto bail = [&](int code) {
        destroy(h);
        return code;
    };
    (void)hipGetDevice(&h->device);
    h->sparse = sparse;
    h->v2 = v2;
    h->ola = ola || v2;
    if (!sparse) h->bg_pad = bg_pad_for(channels, block);
    // a group member runs its setup and host-I/O work on its group's stream (upols_group.hip),
    // every other handle on one of its device's four shared streams (dmem.hip shared_stream: a
    // stream of its own would cost ~4 ms to create and ~3 ms to destroy; the first four handles on
    // a device create them)
    h->stream = borrow;
    if (!borrow) {
#ifdef NEO_OWN_STREAM  // diagnostic builds (A/B): a stream of its own per handle, as before round 5 (never destroyed)
        if (hipStreamCreateWithFlags(&h->stream, hipStreamDefault) != hipSuccess)
            return bail(fail(NEO_HIP_ERUNTIME, "hipStreamCreate failed"));
#else
        if (int rc = shared_stream(&h->stream)) return bail(rc);
#endif
    }
    const size_t rowbytes = size_t(block) * sizeof(cf);
    const size_t nrows = size_t(channels) * size_t(h->ring);  // H uses the first P rows of each channel
    const size_t ringbytes = (sparse ? 1 : 2) * nrows * rowbytes;
    if (dalloc(sparse ? &h->fdl : &h->H, ringbytes) || dalloc(&h->part, size_t(channels) * h->shape.S * rowbytes) ||
        dalloc(&h->prev, size_t(channels) * block * sizeof(float)) || dalloc(&h->arrivals, size_t(channels) * sizeof(int)) ||
        (v2 && (dalloc(&h->window, size_t(channels) * 2 * block * sizeof(float)) ||
                dalloc(&h->tmp, size_t(channels) * rowbytes))) ||
        (sparse && sparse_alloc(h)))
        return bail(fail(NEO_HIP_ENOMEM, "device allocation of %zu bytes failed", ringbytes));
    if (!sparse) h->fdl = h->H + nrows * size_t(block);
    h->H_alloc = h->H;
    if (int rc = shared_tw(&h->tw, block)) return bail(rc);
    // stream-ordered zeroing, one wait at the end (the caller's later work may run on any stream)
    if (!sparse && hipMemsetAsync(h->H, 0, nrows * rowbytes, h->stream) != hipSuccess)
        return bail(fail(NEO_HIP_ERUNTIME, "memset failed"));
    if (int rc = reset_state(h, h->stream)) return bail(rc);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return bail(fail(NEO_HIP_ERUNTIME, "sync failed"));
    *out = h;
    return NEO_HIP_OK;
}
}  // namespace

int neo_hip::create_handle(int channels, int block, int partitions, int device, int method, hipStream_t stream,
                           neo_hip_upols** out)
{
    const int rc = create_convolver(channels, block, partitions, device, method == 2 ? upols_kind::v2 : upols_kind::dense,
                                    method >= 1, nullptr, out, stream);
    if (!rc) (*out)->grouped = true;
    return rc;
}

// -- the filter calls: checks, set_begin, a body that names what differs (pack, or normalize +
// partition; the caller's mask or the perceptual one; the dense or the sparse store), set_end. Every
// temporary is pooled scratch that set_end gives back once the handle's stream is joined. ----------
namespace {

// after this handle's steps on any stream (and a device input's producer); a resident
// latency-mode kernel leaves first
int set_begin(upols_t* h, bool device_input)
{
    if (int rc = persist_stop(h)) return rc;
    return setup_join(h, device_input);
}

// A filter call's last steps, rc its body's result: the levels' and the offline windows' spectra
// are stale, the state is rebuilt as the reference's filter() does
// (uniform_partitioned_convolver.hpp:37-45) and, its next call being an ordinary block step
// (:47-65), the levels' setup runs here, not there; then the stream is joined and the scratch goes
// back, whatever rc is. (A sparse handle has no levels: both level calls change nothing.)
int set_end(upols_t* h, int rc, std::initializer_list<void*> scratch)
{
    lvl_filter_changed(h);
    h->fade_left = h->fade_total = 0;  // a running fade is cancelled: the filter just loaded (bank A) is the filter
    if (!rc) h->has_filter = true;
    if (!rc) rc = reset_state(h, h->stream);
    if (!rc) rc = lvl_setup_prime(h);
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    for (void* p : scratch) dfree(p);
    return rc;
}

int check_impulse(const upols_t* h, int64_t length)
{
    if (partitions_for(length, h->B) != h->P)
        return fail(NEO_HIP_EINVAL, "impulse of %lld taps gives %lld partitions, convolver has %d", (long long)length,
                    (long long)partitions_for(length, h->B), h->P);
    return NEO_HIP_OK;
}

// impulse [C][length], host or device -> a copy of it (*tmp), normalized on request, partitioned on s:
// packed into `bank` (a filter bank of the handle's layout; out null) or as [C][P][B + 1] into out.
// The copy is pooled scratch (stage_in: the caller gives it back once s is joined) or, stream_scratch,
// stream-ordered scratch (the caller frees it on s: no host-side wait anywhere)
int load_impulse(upols_t* h, const float* ir, int64_t length, int normalize, int is_device, cf* out, float** tmp, cf* bank,
                 hipStream_t s, bool stream_scratch = false)
{
    const float* d = nullptr;
    const size_t bytes = size_t(h->C) * size_t(length) * sizeof(float);
    int rc = NEO_HIP_OK;
    if (stream_scratch) {
        if (hipMallocAsync(reinterpret_cast<void**>(tmp), bytes, s) != hipSuccess) {
            (void)hipGetLastError();
            return fail(NEO_HIP_ENOMEM, "allocation of %zu bytes failed", bytes);
        }
        if (hipMemcpyAsync(*tmp, ir, bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s) != hipSuccess)
            rc = fail(NEO_HIP_ERUNTIME, "copy to the device failed");
        d = *tmp;
    } else {
        rc = stage_in(ir, bytes, is_device != 0, true, s, tmp, &d);
    }
    if (!rc && normalize) rc = normalize_device(*tmp, h->C, length, s);
    if (!rc)
        rc = out ? partition_device(d, h->C, length, h->B, false, out, h->tw, s)
                 : partition_device(d, h->C, length, h->B, true, bank, h->tw, s, h->shape.cstride, h->shape.pstride);
    return rc;
}

// a sparse handle's perceptual calls: their checks, and the store of a device filter [C][P][B + 1]
// under the mask the predicate gives it (perceptual.hip; w: the host weights [B + 1], alive until
// the stream is joined)
int check_perceptual(const char* who, const upols_t* h, const void* src, const neo_hip_perceptual* pp)
{
    if (!h || !src || !pp) return fail(NEO_HIP_EINVAL, "%s: null handle, input or parameters", who);
    if (!h->sparse) return fail(NEO_HIP_EINVAL, "%s: not a sparse handle (neo_hip_upols_create_sparse)", who);
    if (const char* why = perceptual_check(h->B, pp)) return fail(NEO_HIP_EINVAL, "%s: %s", who, why);
    return NEO_HIP_OK;
}

size_t filter_elems(const upols_t* h) { return size_t(h->C) * size_t(h->P) * size_t(h->B + 1); }

int store_perceptual(upols_t* h, const cf* filter, const neo_hip_perceptual* pp, const std::vector<float>& w,
                     uint8_t** mask, float** tmp)
{
    if (dalloc(mask, filter_elems(h))) return fail(NEO_HIP_ENOMEM, "allocation failed");
    if (int rc = perceptual_mask_device(filter, h->C, h->B, h->P, pp, w.data(), *mask, tmp, h->stream)) return rc;
    return sparse_set_filter(h, filter, *mask, h->stream);
}

std::vector<float> weights_for(const upols_t* h, const neo_hip_perceptual* pp)
{
    std::vector<float> w(size_t(h->B) + 1);
    perceptual_weights(h->B, pp, w.data());
    return w;
}

// -- live filter updates: update_* = check, the fade's buffers, the load into the spare bank on the
// call's stream, update_end (overlap-add's priming pass, the fade armed) -------------------------

// what every update checks before it touches anything (sparse_call: one of the sparse forms, which
// take sparse handles only; the dense forms keep refusing them)
int update_check(const upols_t* h, int fade_blocks, int curve, bool sparse_call = false)
{
    if (h->sparse && !sparse_call) return fail(NEO_HIP_EINVAL, "filter update: a sparse handle keeps no dense filter bank");
    if (!h->sparse && sparse_call)
        return fail(NEO_HIP_EINVAL, "sparse filter update: not a sparse handle (neo_hip_upols_create_sparse)");
    if (h->v2) return fail(NEO_HIP_EINVAL, "filter update: upola_convolver_v2 handles (sub-block input) are not faded");
    if (h->grouped) return fail(NEO_HIP_EINVAL, "filter update: the handle belongs to a convolver group");
    if (h->sched.persist) return fail(NEO_HIP_EINVAL, "filter update: the handle is in latency mode (set_persistent)");
    if (!h->has_filter) return fail(NEO_HIP_EINVAL, "filter update: no filter set (neo_hip_upols_set_filter)");
    if (fade_blocks < 1 || fade_blocks > kMatrixFadeMaxBlocks)
        return fail(NEO_HIP_EINVAL, "filter update: fade_blocks must be in [1, %d]", kMatrixFadeMaxBlocks);
    if (curve < 0 || curve >= kMatrixFadeCurves)
        return fail(NEO_HIP_EINVAL, "filter update: curve must be 0 (linear) or 1 (raised cosine)");
    if (h->fade_left > 0) return fail(NEO_HIP_EINVAL, "filter update: a fade is still running (%d blocks left)", h->fade_left);
    return NEO_HIP_OK;
}

// device memory: the caller's stream; host memory: the handle's own unless one is given
hipStream_t update_stream(const upols_t* h, int is_device, void* stream)
{
    return is_device || stream ? as_stream(stream) : h->stream;
}

// the call's stream noted; a host filter's call is synchronous, so it also comes after the
// handle's earlier steps on every stream (the last fade step may still read the spare bank)
int update_begin(upols_t* h, bool is_device, hipStream_t s)
{
    if (!is_device)
        if (int rc = h->used.join()) return rc;
    return note_stream(h, s);
}

// the spare bank (zero, on s: rows >= P of a channel stay zero as in the first bank), the fade
// step's slabs and bank B's overlap-add tails, at the first update; kept until the handle goes
int fade_buffers(upols_t* h, hipStream_t s)
{
    if (h->H2) return NEO_HIP_OK;
    const upols_fade_plan f = upols_fade_split(h->shape);
    cf *bank = nullptr, *slabs = nullptr;
    float* tails = nullptr;
    if (dalloc(&bank, size_t(f.bank_bytes)) || dalloc(&slabs, size_t(f.slab_bytes)) ||
        (h->ola && dalloc(&tails, size_t(h->C) * h->B * sizeof(float)))) {
        dfree(bank);
        dfree(slabs);
        dfree(tails);
        return fail(NEO_HIP_ENOMEM, "filter update: allocation of the second bank (%lld bytes) failed", (long long)f.bank_bytes);
    }
    if (hipMemsetAsync(bank, 0, size_t(f.bank_bytes), s) != hipSuccess) {
        dfree(bank);
        dfree(slabs);
        dfree(tails);
        return fail(NEO_HIP_ERUNTIME, "memset failed");
    }
    h->H2 = bank;
    h->part_f = slabs;
    h->ovl2 = tails;
    h->fade_S = f.S;
    h->fade_rows = f.rows;
    return NEO_HIP_OK;
}

// An update call after its load (rc) on s. Overlap-add: a fade that starts at block k needs bank
// B's tail of block k - 1; the rows (w - 1 - p) mod ring, p < P, are all intact (a step writes row
// w alone), so one pass of the spare bank at write position w - 1 (no window, no insert) and the
// finish's prime form leave it in ovl2. Nothing stepped since a reset: the tail is zero. Then the
// fade is armed. Host memory: complete on return.
int update_end(upols_t* h, int rc, bool is_device, int fade_blocks, int curve, hipStream_t s)
{
    if (!rc && h->ola) {
        if (h->fdl_zero) {
            if (hipMemsetAsync(h->ovl2, 0, size_t(h->C) * h->B * sizeof(float), s) != hipSuccess)
                rc = fail(NEO_HIP_ERUNTIME, "memset failed");
        } else {
            const int w1 = (h->wpos + h->ring - 1) % h->ring;
            rc = h->sparse ? launch_sparse_fade_mac(h, h->sp2, h->sp2, nullptr, 0, h->fade_S, h->fade_rows, w1, true, s)
                           : launch_upols_fade_mac(h, h->H2, h->H2, nullptr, 0, h->fade_S, h->fade_rows, w1, true, s);
            if (!rc)
                rc = launch_matrix_fade_finish(h->part_f, nullptr, 0, h->prev, h->ovl2, h->tw, h->B, h->C, h->fade_S, true, true,
                                               0, 1, 0, s);
        }
    }
    if (!is_device && hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    if (!rc) {
        h->fade_left = h->fade_total = fade_blocks;
        h->fade_curve = curve;
    }
    return rc;
}

// A sparse handle's update after its checks: the call's stream, the fixed-size buffers (first update),
// `load` (what differs between the three forms: the filter [C][P][B + 1] and its mask on the device,
// on s; scratch it allocates goes into `scratch`), the one packing path into the spare bank, then
// update_end. NOT asynchronous, even for device memory: sparse_fill waits on s for the three
// counts that size bank B's tiles (the stream, never the device), and pooled scratch is given back
// after a second wait on s. That first wait also covers the last step of an earlier fade, so the
// retired bank's tiles go back to the pool inside sparse_fill.
template<class Load>
int sparse_update(upols_t* h, int is_device, int fade_blocks, int curve, void* stream, Load load)
{
    device_guard g(h->device);
    if (g.rc) return g.rc;
    hipStream_t s = update_stream(h, is_device, stream);
    if (int rc = update_begin(h, is_device != 0, s)) return rc;
    if (int rc = sparse_fade_buffers(h, s)) return rc;
    std::vector<void*> scratch;
    const cf* filter = nullptr;
    const uint8_t* mask = nullptr;
    int rc = load(s, &filter, &mask, scratch);
    if (!rc) rc = sparse_fill(h, h->sp2, filter, mask, s);
    const bool wait = !is_device || !scratch.empty();
    rc = update_end(h, rc, !wait, fade_blocks, curve, s);  // (is_device = false: it waits on s)
    for (void* p : scratch) dfree(p);
    return rc;
}

}  // namespace

extern "C" {

NEO_HIP_API int neo_hip_upols_create_sparse(int channels, int block, int partitions, int device, int method,
                                            const neo_hip_upols_opts* opts, neo_hip_upols** out)
{
    if (method < 0 || method > 1)
        return fail(NEO_HIP_EINVAL, "sparse convolvers: method must be 0 (upols) or 1 (upola); whole blocks only");
    return create_convolver(channels, block, partitions, device, upols_kind::sparse, method == 1, opts, out);
}

NEO_HIP_API int neo_hip_upols_set_filter_sparse(neo_hip_upols* h, const void* filter, const uint8_t* mask, int is_device)
{
    if (!h || !filter || !mask) return fail(NEO_HIP_EINVAL, "null handle, filter or mask");
    if (!h->sparse) return fail(NEO_HIP_EINVAL, "set_filter_sparse: not a sparse handle (neo_hip_upols_create_sparse)");
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = set_begin(h, is_device != 0)) return rc;
    const size_t n = filter_elems(h);
    cf* tmpf = nullptr;
    const cf* src = nullptr;
    uint8_t* tmpm = nullptr;
    const uint8_t* msk = nullptr;
    int rc = stage_in(static_cast<const cf*>(filter), n * sizeof(cf), is_device != 0, false, h->stream, &tmpf, &src);
    if (!rc) rc = stage_in(mask, n, is_device != 0, false, h->stream, &tmpm, &msk);
    if (!rc) rc = sparse_set_filter(h, src, msk, h->stream);
    return set_end(h, rc, {tmpf, tmpm});
}

// The perceptual forms: the mask is made on the device (perceptual.hip) from spectra that are
// already there, then sparse_set_filter runs unchanged.
NEO_HIP_API int neo_hip_upols_set_filter_perceptual(neo_hip_upols* h, const void* filter, const neo_hip_perceptual* pp,
                                                    int is_device)
{
    if (int rc = check_perceptual("set_filter_perceptual", h, filter, pp)) return rc;
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = set_begin(h, is_device != 0)) return rc;
    const std::vector<float> w = weights_for(h, pp);
    cf* tmpf = nullptr;
    uint8_t* mask = nullptr;
    float* tmp = nullptr;
    const cf* src = nullptr;
    int rc = stage_in(static_cast<const cf*>(filter), filter_elems(h) * sizeof(cf), is_device != 0, false, h->stream, &tmpf, &src);
    if (!rc) rc = store_perceptual(h, src, pp, w, &mask, &tmp);
    return set_end(h, rc, {tmp, tmpf, mask});
}

NEO_HIP_API int neo_hip_upols_set_impulse_perceptual(neo_hip_upols* h, const float* ir, int64_t length, int normalize,
                                                     const neo_hip_perceptual* pp, int is_device)
{
    if (length < 1) return fail(NEO_HIP_EINVAL, "set_impulse_perceptual: empty impulse");
    if (int rc = check_perceptual("set_impulse_perceptual", h, ir, pp)) return rc;
    if (int rc = check_impulse(h, length)) return rc;
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = set_begin(h, is_device != 0)) return rc;
    const std::vector<float> w = weights_for(h, pp);
    float* d = nullptr;
    cf* parts = nullptr;
    uint8_t* mask = nullptr;
    float* tmp = nullptr;
    int rc = dalloc(&parts, filter_elems(h) * sizeof(cf)) ? fail(NEO_HIP_ENOMEM, "allocation failed") : NEO_HIP_OK;
    if (!rc) rc = load_impulse(h, ir, length, normalize, is_device, parts, &d, nullptr, h->stream);
    if (!rc) rc = store_perceptual(h, parts, pp, w, &mask, &tmp);
    return set_end(h, rc, {tmp, d, parts, mask});
}

NEO_HIP_API int neo_hip_upols_sparse_info(neo_hip_upols* h, int64_t* kept_bins, int64_t* kept_tiles, int64_t* filter_bytes)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (!h->sparse) return fail(NEO_HIP_EINVAL, "sparse_info: not a sparse handle");
    // from a live update's call on: the bank being faded to
    const int64_t bins = h->fade_left > 0 ? h->sp2.bins : h->sp_bins, tiles = h->fade_left > 0 ? h->sp2.tiles : h->sp_tiles;
    if (kept_bins) *kept_bins = bins;
    if (kept_tiles) *kept_tiles = tiles;
    if (filter_bytes)  // the compacted tiles, the bitmaps and the offsets: what stands in for the [C][R][B] filter
        *filter_bytes = tiles * int64_t(kSparseTile * sizeof(cf)) +
                        int64_t(h->C) * (int64_t(h->P) * sparse_words(h->B) + h->P + 1) * int64_t(sizeof(uint32_t));
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_sparse_window_plan(const uint32_t* tile_mask, int channels, int block, int partitions,
                                                 int window, uint32_t* win_mask, int64_t* window_tiles)
{
    if (!sparse_window_plan(tile_mask, channels, block, partitions, window, win_mask, window_tiles))
        return fail(NEO_HIP_EINVAL, "sparse_window_plan: null pointer, channels or partitions < 1, block not a power of "
                                    "two in [16, 4096], or window not a power of two in [2, 32]");
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_sparse_batch_info(neo_hip_upols* h, int* blocks_per_pass, int* splits, int64_t* window_tiles)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (!h->sparse) return fail(NEO_HIP_EINVAL, "sparse_batch_info: not a sparse handle");
    if (blocks_per_pass) *blocks_per_pass = batch_blocks(h);
    if (splits) *splits = h->shape.Sb;
    if (window_tiles) *window_tiles = h->sp_wtiles;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_sparse_plan(const uint8_t* mask, int channels, int block, int partitions,
                                          uint32_t* tile_mask, uint32_t* row_off, int64_t* kept_bins, int64_t* kept_tiles)
{
    if (!sparse_plan(mask, channels, block, partitions, tile_mask, row_off, kept_bins, kept_tiles))
        return fail(NEO_HIP_EINVAL, "sparse_plan: null pointer, channels or partitions < 1, or block not a power of two "
                                    "in [16, 4096]");
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_create(int channels, int block, int partitions, int device, neo_hip_upols** out)
{
    return create_convolver(channels, block, partitions, device, upols_kind::dense, false, nullptr, out);
}

NEO_HIP_API int neo_hip_upola_create(int channels, int block, int partitions, int device, neo_hip_upols** out)
{
    return create_convolver(channels, block, partitions, device, upols_kind::dense, true, nullptr, out);
}

NEO_HIP_API int neo_hip_upola2_create(int channels, int block, int partitions, int device, neo_hip_upols** out)
{
    return create_convolver(channels, block, partitions, device, upols_kind::v2, true, nullptr, out);
}

NEO_HIP_API int neo_hip_upols_create_ex(int channels, int block, int partitions, int device, int method,
                                        const neo_hip_upols_opts* opts, neo_hip_upols** out)
{
    if (method < 0 || method > 2) return fail(NEO_HIP_EINVAL, "method must be 0 (upols), 1 (upola) or 2 (upola v2)");
    return create_convolver(channels, block, partitions, device, method == 2 ? upols_kind::v2 : upols_kind::dense,
                            method >= 1, opts, out);
}

NEO_HIP_API int neo_hip_upols_destroy(neo_hip_upols* h)
{
    if (!h) return NEO_HIP_OK;
    device_guard g(h->device);
    (void)persist_stop(h);
    (void)setup_join(h);
    destroy(h);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_info(neo_hip_upols* h, int* channels, int* block, int* partitions, int* splits)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (channels) *channels = h->C;
    if (block) *block = h->B;
    if (partitions) *partitions = h->P;
    if (splits) *splits = h->shape.S;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_reset(neo_hip_upols* h)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    device_guard g(h->device);
    if (int rc = set_begin(h, false)) return rc;  // after this handle's steps on any stream
    if (h->fade_left > 0) fade_swap(h);  // a running fade completes: the new filter is the filter
    if (h->sparse) sparse_release_spare(h);  // joined above: a retired sparse bank's tiles go back
    int rc = reset_state(h, h->stream);
    if (!rc) rc = lvl_setup_prime(h);  // the next call is an ordinary streaming step
    if (rc) return rc;
    NEO_HIP_CHECK(hipStreamSynchronize(h->stream));
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_set_filter(neo_hip_upols* h, const void* filter, int is_device)
{
    if (!h || !filter) return fail(NEO_HIP_EINVAL, "null handle or filter");
    if (h->sparse)
        return fail(NEO_HIP_EINVAL, "set_filter: a sparse handle keeps no dense filter (neo_hip_upols_set_filter_sparse)");
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = set_begin(h, is_device != 0)) return rc;
    cf* tmp = nullptr;
    const cf* src = nullptr;
    int rc = stage_in(static_cast<const cf*>(filter), filter_elems(h) * sizeof(cf), is_device != 0, false, h->stream, &tmp, &src);
    if (!rc) rc = pack_filter(h, src, h->stream);
    return set_end(h, rc, {tmp});
}

NEO_HIP_API int neo_hip_upols_set_impulse(neo_hip_upols* h, const float* ir, int64_t length, int normalize,
                                          int is_device)
{
    if (!h || !ir || length < 1) return fail(NEO_HIP_EINVAL, "null handle/ir or empty impulse");
    if (h->sparse)
        return fail(NEO_HIP_EINVAL, "set_impulse: a sparse handle takes a partitioned filter and its mask "
                                    "(neo_hip_upols_set_filter_sparse)");
    if (int rc = check_impulse(h, length)) return rc;
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = set_begin(h, is_device != 0)) return rc;
    float* d = nullptr;
    const int rc = load_impulse(h, ir, length, normalize, is_device, nullptr, &d, h->H, h->stream);
    return set_end(h, rc, {d});
}

NEO_HIP_API int neo_hip_upols_update_filter(neo_hip_upols* h, const void* filter, int is_device, int fade_blocks,
                                            int curve, void* stream)
{
    if (!h || !filter) return fail(NEO_HIP_EINVAL, "null handle or filter");
    if (int rc = update_check(h, fade_blocks, curve)) return rc;
    device_guard g(h->device);
    if (g.rc) return g.rc;
    hipStream_t s = update_stream(h, is_device, stream);
    if (int rc = update_begin(h, is_device != 0, s)) return rc;
    if (int rc = fade_buffers(h, s)) return rc;
    cf* tmp = nullptr;
    const cf* src = nullptr;
    int rc = stage_in(static_cast<const cf*>(filter), filter_elems(h) * sizeof(cf), is_device != 0, false, s, &tmp, &src);
    if (!rc) rc = pack_filter(h, src, s, h->H2);
    rc = update_end(h, rc, is_device != 0, fade_blocks, curve, s);
    dfree(tmp);  // a host filter's staging: s was joined above
    return rc;
}

NEO_HIP_API int neo_hip_upols_update_impulse(neo_hip_upols* h, const float* ir, int64_t length, int normalize,
                                             int is_device, int fade_blocks, int curve, void* stream)
{
    if (!h || !ir || length < 1) return fail(NEO_HIP_EINVAL, "null handle/ir or empty impulse");
    if (int rc = update_check(h, fade_blocks, curve)) return rc;
    if (int rc = check_impulse(h, length)) return rc;
    device_guard g(h->device);
    if (g.rc) return g.rc;
    hipStream_t s = update_stream(h, is_device, stream);
    if (int rc = update_begin(h, is_device != 0, s)) return rc;
    if (int rc = fade_buffers(h, s)) return rc;
    // the impulse's working copy: a device impulse leaves the call asynchronous, so its copy is
    // stream-ordered scratch; a host one is staged in pooled scratch and the call waits for s
    float* d = nullptr;
    int rc = load_impulse(h, ir, length, normalize, is_device, nullptr, &d, h->H2, s, is_device != 0);
    if (is_device && d && hipFreeAsync(d, s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "impulse scratch free failed");
    rc = update_end(h, rc, is_device != 0, fade_blocks, curve, s);
    if (!is_device) dfree(d);
    return rc;
}

NEO_HIP_API int neo_hip_upols_update_filter_sparse(neo_hip_upols* h, const void* filter, const uint8_t* mask, int is_device,
                                                   int fade_blocks, int curve, void* stream)
{
    if (!h || !filter || !mask) return fail(NEO_HIP_EINVAL, "update_filter_sparse: null handle, filter or mask");
    if (int rc = update_check(h, fade_blocks, curve, true)) return rc;
    return sparse_update(h, is_device, fade_blocks, curve, stream,
                         [&](hipStream_t s, const cf** f, const uint8_t** m, std::vector<void*>& scratch) {
                             const size_t n = filter_elems(h);
                             cf* tmpf = nullptr;
                             uint8_t* tmpm = nullptr;
                             int rc = stage_in(static_cast<const cf*>(filter), n * sizeof(cf), is_device != 0, false, s, &tmpf, f);
                             if (tmpf) scratch.push_back(tmpf);
                             if (!rc) rc = stage_in(mask, n, is_device != 0, false, s, &tmpm, m);
                             if (tmpm) scratch.push_back(tmpm);
                             return rc;
                         });
}

NEO_HIP_API int neo_hip_upols_update_filter_perceptual(neo_hip_upols* h, const void* filter, const neo_hip_perceptual* pp,
                                                       int is_device, int fade_blocks, int curve, void* stream)
{
    if (int rc = check_perceptual("update_filter_perceptual", h, filter, pp)) return rc;
    if (int rc = update_check(h, fade_blocks, curve, true)) return rc;
    const std::vector<float> w = weights_for(h, pp);  // alive until the call's last wait on its stream
    return sparse_update(h, is_device, fade_blocks, curve, stream,
                         [&](hipStream_t s, const cf** f, const uint8_t** m, std::vector<void*>& scratch) {
                             cf* tmpf = nullptr;
                             uint8_t* msk = nullptr;
                             float* tmp = nullptr;
                             int rc = stage_in(static_cast<const cf*>(filter), filter_elems(h) * sizeof(cf), is_device != 0, false,
                                               s, &tmpf, f);
                             if (tmpf) scratch.push_back(tmpf);
                             if (!rc && dalloc(&msk, filter_elems(h))) rc = fail(NEO_HIP_ENOMEM, "allocation failed");
                             if (msk) scratch.push_back(msk);
                             if (!rc) rc = perceptual_mask_device(*f, h->C, h->B, h->P, pp, w.data(), msk, &tmp, s);
                             if (tmp) scratch.push_back(tmp);
                             *m = msk;
                             return rc;
                         });
}

NEO_HIP_API int neo_hip_upols_update_impulse_perceptual(neo_hip_upols* h, const float* ir, int64_t length, int normalize,
                                                        const neo_hip_perceptual* pp, int is_device, int fade_blocks,
                                                        int curve, void* stream)
{
    if (length < 1) return fail(NEO_HIP_EINVAL, "update_impulse_perceptual: empty impulse");
    if (int rc = check_perceptual("update_impulse_perceptual", h, ir, pp)) return rc;
    if (int rc = update_check(h, fade_blocks, curve, true)) return rc;
    if (int rc = check_impulse(h, length)) return rc;
    const std::vector<float> w = weights_for(h, pp);
    return sparse_update(h, is_device, fade_blocks, curve, stream,
                         [&](hipStream_t s, const cf** f, const uint8_t** m, std::vector<void*>& scratch) {
                             cf* parts = nullptr;
                             uint8_t* msk = nullptr;
                             float *d = nullptr, *tmp = nullptr;
                             int rc = dalloc(&parts, filter_elems(h) * sizeof(cf)) ? fail(NEO_HIP_ENOMEM, "allocation failed")
                                                                                  : NEO_HIP_OK;
                             if (parts) scratch.push_back(parts);
                             if (!rc) rc = load_impulse(h, ir, length, normalize, is_device, parts, &d, nullptr, s);
                             if (d) scratch.push_back(d);
                             if (!rc && dalloc(&msk, filter_elems(h))) rc = fail(NEO_HIP_ENOMEM, "allocation failed");
                             if (msk) scratch.push_back(msk);
                             if (!rc) rc = perceptual_mask_device(parts, h->C, h->B, h->P, pp, w.data(), msk, &tmp, s);
                             if (tmp) scratch.push_back(tmp);
                             *f = parts;
                             *m = msk;
                             return rc;
                         });
}

NEO_HIP_API int neo_hip_upols_sparse_fade_plan(const uint8_t* mask_a, const uint8_t* mask_b, int channels, int block,
                                               int partitions, int64_t* tiles_a, int64_t* tiles_b, int64_t* tiles_union,
                                               int* splits, int64_t* step_bytes)
{
    // the splits of a sparse handle of this shape with default options (the fade step runs the plain step's)
    upols_shape shape;
    sparse_fade_cost f;
    const char* why = make_upols_shape(channels, block, partitions, nullptr, upols_kind::sparse, false, shape);
    if (why || !sparse_fade_plan(mask_a, mask_b, channels, block, partitions, upols_fade_split(shape).S, &f))
        return fail(NEO_HIP_EINVAL, "sparse_fade_plan: %s", why ? why : "null mask");
    if (tiles_a) *tiles_a = f.tiles_a;
    if (tiles_b) *tiles_b = f.tiles_b;
    if (tiles_union) *tiles_union = f.tiles_union;
    if (splits) *splits = upols_fade_split(shape).S;
    if (step_bytes) *step_bytes = f.step_bytes;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_fade_info(neo_hip_upols* h, int* remaining_blocks, int* fade_blocks, int64_t* bank_bytes)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (remaining_blocks) *remaining_blocks = h->fade_left;
    if (fade_blocks) *fade_blocks = h->fade_total;
    // dense: the second bank [C][ring][B]; sparse: the spare bank's tables plus the tiles it holds
    if (bank_bytes) *bank_bytes = h->sparse ? sparse_spare_bytes(h) : h->H2 ? upols_fade_split(h->shape).bank_bytes : 0;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_process_device(neo_hip_upols* h, const float* in, int64_t ld_in, float* out,
                                             int64_t ld_out, void* stream)
{
    if (!h || !in || !out) return fail(NEO_HIP_EINVAL, "null handle or buffer");
    if (ld_in < h->B || ld_out < h->B) return fail(NEO_HIP_EINVAL, "leading dimension smaller than the block");
    if (!io_aligned(in, out, ld_in, ld_out))
        return fail(NEO_HIP_EINVAL, "device I/O must be 16-byte aligned (ld multiple of 4)");
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (h->v2) return process_samples(h, in, ld_in, out, ld_out, h->B, as_stream(stream));  // may be mid-block
    return launch_step(h, in, ld_in, out, ld_out, as_stream(stream));  // NULL = HIP null stream
}

NEO_HIP_API int neo_hip_upols_process_blocks(neo_hip_upols* h, const float* in, float* out, int64_t ld, int64_t nblocks,
                                             void* stream)
{
    if (!h || !in || !out) return fail(NEO_HIP_EINVAL, "null handle or buffer");
    if (nblocks < 0 || ld < nblocks * h->B) return fail(NEO_HIP_EINVAL, "ld < nblocks * block");
    if (!io_aligned(in, out, ld, ld))
        return fail(NEO_HIP_EINVAL, "device I/O must be 16-byte aligned (ld multiple of 4)");
    device_guard g(h->device);
    if (g.rc) return g.rc;
    // whole groups of T blocks per pass (batching on), the rest one block per pass
    return process_samples(h, in, ld, out, ld, nblocks * h->B, as_stream(stream));
}

NEO_HIP_API int neo_hip_upols_process(neo_hip_upols* h, float* io, int io_is_device, void* stream)
{
    if (!h || !io) return fail(NEO_HIP_EINVAL, "null handle or buffer");
    if (io_is_device) return neo_hip_upols_process_device(h, io, h->B, io, h->B, stream);
    device_guard g(h->device);
    if (g.rc) return g.rc;
    hipStream_t s = stream ? as_stream(stream) : h->stream;  // host I/O: own stream unless given
    const size_t bytes = size_t(h->C) * h->B * sizeof(float);
    // Host buffers (the plugin's processFrame pattern, DenseConvolution.cpp:62-74): the step
    // kernel reads the block from host memory and writes the output back itself over PCIe
    // (zero-copy, no DMA launches). Page-locked memory (neo_hip_host_register, hipHostMalloc)
    // is used in place; any other buffer goes through the handle's mapped pinned staging.
    float* dio = host_mapped(io);
    const bool staged = !dio || (reinterpret_cast<uintptr_t>(dio) & 15);
    if (staged) {
        if (!h->io_host) {
            if (int rc = halloc(reinterpret_cast<void**>(&h->io_host), reinterpret_cast<void**>(&h->io), bytes)) return rc;
        }
        std::memcpy(h->io_host, io, bytes);
        dio = h->io;
    }
    int rc = h->v2 ? process_samples(h, dio, h->B, dio, h->B, h->B, s) : launch_step(h, dio, h->B, dio, h->B, s);
    if (rc) return rc;
    if ((rc = spin_sync(s))) return rc;  // the block's deadline: poll, do not yield the thread
    if (staged) std::memcpy(io, h->io_host, bytes);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_process_samples(neo_hip_upols* h, const float* in, int64_t ld_in, float* out,
                                              int64_t ld_out, int64_t num_samples, int is_device, void* stream)
{
    if (!h || !in || !out) return fail(NEO_HIP_EINVAL, "null handle or buffer");
    if (num_samples < 0 || ld_in < num_samples || ld_out < num_samples)
        return fail(NEO_HIP_EINVAL, "num_samples must be in [0, ld]");
    if (num_samples == 0) return NEO_HIP_OK;
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (is_device) return process_samples(h, in, ld_in, out, ld_out, num_samples, as_stream(stream));
    hipStream_t s = stream ? as_stream(stream) : h->stream;
    // host I/O: pinned staging (grown on demand), 1-D copies, synchronous like process()
    const size_t count = size_t(h->C) * size_t(num_samples);
    if (count > h->samples_cap) {
        NEO_HIP_CHECK(hipStreamSynchronize(s));  // no queued work on the old staging
        dfree(h->samples_dev);
        hfree(h->samples_host);
        h->samples_dev = nullptr;
        h->samples_host = nullptr;
        h->samples_cap = 0;
        if (int rc = dalloc(&h->samples_dev, count * sizeof(float))) return rc;
        void* dmap = nullptr;  // not used: the samples go by DMA
        if (int rc = halloc(reinterpret_cast<void**>(&h->samples_host), &dmap, count * sizeof(float))) return rc;
        h->samples_cap = count;
    }
    for (int c = 0; c < h->C; ++c)
        std::copy(in + c * ld_in, in + c * ld_in + num_samples, h->samples_host + size_t(c) * num_samples);
    NEO_HIP_CHECK(hipMemcpyAsync(h->samples_dev, h->samples_host, count * sizeof(float), hipMemcpyHostToDevice, s));
    int rc = process_samples(h, h->samples_dev, num_samples, h->samples_dev, num_samples, num_samples, s);
    if (rc) return rc;
    NEO_HIP_CHECK(hipMemcpyAsync(h->samples_host, h->samples_dev, count * sizeof(float), hipMemcpyDeviceToHost, s));
    NEO_HIP_CHECK(hipStreamSynchronize(s));
    for (int c = 0; c < h->C; ++c)
        std::copy(h->samples_host + size_t(c) * num_samples, h->samples_host + size_t(c + 1) * num_samples,
                  out + c * ld_out);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_batch_info(neo_hip_upols* h, int* blocks_per_pass, int* splits)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (blocks_per_pass) *blocks_per_pass = h->shape.batch ? batch_blocks(h) : 1;
    if (splits) *splits = h->shape.batch ? h->shape.Sb : h->shape.S;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_set_batch(neo_hip_upols* h, int enable)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (enable && h->ring - h->P < batch_blocks(h) - 1)
        return fail(NEO_HIP_EINVAL, "the FDL ring is too short for a batch of %d blocks", batch_blocks(h));
    h->shape.batch = enable != 0;  // (a sparse handle: off until asked for; its batched MAC is k_sparse_batch_mac)
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_set_offline(neo_hip_upols* h, int enable)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (enable && h->sparse) return fail(NEO_HIP_EINVAL, "a sparse handle has no offline windows (no dense filter spectra)");
    if (enable && (h->v2 || h->P < kOffMinP))
        return fail(NEO_HIP_EINVAL, "offline windows take whole-block handles of >= %d partitions", kOffMinP);
    h->shape.off = enable != 0;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_get_offline(neo_hip_upols* h, int* enabled, int* segments)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (enabled) *enabled = h->shape.off;
    if (segments) *segments = h->shape.off_nseg;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_set_ahead(neo_hip_upols* h, int enable)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (enable && h->sparse) return fail(NEO_HIP_EINVAL, "a sparse handle has no streaming levels (no dense filter)");
    if (enable && h->v2) return fail(NEO_HIP_EINVAL, "streaming levels are for whole-block upols / upola handles");
    if (enable && h->B > 1024) return fail(NEO_HIP_EINVAL, "streaming levels take blocks up to 1024");
    device_guard g(h->device);
    if (int rc = persist_stop(h)) return rc;
    if (!enable) h->sched.persist = false;  // the latency mode runs the levels
    h->shape.ahead = enable != 0;
    h->lv_n = -1;  // the FDL is complete at any block boundary: the next step primes the levels
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_set_paced(neo_hip_upols* h, int enable)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (enable < 0 || enable > 2) return fail(NEO_HIP_EINVAL, "paced: 0 off, 1 a piece per call, 2 two pieces per group");
    if (enable && h->sparse) return fail(NEO_HIP_EINVAL, "a sparse handle has no background work to pace (no streaming levels)");
    if (enable == h->paced) return NEO_HIP_OK;
    if (int rc = persist_stop(h)) return rc;  // a resident latency-mode kernel leaves first (lv_n restarts)
    if (int rc = lvl_join(h, h->stream)) return rc;
    NEO_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->paced = enable;
    h->lv_n = -1;  // the levels re-prime: no group is half issued in the other form
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_set_persistent(neo_hip_upols* h, int enable, double idle_ms)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (enable) {
        if (h->sparse) return fail(NEO_HIP_EINVAL, "latency mode: a sparse handle has no persistent step");
        if (const char* why = persist_ineligible(h)) return fail(NEO_HIP_EINVAL, "latency mode: %s", why);
        if (h->fade_left > 0)
            return fail(NEO_HIP_EINVAL, "latency mode: a filter fade is still running (%d blocks left)", h->fade_left);
        if (!(idle_ms > 0.0 && idle_ms <= 10000.0)) return fail(NEO_HIP_EINVAL, "idle_ms must be in (0, 10000]");
        if (int rc = setup_join(h)) return rc;  // this handle's steps queued on any stream come first
        h->ps_idle_ms = idle_ms;
        h->sched.persist = true;
        h->ps_valid = false;  // the persistent schedule primes the levels at its first block
        return NEO_HIP_OK;
    }
    h->sched.persist = false;
    return persist_stop(h);
}

NEO_HIP_API int neo_hip_upols_get_persistent(neo_hip_upols* h, int* enabled, int* running, int64_t* launches)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (enabled) *enabled = h->sched.persist;
    if (running) *running = h->ps_running && h->ps_mb && __atomic_load_n(&h->ps_mb->alive, __ATOMIC_ACQUIRE);
    if (launches) *launches = h->ps_launches;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_persist_step_times(neo_hip_upols* h, double* us, int64_t cap, int64_t* count)
{
    if (!h || (cap > 0 && !us)) return fail(NEO_HIP_EINVAL, "null handle or output");
    if (count) *count = 0;
    if (!h->ps_tl || h->lv_n <= h->ps_n0 || !h->ps_valid) return NEO_HIP_OK;
    device_guard g(h->device);
    if (g.rc) return g.rc;
    std::vector<unsigned long long> tl(2 * kPsRing);
    NEO_HIP_CHECK(hipMemcpy(tl.data(), h->ps_tl, tl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    // the last min(kPsRing - 1, steps of this launch) steps, oldest first
    const int64_t last = h->lv_n - 1, k = std::min<int64_t>({int64_t(kPsRing) - 1, last - h->ps_n0 + 1, cap});
    for (int64_t i = 0; i < k; ++i) {
        const int64_t n = last - k + 1 + i, slot = n % kPsRing;
        us[i] = double(tl[size_t(2 * slot + 1)] - tl[size_t(2 * slot)]) * 1e-2;  // 100 MHz ticks -> us
    }
    if (count) *count = k;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_get_ahead(neo_hip_upols* h, int* enabled, int* phase, int* window, int* splits)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (enabled) *enabled = h->shape.ahead;
    if (phase) *phase = int(h->lv_n < 0 ? 0 : h->lv_n % kFarT);
    if (window) *window = h->sched.lv.nseg ? kFarT : (h->sched.lv.n ? h->sched.lv.T[h->sched.lv.n - 1] : 1);
    if (splits) *splits = h->sched.lv.n + (h->sched.lv.nseg ? 1 : 0);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_set_timing(neo_hip_upols* h, int enable)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (enable < 0) return fail(NEO_HIP_EINVAL, "timing stride %d < 0", enable);
    h->timing = enable;
    h->tick = 0;
    return NEO_HIP_OK;
}

// fold the recorded event groups into the per-part sums and the per-group totals
static int drain_events(upols_t* h)
{
    for (size_t i = 0; i < h->events_used; ++i) {
        const auto& e = h->events[i];
        NEO_HIP_CHECK(hipEventSynchronize(e.e[e.n - 1]));
        float tot = 0.f;
        NEO_HIP_CHECK(hipEventElapsedTime(&tot, e.e[0], e.e[e.n - 1]));
        if (e.part == 0) h->group_ms.push_back(tot);  // step times: the caller's stream only
        for (int k = 0; k + 1 < e.n; ++k) {
            float t = 0.f;
            NEO_HIP_CHECK(hipEventElapsedTime(&t, e.e[k], e.e[k + 1]));
            h->part_ms[k + e.part] += t;
            ++h->part_n[k + e.part];
        }
        if (e.n >= 3) {
            h->part_ms[3] += tot;
            ++h->part_n[3];
        }
    }
    h->events_used = 0;
    return NEO_HIP_OK;
}

// forget the drained times: the per-part sums and the per-group totals
static void clear_timing(upols_t* h)
{
    h->group_ms.clear();
    for (int k = 0; k < 4; ++k) {
        h->part_ms[k] = 0.0;
        h->part_n[k] = 0;
    }
}

NEO_HIP_API int neo_hip_upols_timing_detail(neo_hip_upols* h, double* ms, int64_t* launches)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    device_guard g(h->device);
    if (int rc = drain_events(h)) return rc;
    for (int k = 0; k < 4; ++k) {
        if (ms) ms[k] = h->part_ms[k];
        if (launches) launches[k] = h->part_n[k];
    }
    clear_timing(h);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_step_times(neo_hip_upols* h, double* ms, int64_t cap, int64_t* count)
{
    if (!h || (cap > 0 && !ms)) return fail(NEO_HIP_EINVAL, "null handle or buffer");
    device_guard g(h->device);
    if (int rc = drain_events(h)) return rc;
    const int64_t n = int64_t(h->group_ms.size());
    for (int64_t i = 0; i < std::min(n, cap); ++i) ms[i] = h->group_ms[size_t(i)];
    if (count) *count = n;
    clear_timing(h);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols_timing(neo_hip_upols* h, double* mac_ms, int64_t* launches)
{
    double ms[4];
    int64_t n[4];
    int rc = neo_hip_upols_timing_detail(h, ms, n);
    if (rc) return rc;
    const int k = n[3] ? 3 : 0;  // streaming-level steps: the whole step; else the MAC kernel
    if (mac_ms) *mac_ms = ms[k];
    if (launches) *launches = n[k];
    return NEO_HIP_OK;
}

}  // extern "C"
