// upols_f64_batch.hip — batched passes of the double-precision UPOLS / UPOLA convolvers: T
// consecutive blocks of every channel per read of the filter and the delay line (the plain step,
// upols_f64.hip, reads both once per block). The index rules and the plan are upols_f64_plan.hpp's.
//   k_upols64_bwindow   launch 1, grid C x T: block j's 2B window, r2c, spectrum into scratch row N[j]
//   k_upols64_bmac      launch 2, one workgroup per (channel, split, 256 bins): T accumulators and a
//                       sliding window of T delay-line rows per lane, ascending p, one slab row per block
//   k_upols64_bfinish   launch 3, grid C x T: slabs in order, c2r, output; the last min(T, P) blocks
//                       commit their scratch row to the ring; the last block saves prev
//   k_upols64_bola      launch 4, overlap-add only, grid C x T: out_j += tail_{j-1}, overlap = tail_{T-1}
// Fixed order, no atomics: equal calls give equal bits. The ring is written in launch 3 alone, after
// every MAC workgroup has read it.
#include "upols_f64_handle.hpp"

#include <algorithm>

namespace neo_hip {

// Block j of channel c: the window (overlap-save: x_{j-1} | x_j with x_{-1} = prev; overlap-add:
// x_j | zeros), the B-point complex Stockham and the r2c split as k_upols64_step does them, the
// spectrum into the scratch row N[c][j]. prev and the ring are read only.
template<int B, bool OLA>
__global__ __launch_bounds__(256) void k_upols64_bwindow(const double* __restrict__ in, int64_t ld_in,
                                                         const double* __restrict__ prev, cd* __restrict__ N,
                                                         const cd* __restrict__ twg)
{
    using K = cfg64<B>;
    constexpr int E = K::EW, T = B / E;
    static_assert(T <= 256 && B % E == 0, "window FFT must fit one 256-lane workgroup");
    __shared__ cd fft[K::LL];
    __shared__ cd tw[K::TW1 + K::TW2];
    const int tid = threadIdx.x, c = blockIdx.x, j = blockIdx.y;
    const bool active = tid < T;
    for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];
    const cd* iz = reinterpret_cast<const cd*>(in + int64_t(c) * ld_in + int64_t(j) * B);  // z[n] = w[2n] + i w[2n+1]
    const cd* pz = j == 0 ? reinterpret_cast<const cd*>(prev + int64_t(c) * B) : iz - B / 2;
    cd v[E];
    if (active) {
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int n = tid + m * T;
            if constexpr (OLA) v[m] = n < B / 2 ? iz[n] : cd{0.0, 0.0};
            else v[m] = n < B / 2 ? pz[n] : iz[n - B / 2];
        }
    }
    __syncthreads();
    stockham<B, E, -1>(v, fft, tw, tid, active);
    if (active) {
#pragma unroll
        for (int m = 0; m < E; ++m) fft[lpad(tid + m * T)] = v[m];
    }
    __syncthreads();
    cd* row = N + (int64_t(c) * gridDim.y + j) * B;
    for (int q = tid; q < B; q += 256) row[q] = r2c_split<B>(fft, tw + K::TW1, q);
}

// One bin per lane, T blocks per lane. At partition p block j needs window row e = j - p
// (upols64_window_src); a step on, block j needs what block j - 1 held, so the T rows stay in
// registers and one row enters per partition: the ring row of e = -(p + 1), for block 0. The loop is
// unrolled T steps at a time so that every register index is a constant: at step k of a chunk block
// j's row is slot (j - k) mod T, and the row that enters replaces the one block T - 1 is done with.
// Only the prologue can meet a scratch row (e >= 0). Filter and entering rows are loaded U steps
// ahead. Steps of the last chunk past the split's end multiply by a zero filter value. Packed bin 0 holds two real products (DC, Nyquist): its lane multiplies by
// (hr, 0 | hi, 0) where the others take (hr, -hi | hr, hi), so the cross terms add an exact zero.
// Rows shorter than the workgroup: RPI splits share a workgroup.
template<int B, int T>
__global__ __launch_bounds__(256) void k_upols64_bmac(const cd* __restrict__ H, const cd* __restrict__ fdl,
                                                      const cd* __restrict__ N, cd* __restrict__ bpart, int P, int S,
                                                      int rows, int w)
{
    using K = cfg64<B>;
    constexpr int U = 4;
    static_assert(T % U == 0, "the prefetch slots rotate inside a chunk");
    const int tid = threadIdx.x, c = blockIdx.x;
    const int s = blockIdx.y * K::RPI + tid / K::QT;
    if (s >= S) return;
    const int q = blockIdx.z * K::QT + tid % K::QT;
    const int p0 = s * rows, p1 = min(P, p0 + rows);
    const cd* Hc = H + int64_t(c) * P * B + q;
    const cd* Fc = fdl + int64_t(c) * P * B + q;
    const cd* Nc = N + int64_t(c) * T * B + q;
    const bool bin0 = q == 0;

    cd acc[T], win[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        acc[j] = cd{0.0, 0.0};
        const upols64_row_src r = upols64_window_src(j - p0, w, P);
        win[j] = ld_nt((r.scratch ? Nc : Fc) + int64_t(r.row) * B);
    }
    // step p takes filter row p and hands on the ring row of e = -(p + 1); past the split's end both
    // loads stay on the split's last rows (no branch, nothing read outside the split) and the filter
    // value is zeroed: what enters then meets zeros only
    const int plast = p1 - 1;
    auto filter_row = [&](int p) {
        const cd h = ld_nt(Hc + int64_t(min(p, plast)) * B);
        return p < p1 ? h : cd{0.0, 0.0};
    };
    auto entering_row = [&](int p) {
        const int r = w - min(p + 1, plast);
        return ld_nt(Fc + int64_t(r < 0 ? r + P : r) * B);
    };
    cd hq[U], xq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        hq[u] = filter_row(p0 + u);
        xq[u] = entering_row(p0 + u);
    }
#pragma unroll 1
    for (int base = p0; base < p1; base += T) {
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const cd h = hq[k % U], xin = xq[k % U];
            hq[k % U] = filter_row(base + k + U);
            xq[k % U] = entering_row(base + k + U);
            const double a = h.x, b = bin0 ? 0.0 : -h.y, c2 = bin0 ? h.y : h.x, d = bin0 ? 0.0 : h.y;
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const cd x = win[(j - k + T) % T];
                acc[j].x = fma(b, x.y, fma(a, x.x, acc[j].x));
                acc[j].y = fma(d, x.x, fma(c2, x.y, acc[j].y));
            }
            win[(T - 1 - k) % T] = xin;
            // keep the scheduler from hoisting the whole chunk's loads to its top: U steps of
            // prefetch hold 8 U VGPRs, T steps would not fit
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    cd* slab = bpart + (int64_t(c) * S + s) * T * B + q;
#pragma unroll
    for (int j = 0; j < T; ++j) slab[int64_t(j) * B] = acc[j];
}

// Block j of channel c: the S slab rows of the block summed in the order s = 0..S-1, the c2r join,
// the inverse Stockham and the double scale 1/(2B) as k_upols64_finish does them. Overlap-save:
// out_j = window samples [B, 2B). Overlap-add: out_j = samples [0, B), tail row j = samples [B, 2B)
// (k_upols64_bola adds the tails). Before any of it the workgroup commits its scratch row to the ring
// (upols64_commit_row) and, overlap-save and j = T - 1, saves x_{T-1} as the next prev: out_{T-1} may
// alias it, and the barriers of the transform lie between the two.
template<int B, bool OLA>
__global__ __launch_bounds__(256) void k_upols64_bfinish(const cd* __restrict__ bpart, const cd* __restrict__ N,
                                                         cd* __restrict__ fdl, const double* in, int64_t ld_in,
                                                         double* __restrict__ prev, double* out, int64_t ld_out,
                                                         double* __restrict__ tails, const cd* __restrict__ twg, int P,
                                                         int S, int w)
{
    using K = cfg64<B>;
    constexpr int E = K::EF, T = B / E;
    static_assert(T <= 256 && B % E == 0, "c2r must fit one 256-lane workgroup");
    __shared__ cd fft[K::LL];
    __shared__ cd tw[K::TW1 + K::TW2];
    const int tid = threadIdx.x, c = blockIdx.x, j = blockIdx.y, TB = gridDim.y;
    for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];
    if (const int row = upols64_commit_row(j, TB, P, w); row >= 0) {
        const cd* src = N + (int64_t(c) * TB + j) * B;
        cd* dst = fdl + (int64_t(c) * P + row) * B;
        for (int k = tid; k < B; k += 256) dst[k] = src[k];
    }
    if constexpr (!OLA) {
        if (j == TB - 1) {
            const cd* iz = reinterpret_cast<const cd*>(in + int64_t(c) * ld_in + int64_t(j) * B);
            cd* pz = reinterpret_cast<cd*>(prev + int64_t(c) * B);
            for (int i = tid; i < B / 2; i += 256) pz[i] = iz[i];
        }
    }
    const cd* pc = bpart + (int64_t(c) * S * TB + j) * B;
    const int64_t ss = int64_t(TB) * B;  // from split to split
    for (int k = tid; k < B; k += 256) {
        cd sum = pc[k];
        int t = 1;
        for (; t + 3 < S; t += 4) {
            cd r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = pc[(t + u) * ss + k];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                sum.x += r[u].x;
                sum.y += r[u].y;
            }
        }
        for (; t < S; ++t) {
            const cd r = pc[t * ss + k];
            sum.x += r.x;
            sum.y += r.y;
        }
        fft[k] = sum;
    }
    __syncthreads();
    const bool active = tid < T;
    cd v[E];
    if (active) {
        const cd x0 = fft[0];
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int k = tid + m * T;
            v[m] = k == 0 ? c2r_join<B>(cd{x0.x, 0.0}, cd{x0.y, 0.0}, tw + K::TW1, 0)
                          : c2r_join<B>(fft[k], fft[B - k], tw + K::TW1, k);
        }
    }
    __syncthreads();  // the spectrum is in registers: the tile is the transform's from here
    stockham<B, E, +1>(v, fft, tw, tid, active);
    if (active) {
        const double scale = 1.0 / double(2 * B);
        cd* o = reinterpret_cast<cd*>(out + int64_t(c) * ld_out + int64_t(j) * B);
        if constexpr (OLA) {
            cd* tl = reinterpret_cast<cd*>(tails + (int64_t(c) * TB + j) * B);
#pragma unroll
            for (int m = 0; m < E / 2; ++m) o[tid + m * T] = cd{v[m].x * scale, v[m].y * scale};
#pragma unroll
            for (int m = E / 2; m < E; ++m) tl[tid + m * T - B / 2] = cd{v[m].x * scale, v[m].y * scale};
        } else {
#pragma unroll
            for (int m = E / 2; m < E; ++m) o[tid + m * T - B / 2] = cd{v[m].x * scale, v[m].y * scale};
        }
    }
}

// Overlap-add: out_j += tail_{j-1}, with tail_{-1} the overlap the pass began with; the workgroup of
// j = 0 then stores tail_{T-1} as the next overlap, each lane over the words it has just read.
__global__ __launch_bounds__(256) void k_upols64_bola(double* __restrict__ out, int64_t ld_out,
                                                      const double* __restrict__ tails, double* __restrict__ ovl, int B)
{
    const int c = blockIdx.x, j = blockIdx.y, TB = gridDim.y;
    cd* o = reinterpret_cast<cd*>(out + int64_t(c) * ld_out + int64_t(j) * B);
    const cd* tl = reinterpret_cast<const cd*>(tails + int64_t(c) * TB * B);
    cd* ov = reinterpret_cast<cd*>(ovl + int64_t(c) * B);
    const cd* before = j == 0 ? ov : tl + int64_t(j - 1) * (B / 2);
    const cd* last = tl + int64_t(TB - 1) * (B / 2);
    for (int n = threadIdx.x; n < B / 2; n += 256) {
        const cd a = o[n], t = before[n];
        o[n] = cd{a.x + t.x, a.y + t.y};
        if (j == 0) ov[n] = last[n];
    }
}

void batch_free64(neo_hip_upols64* h)
{
    dfree(h->bscratch);
    dfree(h->bpart);
    dfree(h->btail);
    h->bscratch = nullptr;
    h->bpart = nullptr;
    h->btail = nullptr;
    h->batch = upols64_batch_shape{};
}

template<int B, bool OLA, int T>
static int launch_pass(neo_hip_upols64* h, const double* in, int64_t ld_in, double* out, int64_t ld_out, hipStream_t s)
{
    using K = cfg64<B>;
    const upols64_shape& sh = h->shape;
    const upols64_batch_shape& b = h->batch;
    const dim3 ct(unsigned(sh.C), unsigned(T));
    hipLaunchKernelGGL((k_upols64_bwindow<B, OLA>), ct, dim3(256), 0, s, in, ld_in, h->prev, h->bscratch, h->tw);
    NEO_HIP_LAUNCH_CHECK();
    const dim3 gm(unsigned(sh.C), unsigned((b.S + K::RPI - 1) / K::RPI), unsigned(B / K::QT));
    hipLaunchKernelGGL((k_upols64_bmac<B, T>), gm, dim3(256), 0, s, h->H, h->fdl, h->bscratch, h->bpart, sh.P, b.S, b.rows,
                       h->wpos);
    NEO_HIP_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_upols64_bfinish<B, OLA>), ct, dim3(256), 0, s, h->bpart, h->bscratch, h->fdl, in, ld_in, h->prev,
                       out, ld_out, h->btail, h->tw, sh.P, b.S, h->wpos);
    NEO_HIP_LAUNCH_CHECK();
    if constexpr (OLA) {
        hipLaunchKernelGGL(k_upols64_bola, ct, dim3(256), 0, s, out, ld_out, h->btail, h->prev, B);
        NEO_HIP_LAUNCH_CHECK();
    }
    h->wpos = (h->wpos + T) % sh.P;
    return NEO_HIP_OK;
}

template<int B>
static int launch_pass_of(neo_hip_upols64* h, const double* in, int64_t ld_in, double* out, int64_t ld_out, hipStream_t s)
{
    const bool t16 = h->batch.T == 16;
    if (h->shape.ola)
        return t16 ? launch_pass<B, true, 16>(h, in, ld_in, out, ld_out, s) : launch_pass<B, true, 8>(h, in, ld_in, out, ld_out, s);
    return t16 ? launch_pass<B, false, 16>(h, in, ld_in, out, ld_out, s) : launch_pass<B, false, 8>(h, in, ld_in, out, ld_out, s);
}

int launch_pass64(neo_hip_upols64* h, const double* in, int64_t ld_in, double* out, int64_t ld_out, hipStream_t s)
{
    NEO_UPOLS_DISPATCH(h->shape.B, return launch_pass_of<BB>(h, in, ld_in, out, ld_out, s))
    return NEO_HIP_OK;
}

// Launches 1 and 3 (+ 4) on their own, for the window passes (upols_f64_offline.hip): TB blocks, the
// fresh rows in N [C][TB][B], one slab row per block in `slab` [C][TB][B], the tails in `tails`.
template<int B>
static int launch_bwindow_of(neo_hip_upols64* h, const double* in, int64_t ld_in, cd* N, int TB, hipStream_t s)
{
    const dim3 ct(unsigned(h->shape.C), unsigned(TB));
    if (h->shape.ola) hipLaunchKernelGGL((k_upols64_bwindow<B, true>), ct, dim3(256), 0, s, in, ld_in, h->prev, N, h->tw);
    else hipLaunchKernelGGL((k_upols64_bwindow<B, false>), ct, dim3(256), 0, s, in, ld_in, h->prev, N, h->tw);
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

template<int B>
static int launch_bfinish_of(neo_hip_upols64* h, const cd* slab, const cd* N, double* tails, int TB, const double* in,
                             int64_t ld_in, double* out, int64_t ld_out, hipStream_t s)
{
    const upols64_shape& sh = h->shape;
    const dim3 ct(unsigned(sh.C), unsigned(TB));
    if (sh.ola) {
        hipLaunchKernelGGL((k_upols64_bfinish<B, true>), ct, dim3(256), 0, s, slab, N, h->fdl, in, ld_in, h->prev, out,
                           ld_out, tails, h->tw, sh.P, 1, h->wpos);
        NEO_HIP_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_upols64_bola, ct, dim3(256), 0, s, out, ld_out, tails, h->prev, B);
    } else {
        hipLaunchKernelGGL((k_upols64_bfinish<B, false>), ct, dim3(256), 0, s, slab, N, h->fdl, in, ld_in, h->prev, out,
                           ld_out, tails, h->tw, sh.P, 1, h->wpos);
    }
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

int launch_bwindow64(neo_hip_upols64* h, const double* in, int64_t ld_in, cd* N, int TB, hipStream_t s)
{
    NEO_UPOLS_DISPATCH(h->shape.B, return launch_bwindow_of<BB>(h, in, ld_in, N, TB, s))
    return NEO_HIP_OK;
}

int launch_bfinish64(neo_hip_upols64* h, const cd* slab, const cd* N, double* tails, int TB, const double* in,
                     int64_t ld_in, double* out, int64_t ld_out, hipStream_t s)
{
    NEO_UPOLS_DISPATCH(h->shape.B, return launch_bfinish_of<BB>(h, slab, N, tails, TB, in, ld_in, out, ld_out, s))
    return NEO_HIP_OK;
}

}  // namespace neo_hip

using namespace neo_hip;

extern "C" {

NEO_HIP_API int neo_hip_upols64_set_batch(neo_hip_upols64* h, int blocks)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (blocks < 0) return fail(NEO_HIP_EINVAL, "blocks per pass must be 0 (off), 1 (automatic), 8 or 16");
    upols64_batch_shape b;
    if (blocks)
        if (const char* why = make_upols64_batch_shape(h->shape, blocks, h->split_workgroups, b))
            return fail(NEO_HIP_EINVAL, "%s", why);
    if (b.T == h->batch.T) return NEO_HIP_OK;
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = setup_join64(h, false)) return rc;  // no pass in flight on the buffers that go
    batch_free64(h);
    if (b.T == 1) return NEO_HIP_OK;
    if (dalloc(&h->bscratch, size_t(b.scratch_bytes)) || dalloc(&h->bpart, size_t(b.slab_bytes)) ||
        (b.tail_bytes && dalloc(&h->btail, size_t(b.tail_bytes)))) {
        batch_free64(h);
        return fail(NEO_HIP_ENOMEM, "device allocation of %lld bytes failed", (long long)b.extra_bytes);
    }
    h->batch = b;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols64_batch_info(neo_hip_upols64* h, int* blocks_per_pass, int* splits, int64_t* extra_bytes)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (blocks_per_pass) *blocks_per_pass = h->batch.T;
    if (splits) *splits = h->batch.S;
    if (extra_bytes) *extra_bytes = h->batch.extra_bytes;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols64_batch_plan(int channels, int block, int partitions, int method, int split_workgroups,
                                           int blocks, int* blocks_per_pass, int* splits, int* rows, int64_t* extra_bytes,
                                           int64_t* pass_bytes)
{
    upols64_shape sh;
    if (const char* why = make_upols64_shape(channels, block, partitions, method, split_workgroups, sh))
        return fail(NEO_HIP_EINVAL, "%s", why);
    upols64_batch_shape b;
    if (const char* why = make_upols64_batch_shape(sh, blocks, split_workgroups, b)) return fail(NEO_HIP_EINVAL, "%s", why);
    if (blocks_per_pass) *blocks_per_pass = b.T;
    if (splits) *splits = b.S;
    if (rows) *rows = b.rows;
    if (extra_bytes) *extra_bytes = b.extra_bytes;
    if (pass_bytes) *pass_bytes = b.pass_bytes;
    return NEO_HIP_OK;
}

}  // extern "C"
