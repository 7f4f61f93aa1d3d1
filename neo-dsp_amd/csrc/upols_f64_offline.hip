// upols_f64_offline.hip — offline windows of the double-precision UPOLS / UPOLA convolvers: 128
// consecutive blocks of every channel per pass, computed per bin with 256-point transforms along the
// block axis, so that a bin costs ceil(P / 128) + 2 transforms and ceil(P / 128) spectrum products
// per window where the batched pass (upols_f64_batch.hip) pays P products per block. The rule, the
// row sources and the byte counts are upols_f64_plan.hpp's (upols64_offline_src,
// make_upols64_offline_shape).
//   k_upols64_ohf    setup, grid C nseg x B/8: HF[q] = DFT256 over the partition axis of filter rows
//                    128 q .. 128 q + 127 (zero past P, zero padded), [C][nseg][256][B]
//   k_upols64_bwindow   launch 1 (upols_f64_batch.hip, unchanged), grid C x 128: the fresh rows N
//   k_upols64_omac   launch 2, grid C x B/8: the pairs from the newest back, each pair's older half
//                    loaded once and handed on in registers, one forward transform and one product
//                    with HF[q] per pair, one inverse transform, the 128 rows Y
//   k_upols64_bfinish, k_upols64_bola   launches 3 and 4 (unchanged), grid C x 128, one slab: Y
// A unit is 8 columns (bins) of one channel: 32 lanes per column, 8 values per lane (rows t + 32 m),
// the transform stockham<256, 8> in a 273-element LDS tile per column. Lanes run along the bins
// first, so a wave touches 128 contiguous bytes of each of 8 rows. Packed bin 0 holds two real
// columns (DC, Nyquist): its lanes split the two spectra apart with the mirror bin (through LDS)
// and multiply them one by one. Fixed order q = 0, 1, ..; no atomics: equal calls give equal bits.
#include "upols_f64_handle.hpp"

namespace neo_hip {

constexpr int kOffCols = 8;                  // columns per workgroup
constexpr int kOffE = 8;                     // values of a column per lane
constexpr int kOffT = kOff64F / kOffE;       // lanes per column
constexpr int kOffLL = lds_len(kOff64F);     // one column's transform tile
static_assert(kOffCols * kOffT == 256 && kOffE == 2 * (kOff64W / kOffT), "a lane's first 4 values are a pair's older half");

__device__ __forceinline__ cd cfma(cd a, cd b, cd acc)  // acc + a b
{
    return {fma(-a.y, b.y, fma(a.x, b.x, acc.x)), fma(a.y, b.x, fma(a.x, b.y, acc.y))};
}

// Segment q of channel c, 8 bins: filter rows 128 q + k, k < 128 (zero from row P on) as the first
// half of a 256-point column, forward transform, spectrum row f of HF[c][q].
__global__ __launch_bounds__(256) void k_upols64_ohf(const cd* __restrict__ H, cd* __restrict__ HF,
                                                     const cd* __restrict__ twg, int B, int P, int nseg)
{
    __shared__ cd lds[kOffCols * kOffLL];
    __shared__ cd tw[kOff64F];
    const int tid = threadIdx.x, col = tid % kOffCols, t = tid / kOffCols;
    const int c = blockIdx.x / nseg, q = blockIdx.x - c * nseg, bin = blockIdx.y * kOffCols + col;
    tw[tid] = twg[tid];
    const cd* Hc = H + int64_t(c) * P * B + bin;
    cd v[kOffE];
#pragma unroll
    for (int m = 0; m < kOffE; ++m) {
        const int p = q * kOff64W + t + m * kOffT;
        v[m] = (m < kOffE / 2 && p < P) ? Hc[int64_t(p) * B] : cd{0.0, 0.0};
    }
    __syncthreads();  // twiddles
    stockham<kOff64F, kOffE, -1>(v, lds + col * kOffLL, tw, t, true);
    cd* o = HF + (int64_t(c) * nseg + q) * kOff64F * B + bin;
#pragma unroll
    for (int m = 0; m < kOffE; ++m) o[int64_t(t + m * kOffT) * B] = v[m];
}

// Channel c, 8 bins. Pair q is window rows -128 (q + 1) .. -128 q + 127; lane t of a column holds
// rows t + 32 m of it, so m < 4 is the older half and m >= 4 the newer one, which is pair q - 1's
// older half (pair 0: the fresh rows). Every row is loaded once; rows e <= -P are zero and are not
// loaded (upols64_offline_src). Y[j] = sample 128 + j of the inverse transform of the sum, scaled
// by 1 / 256: rows m >= 4.
__global__ __launch_bounds__(256) void k_upols64_omac(const cd* __restrict__ HF, const cd* __restrict__ fdl,
                                                      const cd* __restrict__ N, cd* __restrict__ Y,
                                                      const cd* __restrict__ twg, int B, int P, int nseg, int w)
{
    __shared__ cd lds[kOffCols * kOffLL];
    __shared__ cd tw[kOff64F];
    __shared__ cd zx[kOff64F], zh[kOff64F];  // bin 0: the pair's and the segment's spectrum, for the mirror bin
    constexpr int HALF = kOffE / 2;
    const int tid = threadIdx.x, col = tid % kOffCols, t = tid / kOffCols;
    const int c = blockIdx.x, bin = blockIdx.y * kOffCols + col;
    const bool unit0 = blockIdx.y == 0;  // uniform per workgroup: the unit holding packed bin 0
    const bool b0 = unit0 && col == 0;
    tw[tid] = twg[tid];
    cd* L = lds + col * kOffLL;
    const cd* Fc = fdl + int64_t(c) * P * B + bin;
    const cd* Nc = N + int64_t(c) * kOff64W * B + bin;
    const cd* Hc = HF + int64_t(c) * nseg * kOff64F * B + bin;
    auto row = [&](int e) {
        const upols64_offline_row r = upols64_offline_src(e, w, P);
        if (r.kind == kOff64Zero) return cd{0.0, 0.0};
        return ld_nt((r.kind == kOff64Scratch ? Nc : Fc) + int64_t(r.row) * B);
    };
    cd newer[HALF], older[HALF], acc[kOffE];
#pragma unroll
    for (int m = 0; m < HALF; ++m) {
        newer[m] = row(t + m * kOffT);
        older[m] = row(t + m * kOffT - kOff64W);
    }
#pragma unroll
    for (int m = 0; m < kOffE; ++m) acc[m] = cd{0.0, 0.0};
    __syncthreads();  // twiddles
#pragma unroll 1
    for (int q = 0; q < nseg; ++q) {
        cd h[kOffE], v[kOffE], next[HALF];
        const cd* Hq = Hc + int64_t(q) * kOff64F * B;
#pragma unroll
        for (int m = 0; m < kOffE; ++m) h[m] = ld_nt(Hq + int64_t(t + m * kOffT) * B);
#pragma unroll
        for (int m = 0; m < HALF; ++m) {
            // the older half of pair q + 1; past the last pair nothing is loaded
            next[m] = q + 1 < nseg ? row(t + m * kOffT - kOff64W * (q + 2)) : cd{0.0, 0.0};
            v[m] = older[m];
            v[m + HALF] = newer[m];
        }
        stockham<kOff64F, kOffE, -1>(v, L, tw, t, true);
        if (unit0) {
            if (b0) {
#pragma unroll
                for (int m = 0; m < kOffE; ++m) {
                    zx[t + m * kOffT] = v[m];
                    zh[t + m * kOffT] = h[m];
                }
            }
            __syncthreads();  // the next writes follow the next transform's barriers
        }
#pragma unroll
        for (int m = 0; m < kOffE; ++m) {
            if (b0) {
                // z = dc + i ny: DFT(dc) = (Z[f] + conj Z[-f]) / 2, DFT(ny) = (Z[f] - conj Z[-f]) / 2i, the
                // filter alike; Y[f] = DFT(dc) HD + i DFT(ny) HN
                const int fm = (kOff64F - (t + m * kOffT)) & (kOff64F - 1);
                const cd zm = cconj(zx[fm]), hm = cconj(zh[fm]);
                const cd ps = cmul(cadd(v[m], zm), cadd(h[m], hm)), pd = cmul(csub(v[m], zm), csub(h[m], hm));
                acc[m].x += 0.25 * (ps.x + pd.y);  // ps - i pd
                acc[m].y += 0.25 * (ps.y - pd.x);
            } else {
                acc[m] = cfma(v[m], h[m], acc[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < HALF; ++m) {
            newer[m] = older[m];
            older[m] = next[m];
        }
    }
    stockham<kOff64F, kOffE, +1>(acc, L, tw, t, true);
    constexpr double sc = 1.0 / kOff64F;
    cd* Yc = Y + int64_t(c) * kOff64W * B + bin;
#pragma unroll
    for (int m = HALF; m < kOffE; ++m) Yc[int64_t(t + (m - HALF) * kOffT) * B] = cd{acc[m].x * sc, acc[m].y * sc};
}

void offline_free64(neo_hip_upols64* h)
{
    dfree(h->ospectra);
    dfree(h->oscratch);
    dfree(h->oy);
    dfree(h->otail);
    h->ospectra = nullptr;
    h->oscratch = nullptr;
    h->oy = nullptr;
    h->otail = nullptr;
    h->oshape = upols64_offline_shape{};
    h->offline = false;
}

int launch_window64(neo_hip_upols64* h, const double* in, int64_t ld_in, double* out, int64_t ld_out, hipStream_t s)
{
    const upols64_shape& sh = h->shape;
    const int nseg = h->oshape.nseg;
    const unsigned units = unsigned(sh.B / kOffCols);
    if (h->ospectra_stale) {
        hipLaunchKernelGGL(k_upols64_ohf, dim3(unsigned(sh.C) * unsigned(nseg), units), dim3(256), 0, s, h->H, h->ospectra,
                           h->otw, sh.B, sh.P, nseg);
        NEO_HIP_LAUNCH_CHECK();
        h->ospectra_stale = false;
    }
    if (int rc = launch_bwindow64(h, in, ld_in, h->oscratch, kOff64W, s)) return rc;
    hipLaunchKernelGGL(k_upols64_omac, dim3(unsigned(sh.C), units), dim3(256), 0, s, h->ospectra, h->fdl, h->oscratch, h->oy,
                       h->otw, sh.B, sh.P, nseg, h->wpos);
    NEO_HIP_LAUNCH_CHECK();
    if (int rc = launch_bfinish64(h, h->oy, h->oscratch, h->otail, kOff64W, in, ld_in, out, ld_out, s)) return rc;
    h->wpos = (h->wpos + kOff64W) % sh.P;
    return NEO_HIP_OK;
}

}  // namespace neo_hip

using namespace neo_hip;

extern "C" {

NEO_HIP_API int neo_hip_upols64_set_offline(neo_hip_upols64* h, int enable)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (enable != 0 && enable != 1) return fail(NEO_HIP_EINVAL, "offline windows: enable must be 0 or 1");
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = setup_join64(h, false)) return rc;  // no pass in flight on the buffers that go
    if (!enable) {
        offline_free64(h);
        return NEO_HIP_OK;
    }
    h->ospectra_stale = true;
    if (h->offline) return NEO_HIP_OK;
    const upols64_offline_shape o = make_upols64_offline_shape(h->shape);
    if (uint64_t(h->shape.C) * uint64_t(o.nseg) > 0x7fffffffu) return fail(NEO_HIP_EINVAL, "offline windows: too many segments");
    const cd* tw = nullptr;
    if (int rc = shared_tw64(&tw, kOff64F)) return rc;
    cd *spectra = nullptr, *scratch = nullptr, *y = nullptr;
    double* tail = nullptr;
    if (dalloc(&spectra, size_t(o.spectra_bytes)) || dalloc(&scratch, size_t(o.scratch_bytes)) ||
        dalloc(&y, size_t(o.y_bytes)) || (o.tail_bytes && dalloc(&tail, size_t(o.tail_bytes)))) {
        dfree(spectra);
        dfree(scratch);
        dfree(y);
        dfree(tail);
        return fail(NEO_HIP_ENOMEM, "device allocation of %lld bytes failed", (long long)(o.spectra_bytes + o.extra_bytes));
    }
    h->ospectra = spectra;
    h->oscratch = scratch;
    h->oy = y;
    h->otail = tail;
    h->otw = tw;
    h->oshape = o;
    h->offline = true;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols64_offline_info(neo_hip_upols64* h, int* blocks_per_pass, int* segments,
                                             int64_t* spectra_bytes, int64_t* extra_bytes)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (blocks_per_pass) *blocks_per_pass = h->offline ? kOff64W : 0;
    if (segments) *segments = h->oshape.nseg;
    if (spectra_bytes) *spectra_bytes = h->oshape.spectra_bytes;
    if (extra_bytes) *extra_bytes = h->oshape.extra_bytes;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols64_offline_plan(int channels, int block, int partitions, int method, int* blocks_per_pass,
                                             int* segments, int64_t* spectra_bytes, int64_t* extra_bytes,
                                             int64_t* pass_bytes)
{
    upols64_shape sh;
    if (const char* why = make_upols64_shape(channels, block, partitions, method, 0, sh)) return fail(NEO_HIP_EINVAL, "%s", why);
    const upols64_offline_shape o = make_upols64_offline_shape(sh);
    if (blocks_per_pass) *blocks_per_pass = kOff64W;
    if (segments) *segments = o.nseg;
    if (spectra_bytes) *spectra_bytes = o.spectra_bytes;
    if (extra_bytes) *extra_bytes = o.extra_bytes;
    if (pass_bytes) *pass_bytes = o.pass_bytes;
    return NEO_HIP_OK;
}

}  // extern "C"
