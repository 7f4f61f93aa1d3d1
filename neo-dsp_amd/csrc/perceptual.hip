// perceptual.hip — the perceptual sparsity predicate on the device (perceptual_plan.hpp is its
// definition): the plugin's sparse_convolve threshold (extra/plugin/src/dsp/DenseConvolution.cpp:
// 110-170) on filter spectra [C][P][B+1] that are already in device memory, so that a sparse
// handle's filter is thinned without the spectra or a mask crossing PCIe.
//
//   k_perc_max   per-channel maximum of re^2 + im^2: reads the spectra once (8 B per bin)
//   k_perc_mask  one workgroup per filter row: the row's B + 1 mask bytes (8 B read, 1 B written
//                per bin); feeds sparse_set_filter unchanged
//   k_perc_hist  the level histograms at column and at tile granularity, [C][144] each
// The weight table is computed on the host in double (perceptual_weights) and uploaded; the
// kernels never evaluate the A-weighting themselves.
#include "perceptual_plan.hpp"
#include "upols_handle.hpp"

#include <algorithm>
#include <vector>

namespace neo_hip {

constexpr int kPercHistRows = 16;  // filter rows per workgroup of k_perc_hist (one flush for all)

// Workgroups g of G stride over channel c's P (B + 1) bins two at a time (float4; the channel starts
// on an 8-byte boundary, so up to one bin before and one after the 16-byte body are taken alone).
// The maximum is non-negative and never NaN (a NaN power loses every comparison), so its bit
// pattern orders like the float: one atomicMax per workgroup into maxp[c] (zeroed before).
__global__ __launch_bounds__(256) void k_perc_max(const cf* __restrict__ filter, int64_t n, int G,
                                                  unsigned* __restrict__ maxp)
{
    __shared__ float part[4];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x / G;
    const int g = int(blockIdx.x - c * G);
    const cf* f = filter + c * n;
    const int head = int((reinterpret_cast<uintptr_t>(f) >> 3) & 1);
    const int64_t pairs = (n - head) >> 1;
    const float4* v = reinterpret_cast<const float4*>(f + head);
    float m = 0.0f;
    auto take = [&](float4 q) {
        const float a = perc_power(q.x, q.y), b = perc_power(q.z, q.w);
        m = a > m ? a : m;
        m = b > m ? b : m;
    };
    const int64_t stride = int64_t(G) * 256;
    int64_t i = int64_t(g) * 256 + tid;
    for (; i + 3 * stride < pairs; i += 4 * stride) {  // four loads in flight per lane
        const float4 q0 = v[i], q1 = v[i + stride], q2 = v[i + 2 * stride], q3 = v[i + 3 * stride];
        take(q0);
        take(q1);
        take(q2);
        take(q3);
    }
    for (; i < pairs; i += stride) take(v[i]);
    if (g == 0 && tid == 0) {
        if (head) take(float4{f[0].x, f[0].y, 0.0f, 0.0f});
        if ((n - head) & 1) take(float4{f[n - 1].x, f[n - 1].y, 0.0f, 0.0f});
    }
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
        if (m > 0.0f) atomicMax(maxp + c, __float_as_uint(m));
    }
}

// One workgroup per filter row (c, p), k_sparse_rows' decomposition: lane t takes the columns
// t, t + 256, ... (coalesced 8-byte loads), the keep bytes are laid out in LDS at the row's offset
// within its first 32-bit word of the mask, and go out as whole words (up to 3 bytes at either
// end alone: a row of B + 1 bytes starts on any byte).
__global__ __launch_bounds__(256) void k_perc_mask(const cf* __restrict__ filter, int B, int P,
                                                   const float* __restrict__ maxp, const float* __restrict__ w, float thr,
                                                   uint8_t* __restrict__ mask)
{
    __shared__ uint32_t keep[(4096 + 1 + 3) / 4 + 1];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x, c = r / P;
    const cf* src = filter + r * (int64_t(B) + 1);
    uint8_t* dst = mask + r * (int64_t(B) + 1);
    const int sh = int(reinterpret_cast<uintptr_t>(dst) & 3);
    const float scale = __fdiv_rn(1.0f, maxp[c]);
    uint8_t* kb = reinterpret_cast<uint8_t*>(keep);
    for (int k = tid; k <= B; k += 256) {
        const cf v = src[k];
        kb[sh + k] = perc_level(perc_power(v.x, v.y), scale, w[k]) > thr ? 1 : 0;
    }
    __syncthreads();
    const int end = sh + B + 1;  // the row is bytes [sh, end) of the LDS image
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst - sh);
    const int w0 = sh ? 1 : 0, w1 = end >> 2;  // whole words [w0, w1); B >= 16: never empty
    for (int i = w0 + tid; i < w1; i += 256) dw[i] = keep[i];
    if (tid >= sh && tid < 4 * w0) dst[tid - sh] = kb[tid];                          // bytes [sh, 4)
    if (tid >= 64 && 4 * w1 + tid - 64 < end) dst[4 * w1 + tid - 64 - sh] = kb[4 * w1 + tid - 64];  // the tail
}

// kPercHistRows rows of one channel per workgroup. Columns as in k_perc_mask; 16 neighbouring
// lanes hold one tile (256 is a multiple of 16), whose level is their maximum (tile 0: also the
// Nyquist column's). Counts go to LDS counters, then one 64-bit atomic add per non-empty counter.
__global__ __launch_bounds__(256) void k_perc_hist(const cf* __restrict__ filter, int B, int P, int GP,
                                                   const float* __restrict__ maxp, const float* __restrict__ w,
                                                   unsigned long long* __restrict__ hist_bins,
                                                   unsigned long long* __restrict__ hist_tiles)
{
    __shared__ unsigned hb[kPercBuckets], ht[kPercBuckets];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x / GP;
    const int g = int(blockIdx.x - c * GP);
    for (int j = tid; j < kPercBuckets; j += 256) hb[j] = ht[j] = 0;
    __syncthreads();
    const float scale = __fdiv_rn(1.0f, maxp[c]);
    const float wB = w[B];
    const int p1 = min(P, (g + 1) * kPercHistRows);
    for (int p = g * kPercHistRows; p < p1; ++p) {
        const cf* src = filter + (c * P + p) * (int64_t(B) + 1);
        const cf nq = src[B];
        const float last = perc_level(perc_power(nq.x, nq.y), scale, wB);
        if (tid == 0) atomicAdd(&hb[perc_bucket(last)], 1u);
        for (int k0 = 0; k0 < B; k0 += 256) {  // uniform bounds: every lane takes part in the shuffles
            const int k = k0 + tid;
            float db = -INFINITY;
            if (k < B) {
                const cf v = src[k];
                db = perc_level(perc_power(v.x, v.y), scale, w[k]);
                atomicAdd(&hb[perc_bucket(db)], 1u);
            }
            float top = k < kPercTile ? fmaxf(last, db) : db;
            for (int o = 8; o; o >>= 1) top = fmaxf(top, __shfl_xor(top, o));
            if (k < B && (tid & (kPercTile - 1)) == 0) atomicAdd(&ht[perc_bucket(top)], 1u);
        }
    }
    __syncthreads();
    for (int j = tid; j < kPercBuckets; j += 256) {
        if (hb[j]) atomicAdd(hist_bins + c * kPercBuckets + j, (unsigned long long)hb[j]);
        if (ht[j]) atomicAdd(hist_tiles + c * kPercBuckets + j, (unsigned long long)ht[j]);
    }
}

// tmp (pooled, the caller's to free once `s` is joined) = maxp [C] then the weights [B + 1];
// weights stays the caller's until then too (it is copied asynchronously).
static int perc_levels_begin(const cf* filter, int C, int B, int P, const float* weights, float** tmp, hipStream_t s)
{
    const int64_t n = int64_t(P) * (int64_t(B) + 1);
    if (int64_t(C) * P > 0x7fffffff) return fail(NEO_HIP_EINVAL, "too many partitions");
    if (int rc = dalloc(tmp, (size_t(C) + size_t(B) + 1) * sizeof(float))) return rc;
    NEO_HIP_CHECK(hipMemsetAsync(*tmp, 0, size_t(C) * sizeof(float), s));
    NEO_HIP_CHECK(hipMemcpyAsync(*tmp + C, weights, (size_t(B) + 1) * sizeof(float), hipMemcpyHostToDevice, s));
    // about 2048 bins per lane-quad pass, up to ~4096 workgroups over all channels
    const int64_t want = (n / 2 + 256 * 8 - 1) / (256 * 8);
    const int G = int(std::max<int64_t>(1, std::min<int64_t>(want, std::max(1, 4096 / C))));
    hipLaunchKernelGGL(k_perc_max, dim3(unsigned(C) * unsigned(G)), dim3(256), 0, s, filter, n, G,
                       reinterpret_cast<unsigned*>(*tmp));
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

int perceptual_mask_device(const cf* filter, int C, int B, int P, const neo_hip_perceptual* pp, const float* weights,
                           uint8_t* mask, float** tmp, hipStream_t s)
{
    if (int rc = perc_levels_begin(filter, C, B, P, weights, tmp, s)) return rc;
    hipLaunchKernelGGL(k_perc_mask, dim3(unsigned(C) * unsigned(P)), dim3(256), 0, s, filter, B, P, *tmp, *tmp + C,
                       pp->threshold_db, mask);
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

namespace {

// the checks every entry point makes before a device is touched
int perc_args(const char* who, bool pointers, int C, int B, int P, const neo_hip_perceptual* pp)
{
    if (!pointers || !pp) return fail(NEO_HIP_EINVAL, "%s: null pointer", who);
    if (C < 1 || P < 1) return fail(NEO_HIP_EINVAL, "%s: channels and partitions must be >= 1", who);
    if (const char* why = perceptual_check(B, pp)) return fail(NEO_HIP_EINVAL, "%s: %s", who, why);
    return NEO_HIP_OK;
}

}  // namespace
}  // namespace neo_hip

using namespace neo_hip;

extern "C" {

NEO_HIP_API int neo_hip_perceptual_weights(int block, const neo_hip_perceptual* pp, float* weights)
{
    if (int rc = perc_args("perceptual_weights", weights != nullptr, 1, block, 1, pp)) return rc;
    perceptual_weights(block, pp, weights);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_perceptual_mask_host(const void* filter, int C, int B, int P, const neo_hip_perceptual* pp,
                                             uint8_t* mask)
{
    if (int rc = perc_args("perceptual_mask_host", filter && mask, C, B, P, pp)) return rc;
    std::vector<float> w(size_t(B) + 1);
    perceptual_weights(B, pp, w.data());
    perceptual_mask(static_cast<const float*>(filter), C, B, P, pp, w.data(), mask);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_perceptual_hist_host(const void* filter, int C, int B, int P, const neo_hip_perceptual* pp,
                                             int64_t* hist_bins, int64_t* hist_tiles)
{
    if (int rc = perc_args("perceptual_hist_host", filter && hist_bins && hist_tiles, C, B, P, pp)) return rc;
    std::vector<float> w(size_t(B) + 1);
    perceptual_weights(B, pp, w.data());
    perceptual_histogram(static_cast<const float*>(filter), C, B, P, pp, w.data(), hist_bins, hist_tiles);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_perceptual_mask(const void* filter, int C, int B, int P, const neo_hip_perceptual* pp,
                                        uint8_t* mask, int is_device, int device)
{
    if (int rc = perc_args("perceptual_mask", filter && mask, C, B, P, pp)) return rc;
    device_guard g(device);
    if (g.rc) return g.rc;
    hipStream_t s = nullptr;
    if (is_device)
        if (int rc = null_join()) return rc;  // after its producer (common.hpp: null_join)
    if (int rs = shared_stream(&s)) return rs;
    std::vector<float> w(size_t(B) + 1);
    perceptual_weights(B, pp, w.data());
    const size_t n = size_t(C) * size_t(P) * (size_t(B) + 1);
    const cf* src = nullptr;
    uint8_t* d_mask = mask;
    cf* tmpf = nullptr;
    uint8_t* tmpm = nullptr;
    float* tmp = nullptr;
    int rc = stage_in(static_cast<const cf*>(filter), n * sizeof(cf), is_device != 0, false, s, &tmpf, &src);
    if (!rc && !is_device) {
        if (dalloc(&tmpm, n)) rc = fail(NEO_HIP_ENOMEM, "allocation failed");
        d_mask = tmpm;
    }
    if (!rc) rc = perceptual_mask_device(src, C, B, P, pp, w.data(), d_mask, &tmp, s);
    if (!rc && !is_device && hipMemcpyAsync(mask, d_mask, n, hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(NEO_HIP_ERUNTIME, "copy back failed");
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    dfree(tmp);  // the stream was joined above
    dfree(tmpf);
    dfree(tmpm);
    return rc;
}

NEO_HIP_API int neo_hip_perceptual_histogram(const void* filter, int C, int B, int P, const neo_hip_perceptual* pp,
                                             int64_t* hist_bins, int64_t* hist_tiles, int is_device, int device)
{
    if (int rc = perc_args("perceptual_histogram", filter && hist_bins && hist_tiles, C, B, P, pp)) return rc;
    device_guard g(device);
    if (g.rc) return g.rc;
    hipStream_t s = nullptr;
    if (is_device)
        if (int rc = null_join()) return rc;  // after its producer (common.hpp: null_join)
    if (int rs = shared_stream(&s)) return rs;
    std::vector<float> w(size_t(B) + 1);
    perceptual_weights(B, pp, w.data());
    const size_t n = size_t(C) * size_t(P) * (size_t(B) + 1);
    const size_t hbytes = size_t(C) * kPercBuckets * sizeof(int64_t);
    const cf* src = nullptr;
    cf* tmpf = nullptr;
    unsigned long long* hist = nullptr;  // [2][C][144]
    float* tmp = nullptr;
    int rc = NEO_HIP_OK;
    if (dalloc(&hist, 2 * hbytes)) rc = fail(NEO_HIP_ENOMEM, "allocation failed");
    else if (hipMemsetAsync(hist, 0, 2 * hbytes, s) != hipSuccess) rc = fail(NEO_HIP_ERUNTIME, "memset failed");
    if (!rc) rc = stage_in(static_cast<const cf*>(filter), n * sizeof(cf), is_device != 0, false, s, &tmpf, &src);
    if (!rc) rc = perc_levels_begin(src, C, B, P, w.data(), &tmp, s);
    if (!rc) {
        const int GP = (P + kPercHistRows - 1) / kPercHistRows;
        if (int64_t(C) * GP > 0x7fffffff) rc = fail(NEO_HIP_EINVAL, "too many partitions");
        else {
            hipLaunchKernelGGL(k_perc_hist, dim3(unsigned(C) * unsigned(GP)), dim3(256), 0, s, src, B, P, GP, tmp, tmp + C,
                               hist, hist + size_t(C) * kPercBuckets);
            if (hipGetLastError() != hipSuccess) rc = fail(NEO_HIP_ERUNTIME, "k_perc_hist launch failed");
        }
    }
    if (!rc && (hipMemcpyAsync(hist_bins, hist, hbytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(hist_tiles, hist + size_t(C) * kPercBuckets, hbytes, hipMemcpyDeviceToHost, s) != hipSuccess))
        rc = fail(NEO_HIP_ERUNTIME, "copy back failed");
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    dfree(tmp);  // the stream was joined above
    dfree(tmpf);
    dfree(hist);
    return rc;
}

}  // extern "C"
