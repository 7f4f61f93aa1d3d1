// upols_matrix_fade.hip — the fade step of a matrix convolver's live filter update
// (neo_hip_matrix_update_filter / _update_impulse, upols_matrix.hip). While a fade runs the handle
// has two filter banks, A (the filter so far) and B (the new one), over the SAME route list. The
// delay line holds input spectra only, so both banks' outputs are formed from the same FDL rows:
//
//   k_matrix_window       (upols_matrix.hip) unchanged: every read of the caller's input
//   k_matrix_fade_step    grid O x S x G, one output per workgroup (the out_tile = 1 row list: the
//                         output's inputs ascending x partitions 0..P-1, cut into S splits at equal
//                         row counts). Per row (i, p) a lane loads the FDL row ONCE and the filter
//                         row of both banks, into two accumulator sets: the register shape of
//                         k_matrix_step's OT = 2 (pinned to 4 waves per SIMD like it). Rows wider
//                         than 512 float4 are cut into G chunks of 512 so that shape holds up to
//                         B = 4096. Every entry of an output's list is a route of it, so no load
//                         goes through an empty descriptor and an input reaches only the outputs it
//                         feeds. Slabs part [O][S][2][B].
//   k_matrix_fade_finish  grid O: per bank the slabs summed in the order s = 0..S-1 and the c2r;
//                         bank A's samples stay in registers across bank B's transform; then
//                         out = a + g (b - a) with g = matrix_fade_gain (matrix_fade.hpp), the first
//                         write of `out` (so in == out stays allowed). Overlap-add keeps a tail per
//                         bank: a and b take their own tail first, both tails are rewritten.
//                         PRIME (at the update call, overlap-add only): bank B alone at write
//                         position w - 1, no output: it leaves bank B's tail of the block before.
// No atomics: equal calls give equal bits.
#include "matrix_fade.hpp"
#include "matrix_plan.hpp"
#include "upols_handle.hpp"
#include "upols_step.hpp"

namespace neo_hip {

// float4 columns of a row per workgroup: at most 2 per lane
template<int B>
constexpr int fade_vpt() { return upols_cfg<B>::VPT > 2 ? 2 : upols_cfg<B>::VPT; }
template<int B>
constexpr int fade_unroll() { return fade_vpt<B>() >= 2 ? 2 : 3; }

template<int B>
__global__ __launch_bounds__(256, 4) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_matrix_fade_step(
    const cf* __restrict__ HA, const cf* __restrict__ HB, const cf* __restrict__ fdl, cf* __restrict__ part,
    const int* __restrict__ tab, int O, int P, int ring, int S, int w)
{
    using K = upols_cfg<B>;
    constexpr int VPT = fade_vpt<B>(), G = K::VPT / VPT, UNROLL = fade_unroll<B>();
    __shared__ __attribute__((aligned(16))) float4 red[K::RPI > 1 ? 256 * 2 * VPT : 1];
    const int tid = threadIdx.x;
    const int g = blockIdx.x % G, os = blockIdx.x / G;
    const int o = os / S, s = os - o * S;
    const int e0 = tab[o], nent = tab[o + 1] - e0;
    const int* ent = tab + O + 1 + 2 * e0;  // {input, route}, inputs ascending
    const int n = nent * P, per = (n + S - 1) / S;
    const int r0 = min(n, s * per), r1 = min(n, r0 + per);

    const int rs = tid / K::QT, q0 = tid - rs * K::QT + g * VPT * K::QT;
    acc4 a[2][2 * VPT];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int v = 0; v < 2 * VPT; ++v) a[b][v] = {0.f, 0.f, 0.f, 0.f};

    const int rowbytes = B * int(sizeof(cf));
    for (int seg = r1 > r0 ? r0 / P : nent; seg < nent && seg * P < r1; ++seg) {
        const int i = ent[2 * seg], r = ent[2 * seg + 1];
        const int pbeg = max(r0, seg * P) - seg * P, pend = min(r1, (seg + 1) * P) - seg * P;
        // a route's filter and an input's ring each span < 2 GiB (make_matrix_plan)
        const __amdgpu_buffer_rsrc_t ha =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(HA + int64_t(r) * P * B), 0, P * rowbytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t hb =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(HB + int64_t(r) * P * B), 0, P * rowbytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t fd =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(fdl + int64_t(i) * ring * B), 0, ring * rowbytes, 0x00020000);
        auto rows = [&]<int N>(int p) {
            float4 xv[N][VPT], hv[2][N][VPT];
#pragma unroll
            for (int u = 0; u < N; ++u) {
                const int pp = p + u * K::RPI;
                const int fr = w >= pp ? w - pp : w - pp + ring;
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    const int q = q0 + v * K::QT;
                    xv[u][v] = buf_ld4<false>(fd, fr * rowbytes + q * 16);
                    hv[0][u][v] = buf_ld4<true>(ha, pp * rowbytes + q * 16);
                    hv[1][u][v] = buf_ld4<true>(hb, pp * rowbytes + q * 16);
                }
            }
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int u = 0; u < N; ++u)
#pragma unroll
                    for (int v = 0; v < VPT; ++v) mac2(a[b][2 * v], a[b][2 * v + 1], hv[b][u][v], xv[u][v]);
        };
        int p = pbeg + rs;
        for (; p + (UNROLL - 1) * K::RPI < pend; p += UNROLL * K::RPI) rows.template operator()<UNROLL>(p);
        for (; p < pend; p += K::RPI) rows.template operator()<1>(p);
    }

    // fold the row groups into group 0 (fixed order), one bank at a time, and publish the slabs
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if constexpr (K::RPI > 1) {
            if (b) __syncthreads();  // the fold of bank A has read red
#pragma unroll
            for (int v = 0; v < VPT; ++v) {
                red[(tid * VPT + v) * 2 + 0] = make_float4(a[b][2 * v].rr, a[b][2 * v].ii, a[b][2 * v].ri, a[b][2 * v].ir);
                red[(tid * VPT + v) * 2 + 1] =
                    make_float4(a[b][2 * v + 1].rr, a[b][2 * v + 1].ii, a[b][2 * v + 1].ri, a[b][2 * v + 1].ir);
            }
            __syncthreads();
            if (rs == 0) {
#pragma unroll 4
                for (int gr = 1; gr < K::RPI; ++gr) {
#pragma unroll
                    for (int v = 0; v < VPT; ++v) {
                        const int idx = ((gr * K::QT + tid) * VPT + v) * 2;  // rs == 0: tid is the lane's column
                        const float4 x0 = red[idx], x1 = red[idx + 1];
                        a[b][2 * v].rr += x0.x; a[b][2 * v].ii += x0.y; a[b][2 * v].ri += x0.z; a[b][2 * v].ir += x0.w;
                        a[b][2 * v + 1].rr += x1.x; a[b][2 * v + 1].ii += x1.y; a[b][2 * v + 1].ri += x1.z; a[b][2 * v + 1].ir += x1.w;
                    }
                }
            }
        }
        float4* slab = reinterpret_cast<float4*>(part + ((int64_t(o) * S + s) * 2 + b) * B);
        if (rs == 0) {
#pragma unroll
            for (int v = 0; v < VPT; ++v) {
                const int q = q0 + v * K::QT;
                const cf b0 = finish(a[b][2 * v], q == 0), b1 = finish(a[b][2 * v + 1], false);
                slab[q] = make_float4(b0.x, b0.y, b1.x, b1.y);
            }
        }
    }
}

// the packed spectrum X (LDS) -> the 2B window samples, unscaled, in registers: lane t holds
// z[t + m T] = samples 2 (t + m T), + 1 (c2r_tail's transform without its stores)
template<int B, int E>
__device__ __forceinline__ void fade_c2r(const cf* X, cf* fft, const cf* tw, cf (&v)[E], int tid)
{
    using K = upols_cfg<B>;
    constexpr int T = B / E;
    static_assert(T <= 256 && B % E == 0, "c2r must fit one 256-lane workgroup");
    const bool active = tid < T;
    if (active) {
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int k = tid + m * T;
            const cf x0 = X[0];
            v[m] = k == 0 ? c2r_join<B>(cf{x0.x, 0.f}, cf{x0.y, 0.f}, tw + K::TW1, 0)
                          : c2r_join<B>(X[k], X[B - k], tw + K::TW1, k);
        }
    }
    stockham<B, E, +1>(v, fft, tw, tid, active);
}

template<int B, bool OLA, bool PRIME>
__global__ __launch_bounds__(256) void k_matrix_fade_finish(const cf* __restrict__ part, float* __restrict__ out,
                                                            int64_t ld_out, float* __restrict__ ovl_a,
                                                            float* __restrict__ ovl_b, const cf* __restrict__ twg, int S,
                                                            int64_t n0, int64_t total, int curve)
{
    using K = upols_cfg<B>;
    constexpr int E = NEO_FINISH_E(B), T = B / E;
    __shared__ __attribute__((aligned(16))) cf X[B];
    __shared__ cf fft[K::LL];
    __shared__ cf tw[K::TW1 + K::TW2];
    const int tid = threadIdx.x, o = blockIdx.x;
    for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];
    // bank `b` of the output's slabs [S][2][B] summed in the order s = 0..S-1 into X
    auto sum_bank = [&](int b) {
        const float4* p4 = reinterpret_cast<const float4*>(part + (int64_t(o) * S * 2 + b) * B);
        for (int q = tid; q < K::Q; q += 256) {
            float4 sum = p4[q];
            int t = 1;
            for (; t + 3 < S; t += 4) {
                float4 r[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = p4[int64_t(t + u) * 2 * K::Q + q];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    sum.x += r[u].x; sum.y += r[u].y; sum.z += r[u].z; sum.w += r[u].w;
                }
            }
            for (; t < S; ++t) {
                const float4 r = p4[int64_t(t) * 2 * K::Q + q];
                sum.x += r.x; sum.y += r.y; sum.z += r.z; sum.w += r.w;
            }
            reinterpret_cast<float4*>(X)[q] = sum;
        }
        __syncthreads();
    };
    const float scale = 1.0f / float(2 * B);
    const bool active = tid < T;
    cf* ob = reinterpret_cast<cf*>(ovl_b + int64_t(o) * B);
    if constexpr (PRIME) {
        cf vb[E];
        sum_bank(1);
        fade_c2r<B, E>(X, fft, tw, vb, tid);
        if (active) {
#pragma unroll
            for (int m = E / 2; m < E; ++m) ob[tid + m * T - B / 2] = {vb[m].x * scale, vb[m].y * scale};
        }
        return;
    }
    cf va[E], vb[E];
    sum_bank(0);
    fade_c2r<B, E>(X, fft, tw, va, tid);
    __syncthreads();  // bank A's reads of X and fft done before bank B's sum overwrites them
    sum_bank(1);
    fade_c2r<B, E>(X, fft, tw, vb, tid);
    if (!active) return;
    cf* oc = reinterpret_cast<cf*>(out + int64_t(o) * ld_out);
    // the mix is out = a + g (b - a): g = 0 gives a exactly
    auto mix = [&](cf x, cf y, int n) {  // n: the pair's index in the block, samples 2 n and 2 n + 1
        const float g0 = matrix_fade_gain(n0 + 2 * n, total, curve), g1 = matrix_fade_gain(n0 + 2 * n + 1, total, curve);
        return cf{x.x + g0 * (y.x - x.x), x.y + g1 * (y.y - x.y)};
    };
    if constexpr (OLA) {
        cf* oa = reinterpret_cast<cf*>(ovl_a + int64_t(o) * B);
        // the same lane reads a tail's pair n (m < E / 2) before it writes it (m >= E / 2: n - B / 2)
#pragma unroll
        for (int m = 0; m < E / 2; ++m) {
            const int n = tid + m * T;
            const cf ta = oa[n], tb = ob[n];
            oc[n] = mix(cf{va[m].x * scale + ta.x, va[m].y * scale + ta.y}, cf{vb[m].x * scale + tb.x, vb[m].y * scale + tb.y}, n);
        }
#pragma unroll
        for (int m = E / 2; m < E; ++m) {
            const int n = tid + m * T - B / 2;
            oa[n] = {va[m].x * scale, va[m].y * scale};
            ob[n] = {vb[m].x * scale, vb[m].y * scale};
        }
    } else {
#pragma unroll
        for (int m = E / 2; m < E; ++m) {  // window samples [B, 2B)
            const int n = tid + m * T - B / 2;
            oc[n] = mix(cf{va[m].x * scale, va[m].y * scale}, cf{vb[m].x * scale, vb[m].y * scale}, n);
        }
    }
}

int matrix_fade_chunks(int B) { return B > 1024 ? B / 1024 : 1; }

int launch_matrix_fade_mac(const cf* HA, const cf* HB, const cf* fdl, cf* part, const int* tab, int B, int P, int ring,
                           int O, int S, int w, hipStream_t s)
{
    const unsigned grid = unsigned(O) * unsigned(S) * unsigned(matrix_fade_chunks(B));
    NEO_UPOLS_DISPATCH(B, {
        static_assert(upols_cfg<BB>::VPT / fade_vpt<BB>() == (BB > 1024 ? BB / 1024 : 1), "chunks per row");
        hipLaunchKernelGGL((k_matrix_fade_step<BB>), dim3(grid), dim3(256), 0, s, HA, HB, fdl, part, tab, O, P, ring, S, w);
    })
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

int launch_matrix_fade_finish(const cf* part, float* out, int64_t ld_out, float* ovl_a, float* ovl_b, const cf* tw, int B,
                              int O, int S, bool ola, bool prime, int64_t n0, int64_t total, int curve, hipStream_t s)
{
#define NEO_FADE_FINISH(OL, PR)                                                                                          \
    NEO_UPOLS_DISPATCH(B, hipLaunchKernelGGL((k_matrix_fade_finish<BB, OL, PR>), dim3(unsigned(O)), dim3(256), 0, s, part, \
                                             out, ld_out, ovl_a, ovl_b, tw, S, n0, total, curve))
    if (prime) NEO_FADE_FINISH(true, true)
    else if (ola) NEO_FADE_FINISH(true, false)
    else NEO_FADE_FINISH(false, false)
#undef NEO_FADE_FINISH
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

}  // namespace neo_hip

using namespace neo_hip;

extern "C" {

NEO_HIP_API int neo_hip_matrix_fade_gains(int block, int fade_blocks, int curve, float* g)
{
    if (block < 16 || block > 4096 || (block & (block - 1)))
        return fail(NEO_HIP_EINVAL, "matrix_fade_gains: block must be a power of two in [16, 4096]");
    if (fade_blocks < 1 || fade_blocks > kMatrixFadeMaxBlocks)
        return fail(NEO_HIP_EINVAL, "matrix_fade_gains: fade_blocks must be in [1, %d]", kMatrixFadeMaxBlocks);
    if (curve < 0 || curve >= kMatrixFadeCurves)
        return fail(NEO_HIP_EINVAL, "matrix_fade_gains: curve must be 0 (linear) or 1 (raised cosine)");
    if (!g) return fail(NEO_HIP_EINVAL, "matrix_fade_gains: null output");
    const int64_t total = int64_t(fade_blocks) * block;
    for (int64_t n = 0; n < total; ++n) g[n] = matrix_fade_gain(n, total, curve);
    return NEO_HIP_OK;
}

}  // extern "C"
