// upols_fade.hip — the fade step of a dense UPOLS / UPOLA handle's live filter update
// (neo_hip_upols_update_filter / _update_impulse, upols.hip). While a fade runs the handle has two
// filter banks of its own layout [C][ring][B], A (the filter so far, h->H) and B (the new one,
// h->H2). The delay line holds input spectra only, so both banks' outputs are formed from the same
// FDL rows and mixed in the time domain:
//
//   k_upols_fade_step     grid C x S (the plain step's splits, upols_fade_split in upols_plan.hpp).
//                         Split 0 runs the window r2c, inserts FDL row w, saves the previous block
//                         (overlap-save) and takes p = 0 from LDS, with the plain step's device
//                         helpers in the plain step's order (upols_step_wg, upols_step.hpp): the row
//                         and the previous block it leaves are the plain step's bit for bit. Per row
//                         (p, ring row (w - p) mod R) a lane loads the FDL value ONCE and the filter
//                         value of both banks, into two accumulator sets: 24 bytes per bin and
//                         partition where two plain passes move 32. A lane keeps at most 2 float4
//                         columns of a row at a time (rows wider than 512 float4 are walked in chunks
//                         of 512, one after the other in the same workgroup), which holds the kernel
//                         to 4 waves per SIMD up to B = 4096. Slabs part [C][S][2][B].
//                         prime (at the update call, overlap-add only): no window and no insert,
//                         p = 0 from ring row w like every other row.
//   k_matrix_fade_finish  (upols_matrix_fade.hip, one "output" per channel) both banks' slabs summed
//                         in the order s = 0..S-1, two c2r, out = a + g (b - a).
// No atomics: equal calls give equal bits.
#include "upols_handle.hpp"
#include "upols_step.hpp"

namespace neo_hip {

// float4 columns of a row a lane holds at a time: at most 2
template<int B>
constexpr int ufade_vpt() { return upols_cfg<B>::VPT > 2 ? 2 : upols_cfg<B>::VPT; }
template<int B>
constexpr int ufade_unroll() { return ufade_vpt<B>() >= 2 ? 2 : 3; }

// 4 waves per SIMD, at most 128 VGPRs (B = 4096: split 0's LDS leaves room for 2 workgroups per CU,
// so the pin there is the register count alone)
template<int B, bool OLA>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(B >= 4096 ? 2 : 4, B >= 4096 ? 2 : 4), amdgpu_num_vgpr(128)))
void k_upols_fade_step(
    const float* __restrict__ in, int64_t ld_in, float* __restrict__ prev, const cf* __restrict__ HA,
    const cf* __restrict__ HB, cf* __restrict__ fdl, cf* __restrict__ part, const cf* __restrict__ twg, int P, int ring,
    int S, int rows, int w, int64_t cstride, int64_t pstride, int prime)
{
    using K = upols_cfg<B>;
    constexpr int VPT = ufade_vpt<B>(), G = K::VPT / VPT, UNROLL = ufade_unroll<B>();
    static_assert(G == 1 || K::RPI == 1, "chunked rows have one row group: the fold's LDS is not reused across chunks");
    __shared__ step_lds<B> L;
    cf* xnew = L.xnew;
    float4* red = L.red;
    const int tid = threadIdx.x;
    const int c = blockIdx.x / S, s = blockIdx.x - c * S;
    const int p0 = s * rows, p1 = min(P, p0 + rows);
    const int64_t crow = int64_t(c) * cstride;  // channel base in both banks and the FDL; row p at + p * pstride
    const int64_t ps4 = pstride / 2;            // row stride in float4 units

    if (!prime && s == 0) {  // the plain step's split 0 (upols_step_wg), statement for statement
        const float* in_c = in + int64_t(c) * ld_in;
        float* prev_c = prev + int64_t(c) * B;
        window_fft<B, OLA, (B / 8 <= 256 ? 8 : B / 256), false>(prev_c, in_c, L.fft, L.tw, tid, twg);
        cf* row = fdl + crow + int64_t(w) * pstride;
        for (int k = tid; k < B; k += 256) {
            const cf x = r2c_split<B>(L.fft, L.tw + K::TW1, k);
            xnew[k] = x;
            row[k] = x;
        }
        if constexpr (!OLA) {  // the window's second half becomes the next call's first half
            for (int i = tid; i < B / 4; i += 256)
                reinterpret_cast<float4*>(prev_c)[i] = reinterpret_cast<const float4*>(in_c)[i];
        }
        __syncthreads();
    }

    const int rs = tid / K::QT, qb = tid - rs * K::QT;
    const float4* A4 = reinterpret_cast<const float4*>(HA + crow);
    const float4* B4 = reinterpret_cast<const float4*>(HB + crow);
    const float4* F4 = reinterpret_cast<const float4*>(fdl + crow);
    const bool head = !prime && p0 == 0;  // p = 0 from LDS
    const int pstart = head ? 1 : p0;

    for (int g = 0; g < G; ++g) {
        const int q0 = qb + g * VPT * K::QT;
        acc4 a[2][2 * VPT];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 2 * VPT; ++v) a[b][v] = {0.f, 0.f, 0.f, 0.f};
        if (head && rs == 0) {
            const float4* Xn = reinterpret_cast<const float4*>(xnew);
#pragma unroll
            for (int v = 0; v < VPT; ++v) {
                const int q = q0 + v * K::QT;
                const float4 x = Xn[q];
                mac2(a[0][2 * v], a[0][2 * v + 1], A4[q], x);
                mac2(a[1][2 * v], a[1][2 * v + 1], B4[q], x);
            }
        }
        // rows p, p + RPI, ... of [pstart, p1): N row groups in flight, the FDL value loaded once for both banks
        auto mac_rows = [&]<int N>(int p) {
            float4 xv[N][VPT], hv[2][N][VPT];
#pragma unroll
            for (int u = 0; u < N; ++u) {
                const int pp = p + u * K::RPI;
                const int fr = w >= pp ? w - pp : w - pp + ring;  // fdl_index.hpp:28-31 ring
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    const int q = q0 + v * K::QT;
                    xv[u][v] = ld4_nt(F4 + int64_t(fr) * ps4 + q);
                    hv[0][u][v] = ld4_nt(A4 + int64_t(pp) * ps4 + q);
                    hv[1][u][v] = ld4_nt(B4 + int64_t(pp) * ps4 + q);
                }
            }
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int u = 0; u < N; ++u)
#pragma unroll
                    for (int v = 0; v < VPT; ++v) mac2(a[b][2 * v], a[b][2 * v + 1], hv[b][u][v], xv[u][v]);
        };
        int p = pstart + rs;
        for (; p + (UNROLL - 1) * K::RPI < p1; p += UNROLL * K::RPI) mac_rows.template operator()<UNROLL>(p);
        for (; p < p1; p += K::RPI) mac_rows.template operator()<1>(p);

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
                            const int idx = ((gr * K::QT + qb) * VPT + v) * 2;
                            const float4 x0 = red[idx], x1 = red[idx + 1];
                            a[b][2 * v].rr += x0.x; a[b][2 * v].ii += x0.y; a[b][2 * v].ri += x0.z; a[b][2 * v].ir += x0.w;
                            a[b][2 * v + 1].rr += x1.x; a[b][2 * v + 1].ii += x1.y; a[b][2 * v + 1].ri += x1.z; a[b][2 * v + 1].ir += x1.w;
                        }
                    }
                }
            }
            float4* slab = reinterpret_cast<float4*>(part + ((int64_t(c) * S + s) * 2 + b) * B);
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
}

int launch_upols_fade_mac(const upols_t* h, const cf* HA, const cf* HB, const float* in, int64_t ld_in, int S, int rows, int w,
                          bool prime, hipStream_t s)
{
    const unsigned grid = unsigned(h->C) * unsigned(S);
    const upols_shape& sh = h->shape;
    NEO_UPOLS_DISPATCH_OLA(h->B, h->ola, hipLaunchKernelGGL((k_upols_fade_step<BB, OL>), dim3(grid), dim3(256), 0, s, in, ld_in,
                                                            h->prev, HA, HB, h->fdl, h->part_f, h->tw, h->P, h->ring, S, rows,
                                                            w, sh.cstride, sh.pstride, int(prime)))
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

}  // namespace neo_hip
