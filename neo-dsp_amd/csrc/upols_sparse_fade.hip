// upols_sparse_fade.hip — the fade step of a sparse UPOLS / UPOLA handle's live filter update
// (neo_hip_upols_update_filter_sparse / _perceptual / _update_impulse_perceptual, upols.hip). While
// a fade runs the handle has two sparse banks (sparse_bank, upols_handle.hpp: bitmaps, offsets,
// bases and compacted tiles), A (the filter so far) and B (the new one). The delay line holds input
// spectra only and is dense [C][R][B], so both banks' outputs are formed from the same FDL rows and
// mixed in the time domain:
//
//   k_upols_sparse_fade_step  grid C x S (the plain step's splits, upols_fade_split), the frame of
//                         k_upols_fade_step (upols_fade.hip): split 0 runs the window r2c, inserts the
//                         whole FDL row w, saves the previous block (overlap-save) and takes p = 0
//                         from LDS, with the plain step's device helpers in the plain step's order:
//                         the row and the previous block it leaves are the plain step's bit for bit.
//                         Per row p the bitmap words and the offset of BOTH banks are loaded (scalar
//                         loads where a wave lies within one row, B >= 128). A lane's tile is kept in
//                         A, in B, in both or in neither: the FDL float4 is loaded once if the tile is
//                         in A | B, each bank's filter float4 at off + popcount(bits below) if that
//                         bank keeps it. Every load goes through a buffer descriptor and a dropped
//                         tile passes kSparseDrop, which moves no data and returns zero (sparse_rows,
//                         upols_step.hpp: the form that won in DESIGN 5.7), so the loads of all rows
//                         in flight issue back to back. A wave with no tile of A | B in the rows in
//                         flight skips them with one uniform branch ahead of the loads. A bank with
//                         no tile at all (val null, a descriptor of size 0) drops every lane: the
//                         fade to or from silence.
//                         Sums in k_upols_fade_step's order: rows p = pstart + rs, + RPI, ...; the row
//                         groups folded in fixed order, bank A then bank B; slabs part [C][S][2][B].
//                         With the same splits the fade equals the dense handle's fade on the zeroed
//                         filters bit for bit, up to the sign of zero (fma(0, x, a) = a).
//                         A lane keeps at most 2 float4 columns (bitmap words) of a row at a time;
//                         wider rows (B >= 2048) are walked in chunks, as the dense fade step does.
//                         prime (at the update call, overlap-add only): no window and no insert,
//                         p = 0 from ring row w like every other row.
//   k_matrix_fade_finish  (upols_matrix_fade.hip, one "output" per channel), unchanged.
// No atomics: equal calls give equal bits.
#include "sparse_plan.hpp"
#include "upols_handle.hpp"
#include "upols_step.hpp"

namespace neo_hip {

// bitmap words (float4 columns) of a row a lane holds at a time: at most 2
template<int B>
constexpr int sfade_vpt() { return upols_cfg<B>::VPT > 2 ? 2 : upols_cfg<B>::VPT; }

// one bank as the kernel takes it
struct sfade_bank {
    const uint32_t* bits;  // [C][P][NW]
    const uint32_t* off;   // [C][P + 1]
    const int64_t* base;   // [C + 1]
    const float4* val;     // compacted tiles, 8 float4 each (null: no tile kept)
};

// Rows in flight per lane and waves per SIMD. B = 128 .. 512 (a wave lies within one row, one float4
// per lane and row): 3 rows at 8 waves, 60 VGPRs. The loop waits for the rows' scalar loads (both
// banks' words and offsets) once per trip, and that wait is what a trip costs below a quarter of the
// tiles: measured at 256 x 512 x 938, 2 rows took the time of the two banks' sparse steps
// one after the other at 4 and at 8 waves alike, 3 rows at 8 waves 0.83 of it at every point; 4 rows
// need 74 VGPRs (5 or 6 waves: 0.76 - 0.87), at 8 waves they spill 5 SGPRs; 6 and 8 rows at 4 waves
// (100, 124 VGPRs) 0.65 - 0.86. B < 128 (per-lane bitmap loads) and B >= 1024 (two words per lane at a
// time, the dense fade step's registers with two banks' bitmap arithmetic on top): 2 rows at 4 waves
// (B = 4096: 2 waves, its LDS). B = 128 and 256 (2 and 4 row groups, the fold's addresses on top):
// 3 rows at 6 waves; at 8 they spill 2 SGPRs.
template<int B>
constexpr int sfade_unroll() { return upols_cfg<B>::QT >= 64 && upols_cfg<B>::VPT == 1 ? 3 : 2; }
template<int B>
constexpr int sfade_waves() { return B >= 4096 ? 2 : B >= 1024 || B < 128 ? 4 : B == 512 ? 8 : 6; }
template<int B, bool OLA>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sfade_waves<B>(), sfade_waves<B>())))
void k_upols_sparse_fade_step(
    const float* __restrict__ in, int64_t ld_in, float* __restrict__ prev, sfade_bank bkA, sfade_bank bkB,
    cf* __restrict__ fdl, cf* __restrict__ part, const cf* __restrict__ twg, int P, int ring, int S, int rows, int w,
    int64_t cstride, int64_t pstride, int prime)
{
    using K = upols_cfg<B>;
    constexpr int NW = K::VPT, VPT = sfade_vpt<B>(), G = NW / VPT, UNROLL = sfade_unroll<B>();
    static_assert(NW == sparse_words(B), "a lane's float4 column v lies in bitmap word v");
    static_assert(G == 1 || K::RPI == 1, "chunked rows have one row group: the fold's LDS is not reused across chunks");
    __shared__ step_lds<B> L;
    cf* xnew = L.xnew;
    float4* red = L.red;
    const int tid = threadIdx.x;
    const int c = blockIdx.x / S, s = blockIdx.x - c * S;
    const int p0 = s * rows, p1 = min(P, p0 + rows);
    const int64_t crow = int64_t(c) * cstride;

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

    int rs = tid / K::QT;
    const int qb = tid - rs * K::QT;
    // a wave lies within one row group (QT >= 64): its row is wave-uniform, the row's words and offsets scalar loads
    if constexpr (K::QT >= 64) rs = __builtin_amdgcn_readfirstlane(rs);
    const int bit = qb >> 3, sub = (qb & 7) * 16;
    const uint32_t below = (1u << bit) - 1u;

    // this channel's tables, its tiles in both banks and its FDL ring, each < 2 GiB (make_upols_shape)
    const uint32_t* bitsA = bkA.bits + int64_t(c) * P * NW;
    const uint32_t* bitsB = bkB.bits + int64_t(c) * P * NW;
    const uint32_t* offA = bkA.off + int64_t(c) * (P + 1);
    const uint32_t* offB = bkB.off + int64_t(c) * (P + 1);
    const __amdgpu_buffer_rsrc_t valA = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float4*>(bkA.val ? bkA.val + bkA.base[c] * 8 : nullptr), 0, bkA.val ? int(offA[P]) * 128 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t valB = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float4*>(bkB.val ? bkB.val + bkB.base[c] * 8 : nullptr), 0, bkB.val ? int(offB[P]) * 128 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t fdlr = __builtin_amdgcn_make_buffer_rsrc(
        fdl + crow, 0, int(int64_t(ring) * pstride * int64_t(sizeof(cf))), 0x00020000);
    const int prow = int(pstride * int64_t(sizeof(cf)));

    const bool head = !prime && p0 == 0;  // p = 0 from LDS
    const int pstart = head ? 1 : p0;

    for (int g = 0; g < G; ++g) {
        const int v0 = g * VPT;            // the chunk's first bitmap word
        const int q0 = qb + v0 * K::QT;    // and the lane's first float4 column in it
        acc4 a[2][2 * VPT];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 2 * VPT; ++v) a[b][v] = {0.f, 0.f, 0.f, 0.f};
        if (head && rs == 0) {  // row 0 starts at tile 0 of the channel's values
            const float4* Xn = reinterpret_cast<const float4*>(xnew);
            uint32_t ta = 0, tb = 0;
            for (int vv = 0; vv < v0; ++vv) {
                ta += uint32_t(__builtin_popcount(bitsA[vv]));
                tb += uint32_t(__builtin_popcount(bitsB[vv]));
            }
#pragma unroll
            for (int v = 0; v < VPT; ++v) {
                const uint32_t wa = bitsA[v0 + v], wb = bitsB[v0 + v];
                const int ha = int(ta + uint32_t(__builtin_popcount(wa & below))) * 128 + sub;
                const int hb = int(tb + uint32_t(__builtin_popcount(wb & below))) * 128 + sub;
                const float4 x = Xn[q0 + v * K::QT];
                mac2(a[0][2 * v], a[0][2 * v + 1], buf_ld4<false>(valA, (wa >> bit) & 1u ? ha : kSparseDrop), x);
                mac2(a[1][2 * v], a[1][2 * v + 1], buf_ld4<false>(valB, (wb >> bit) & 1u ? hb : kSparseDrop), x);
                ta += uint32_t(__builtin_popcount(wa));
                tb += uint32_t(__builtin_popcount(wb));
            }
        }
        // rows p, p + RPI, ... of [pstart, p1): N rows in flight, the FDL value loaded once for both banks
        auto mac_rows = [&]<int N>(int p) {
            uint32_t wa[N][VPT], wb[N][VPT], oa[N], ob[N];
            uint32_t any = 0;
#pragma unroll
            for (int u = 0; u < N; ++u) {
                const int pp = p + u * K::RPI;
                oa[u] = offA[pp];
                ob[u] = offB[pp];
                for (int vv = 0; vv < v0; ++vv) {  // the row's tiles in the chunks before this one
                    oa[u] += uint32_t(__builtin_popcount(bitsA[int64_t(pp) * NW + vv]));
                    ob[u] += uint32_t(__builtin_popcount(bitsB[int64_t(pp) * NW + vv]));
                }
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    wa[u][v] = bitsA[int64_t(pp) * NW + v0 + v];
                    wb[u][v] = bitsB[int64_t(pp) * NW + v0 + v];
                    any |= (wa[u][v] | wb[u][v]) >> bit;
                }
            }
            if (__ballot(any & 1u) == 0) return;
            float4 xv[N][VPT], hv[2][N][VPT];
#pragma unroll
            for (int u = 0; u < N; ++u) {
                const int pp = p + u * K::RPI;
                const int fr = w >= pp ? w - pp : w - pp + ring;  // fdl_index.hpp:28-31 ring
                uint32_t ta = oa[u], tb = ob[u];
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    const uint32_t ba = wa[u][v], bb = wb[u][v];
                    const bool ka = (ba >> bit) & 1u, kb = (bb >> bit) & 1u;
                    const int ha = int(ta + uint32_t(__builtin_popcount(ba & below))) * 128 + sub;
                    const int hb = int(tb + uint32_t(__builtin_popcount(bb & below))) * 128 + sub;
                    const int xt = fr * prow + (q0 + v * K::QT) * 16;
                    xv[u][v] = buf_ld4<true>(fdlr, ka || kb ? xt : kSparseDrop);
                    hv[0][u][v] = buf_ld4<true>(valA, ka ? ha : kSparseDrop);
                    hv[1][u][v] = buf_ld4<true>(valB, kb ? hb : kSparseDrop);
                    ta += uint32_t(__builtin_popcount(ba));
                    tb += uint32_t(__builtin_popcount(bb));
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

int launch_sparse_fade_mac(const upols_t* h, const sparse_bank& a, const sparse_bank& b, const float* in, int64_t ld_in,
                           int S, int rows, int w, bool prime, hipStream_t s)
{
    const unsigned grid = unsigned(h->C) * unsigned(S);
    const upols_shape& sh = h->shape;
    const sfade_bank ba{a.bits, a.off, a.base, reinterpret_cast<const float4*>(a.val)};
    const sfade_bank bb{b.bits, b.off, b.base, reinterpret_cast<const float4*>(b.val)};
    NEO_UPOLS_DISPATCH_OLA(h->B, h->ola, hipLaunchKernelGGL((k_upols_sparse_fade_step<BB, OL>), dim3(grid), dim3(256), 0, s,
                                                            in, ld_in, h->prev, ba, bb, h->fdl, h->part_f, h->tw, h->P, h->ring,
                                                            S, rows, w, sh.cstride, sh.pstride, int(prime)))
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

}  // namespace neo_hip
