// upols_step.hpp — the block step of one workgroup (c, s), shared by the dense plain step
// (upols.hip: k_upols_step, k_plain_persist) and the sparse step (upols_sparse.hip:
// k_upols_sparse_step), which differ in the loop over the partitions only.
#pragma once

#include "upols_device.hpp"

#include <type_traits>

namespace neo_hip {

// One whole block step for every channel (grid C x S, 256 lanes). Workgroup (c, s)
// accumulates partitions [p0, p1) into a partial spectrum; split 0 first runs the
// window r2c and inserts FDL row w. Each workgroup publishes its slab, and the last
// of a channel's S workgroups to arrive (agent-scope release -> counter -> acquire,
// cdna_hip_programming.md §6 G16 / split-K seam) sums the slabs in the fixed order
// s = 0..S-1 and runs the c2r: one launch per block, deterministic results.
// TAIL (upola_convolver_v2 sub-block pieces): no window / insert, partitions p >= 1 only
// (overlap_add_convolver.hpp:96-108), slabs summed by k_upola2_piece.
// latency-mode probe builds (NEO_PS_PROBE): thread 0 stamps point i of the plain step into mk
#ifdef NEO_PS_PROBE
#define NEO_STEP_MARK(i)                                    \
    do {                                                    \
        if (mk && threadIdx.x == 0) mk[i] = wall_clock64(); \
    } while (0)
#else
#define NEO_STEP_MARK(i) \
    do {                 \
    } while (0)
#endif

// the LDS of one step workgroup (k_upols_step, k_plain_persist)
template<int B>
struct step_lds {
    using K = upols_cfg<B>;
    __attribute__((aligned(16))) cf xnew[B];  // new spectrum; later the summed spectrum
    cf fft[K::LL];
    cf tw[K::TW1 + K::TW2];
    __attribute__((aligned(16))) float4 red[K::RPI > 1 ? 256 * 2 * K::VPT : 1];
    int last;
};

// Which filter rows the step's loop over the partitions reads. dense_rows: every column of every
// row, from H [C][R][B]. sparse_rows (upols_sparse.hip, sparse_plan.hpp): the kept 128-B tiles of
// channel c alone, compacted in row order -- per row NW = VPT bitmap words and a tile offset; a
// lane's float4 column q = q0 + v QT belongs to tile q / 8 = bit q0 / 8 of word v. The tiles and
// the channel's FDL ring are read through buffer descriptors (each spans < 2 GiB, checked when
// the handle is made): a lane whose tile is dropped gives an offset past the descriptor's size,
// which moves no data and returns zero, so the row loop has no branch around a load and the
// loads of all its rows in flight issue back to back (a branch per tile made the compiler wait
// for the earlier rows' loads at every join). Its accumulators then take fma(0, 0, a) = a: the
// dense sum with the dropped terms left out.
struct dense_rows {};
struct sparse_rows {
    const uint32_t* bits;  // [P][NW] of this channel
    const uint32_t* off;   // [P + 1] of this channel, tile units
    __amdgpu_buffer_rsrc_t val;  // this channel's compacted tiles, 128 B each
    __amdgpu_buffer_rsrc_t fdl;  // this channel's FDL ring
    int prow;                    // FDL row stride in bytes
};
constexpr int kSparseDrop = 0x7ffffff0;  // past any descriptor's size

template<bool NTH>
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t r, int voff)
{
    typedef unsigned u4v __attribute__((vector_size(16)));  // the builtin's own type
    const u4v u = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, NTH ? 2 : 0);
    return __builtin_bit_cast(float4, u);
}

// sparse_rows: rows pbeg + rs, + RPI, ... below pend into the lane's accumulators, UNROLL rows in
// flight. Per row: the bitmap words and the offset (scalar loads where rs is wave-uniform), then
// per float4 the filter load at tile offset + popcount(bits below the lane's tile) and the FDL
// load at the ring row (w - p) mod R, both past the end for a dropped tile. A wave none of whose
// lanes keeps a tile in any of the UNROLL rows skips them with one uniform branch, taken before
// any of their loads is issued.
template<int B, int UNROLL, bool NTH>
__device__ __forceinline__ void sparse_mac_rows(const sparse_rows& sp, int w, int ring, int rs, int q0, int pbeg,
                                                int pend, acc4 (&a)[2 * upols_cfg<B>::VPT])
{
    using K = upols_cfg<B>;
    const int bit = q0 >> 3, sub = (q0 & 7) * 16;
    const uint32_t below = (1u << bit) - 1u;
    auto rows = [&]<int N>(int p) {
        uint32_t wd[N][K::VPT], o[N];
        uint32_t any = 0;
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const int pp = p + u * K::RPI;
            o[u] = sp.off[pp];
#pragma unroll
            for (int v = 0; v < K::VPT; ++v) {
                wd[u][v] = sp.bits[int64_t(pp) * K::VPT + v];
                any |= wd[u][v] >> bit;
            }
        }
        if (__ballot(any & 1u) == 0) return;
        float4 hv[N][K::VPT], xv[N][K::VPT];
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const int pp = p + u * K::RPI;
            const int fr = w >= pp ? w - pp : w - pp + ring;  // fdl_index.hpp:28-31 ring
            uint32_t t = o[u];
#pragma unroll
            for (int v = 0; v < K::VPT; ++v) {
                const uint32_t b = wd[u][v];
                const bool keep = (b >> bit) & 1u;
                const int ht = int(t + uint32_t(__builtin_popcount(b & below))) * 128 + sub;
                const int xt = fr * sp.prow + (q0 + v * K::QT) * 16;
                hv[u][v] = buf_ld4<NTH>(sp.val, keep ? ht : kSparseDrop);
                xv[u][v] = buf_ld4<true>(sp.fdl, keep ? xt : kSparseDrop);
                t += uint32_t(__builtin_popcount(b));
            }
        }
#pragma unroll
        for (int u = 0; u < N; ++u)
#pragma unroll
            for (int v = 0; v < K::VPT; ++v) mac2(a[2 * v], a[2 * v + 1], hv[u][v], xv[u][v]);
    };
    int p = pbeg + rs;
    for (; p + (UNROLL - 1) * K::RPI < pend; p += UNROLL * K::RPI) rows.template operator()<UNROLL>(p);
    for (; p < pend; p += K::RPI) rows.template operator()<1>(p);
}

// The step of workgroup (c, s): returns true in the workgroup that ran the channel's tail (FUSED:
// the last split to arrive). WT (the latency mode's persistent plain step): the input block read
// at system scope and the output stored write-through.
template<int B, bool FUSED, bool OLA, bool TAIL, int UNROLL, bool WT = false, class SP = dense_rows>
__device__ __forceinline__ bool upols_step_wg(step_lds<B>& L, int c, int s,
    const float* __restrict__ in, int64_t ld_in, float* __restrict__ out, int64_t ld_out, float* __restrict__ prev,
    const cf* __restrict__ H, cf* __restrict__ fdl, cf* __restrict__ part, int* __restrict__ arrivals,
    const cf* __restrict__ twg, int P, int ring, int S, int rows, int w, int64_t cstride, int64_t pstride, int pc,
    unsigned long long* mk = nullptr, SP sp = {})
{
    (void)mk;
    (void)sp;
    using K = upols_cfg<B>;
    constexpr bool SPARSE = std::is_same_v<SP, sparse_rows>;
    static_assert(!SPARSE || !(TAIL || WT), "the sparse step takes whole blocks, no latency mode");
    static_assert(!(TAIL && FUSED), "the v2 tail is summed by k_upola2_piece");
    cf* xnew = L.xnew;
    cf* fft = L.fft;
    cf* tw = L.tw;
    float4* red = L.red;
    int& last = L.last;

    const int tid = threadIdx.x;
    const int p0 = s * rows, p1 = min(P, p0 + rows);
    const int64_t crow = int64_t(c) * cstride;  // channel base in H / FDL (complex units); row p at + p * pstride
    const int64_t ps4 = pstride / 2;            // row stride in float4 units

    if (!TAIL && s == 0) {
        const float* in_c = in + int64_t(c) * ld_in;
        float* prev_c = prev + int64_t(c) * B;
        window_fft<B, OLA, (B / 8 <= 256 ? 8 : B / 256), WT>(prev_c, in_c, fft, tw, tid, twg);
        NEO_STEP_MARK(1);
        cf* row = fdl + crow + int64_t(w) * pstride;
        for (int k = tid; k < B; k += 256) {
            const cf x = r2c_split<B>(fft, tw + K::TW1, k);
            xnew[k] = x;
            row[k] = x;
        }
        if constexpr (!OLA && !WT) {  // the window's second half becomes the next call's first half (WT: window_fft)
            for (int i = tid; i < B / 4; i += 256)
                reinterpret_cast<float4*>(prev_c)[i] = reinterpret_cast<const float4*>(in_c)[i];
        }
        __syncthreads();
    }

    int rs = tid / K::QT;
    const int q0 = tid - rs * K::QT;
    // sparse: a wave lies within one row group (QT >= 64), so its row is wave-uniform and the
    // row's bitmap words and offset are scalar loads
    if constexpr (SPARSE && K::QT >= 64) rs = __builtin_amdgcn_readfirstlane(rs);
    acc4 a[2 * K::VPT];
#pragma unroll
    for (int v = 0; v < 2 * K::VPT; ++v) a[v] = {0.f, 0.f, 0.f, 0.f};

    const float4* H4 = reinterpret_cast<const float4*>(H + crow);
    const float4* F4 = reinterpret_cast<const float4*>(fdl + crow);
    int pstart = p0;
    if (TAIL && p0 == 0) pstart = 1;
    if (!TAIL && p0 == 0) {
        if (rs == 0) {
            const float4* Xn = reinterpret_cast<const float4*>(xnew);
            if constexpr (SPARSE) {  // row 0 starts at tile 0 of the channel's values
#pragma unroll
                for (int v = 0, t = 0; v < K::VPT; ++v) {
                    const uint32_t b = sp.bits[v];
                    const int bit = q0 >> 3;
                    const int ht = (t + __builtin_popcount(b & ((1u << bit) - 1u))) * 128 + (q0 & 7) * 16;
                    mac2(a[2 * v], a[2 * v + 1], buf_ld4<false>(sp.val, (b >> bit) & 1u ? ht : kSparseDrop),
                         Xn[q0 + v * K::QT]);
                    t += __builtin_popcount(b);
                }
            } else {
#pragma unroll
                for (int v = 0; v < K::VPT; ++v) {
                    const int q = q0 + v * K::QT;
                    mac2(a[2 * v], a[2 * v + 1], H4[q], Xn[q]);
                }
            }
        }
        pstart = 1;
    }
    // main loop over [pbeg, pend): UNROLL row-groups in flight, no bounds checks inside.
    // Filter rows below `pc` use the default (cacheable) policy so they can stay resident
    // in the 256 MiB Infinity Cache across steps; everything else streams nontemporally.
    auto mac_rows = [&]<bool NTH>(int pbeg, int pend) {
        if constexpr (SPARSE) {
            sparse_mac_rows<B, UNROLL, NTH>(sp, w, ring, rs, q0, pbeg, pend, a);
            return;
        }
        int p = pbeg + rs;
        for (; p + (UNROLL - 1) * K::RPI < pend; p += UNROLL * K::RPI) {
            float4 hv[UNROLL][K::VPT], xv[UNROLL][K::VPT];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int pp = p + u * K::RPI;
                const int fr = w >= pp ? w - pp : w - pp + ring;  // fdl_index.hpp:28-31 ring
#pragma unroll
                for (int v = 0; v < K::VPT; ++v) {
                    const int q = q0 + v * K::QT;
                    hv[u][v] = ld4<NTH>(H4 + int64_t(pp) * ps4 + q);
                    xv[u][v] = ld4_nt(F4 + int64_t(fr) * ps4 + q);
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                for (int v = 0; v < K::VPT; ++v) mac2(a[2 * v], a[2 * v + 1], hv[u][v], xv[u][v]);
        }
        for (; p < pend; p += K::RPI) {
            const int fr = w >= p ? w - p : w - p + ring;
#pragma unroll
            for (int v = 0; v < K::VPT; ++v) {
                const int q = q0 + v * K::QT;
                mac2(a[2 * v], a[2 * v + 1], ld4<NTH>(H4 + int64_t(p) * ps4 + q), ld4_nt(F4 + int64_t(fr) * ps4 + q));
            }
        }
    };
    const int pmid = min(p1, max(pstart, pc));
    if (pmid > pstart) mac_rows.template operator()<false>(pstart, pmid);
    if (p1 > pmid) mac_rows.template operator()<true>(pmid, p1);
    if (s < 2) NEO_STEP_MARK(2 + s);  // MAC loop issued (its loads land at the first use below)

    if constexpr (K::RPI > 1) {
        // fold the row groups into group 0 (fixed order -> deterministic)
#pragma unroll
        for (int v = 0; v < K::VPT; ++v) {
            red[(tid * K::VPT + v) * 2 + 0] = make_float4(a[2 * v].rr, a[2 * v].ii, a[2 * v].ri, a[2 * v].ir);
            red[(tid * K::VPT + v) * 2 + 1] =
                make_float4(a[2 * v + 1].rr, a[2 * v + 1].ii, a[2 * v + 1].ri, a[2 * v + 1].ir);
        }
        __syncthreads();
        if (rs == 0) {
            for (int g = 1; g < K::RPI; ++g) {
#pragma unroll
                for (int v = 0; v < K::VPT; ++v) {
                    const int idx = ((g * K::QT + q0) * K::VPT + v) * 2;
                    const float4 r0 = red[idx], r1 = red[idx + 1];
                    a[2 * v].rr += r0.x; a[2 * v].ii += r0.y; a[2 * v].ri += r0.z; a[2 * v].ir += r0.w;
                    a[2 * v + 1].rr += r1.x; a[2 * v + 1].ii += r1.y; a[2 * v + 1].ri += r1.z; a[2 * v + 1].ir += r1.w;
                }
            }
        }
    }
    float* out_c = out + int64_t(c) * ld_out;

    if (FUSED && S == 1) {  // whole channel in this workgroup: finish straight from registers
        __syncthreads();  // xnew reads (p = 0) done before it is overwritten
        if (rs == 0) {
#pragma unroll
            for (int v = 0; v < K::VPT; ++v) {
                const int q = q0 + v * K::QT;
                const cf b0 = finish(a[2 * v], q == 0), b1 = finish(a[2 * v + 1], false);
                reinterpret_cast<float4*>(xnew)[q] = make_float4(b0.x, b0.y, b1.x, b1.y);
            }
        }
        __syncthreads();
        c2r_tail<B, OLA, (B / 4 <= 256 ? 4 : B / 256), false, false, WT>(xnew, fft, tw, out_c, prev + int64_t(c) * B, tid);
        return true;
    }

    // publish this split's slab
    float4* slab = reinterpret_cast<float4*>(part + (int64_t(c) * S + s) * B);
    if (rs == 0) {
#pragma unroll
        for (int v = 0; v < K::VPT; ++v) {
            const int q = q0 + v * K::QT;
            const cf b0 = finish(a[2 * v], q == 0), b1 = finish(a[2 * v + 1], false);
            slab[q] = make_float4(b0.x, b0.y, b1.x, b1.y);
        }
    }
    if constexpr (!FUSED) return false;  // k_upols_finish sums the slabs in the next launch
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its stores
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // keep the release's wait (G16 pitfall)
        const int before = __hip_atomic_fetch_add(arrivals + c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = before == S - 1;
    }
    __syncthreads();
    if (!last) return false;  // uniform per workgroup
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(arrivals + c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next step
    }
    NEO_STEP_MARK(4);  // the tail: every split arrived
    if (s != 0)
        for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];
    __syncthreads();

    // sum the S slabs in order s = 0..S-1, 8 loads in flight
    const float4* p4 = reinterpret_cast<const float4*>(part + int64_t(c) * S * B);
    if constexpr (K::Q > 256) {
        // B >= 1024: QI float4 per lane and slab; every lane's loads of SB slabs in flight at once
        // (one trip to memory per SB slabs instead of one per float4: the latency-bound one-channel
        // step at B = 4096), the same order per bin
        constexpr int QI = K::Q / 256, SB = QI >= 8 ? 2 : 16 / QI;
        float4 sum[QI];
#pragma unroll
        for (int i = 0; i < QI; ++i) sum[i] = p4[tid + i * 256];
        int t = 1;
        for (; t + SB - 1 < S; t += SB) {
            float4 r[SB][QI];
#pragma unroll
            for (int u = 0; u < SB; ++u)
#pragma unroll
                for (int i = 0; i < QI; ++i) r[u][i] = p4[int64_t(t + u) * K::Q + tid + i * 256];
#pragma unroll
            for (int u = 0; u < SB; ++u)
#pragma unroll
                for (int i = 0; i < QI; ++i) {
                    sum[i].x += r[u][i].x; sum[i].y += r[u][i].y; sum[i].z += r[u][i].z; sum[i].w += r[u][i].w;
                }
        }
        for (; t < S; ++t) {
            float4 r[QI];
#pragma unroll
            for (int i = 0; i < QI; ++i) r[i] = p4[int64_t(t) * K::Q + tid + i * 256];
#pragma unroll
            for (int i = 0; i < QI; ++i) {
                sum[i].x += r[i].x; sum[i].y += r[i].y; sum[i].z += r[i].z; sum[i].w += r[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < QI; ++i) reinterpret_cast<float4*>(xnew)[tid + i * 256] = sum[i];
    } else
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
        reinterpret_cast<float4*>(xnew)[q] = sum;
    }
    __syncthreads();
    NEO_STEP_MARK(5);  // slabs summed
    c2r_tail<B, OLA, (B / 4 <= 256 ? 4 : B / 256), false, false, WT>(xnew, fft, tw, out_c, prev + int64_t(c) * B, tid);
    NEO_STEP_MARK(6);  // output stores issued
    return true;
}

}  // namespace neo_hip
