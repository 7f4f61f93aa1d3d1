// upols_sparse_batch.hip — the MAC of a batched pass of a sparse handle: T consecutive blocks of
// every channel share ONE pass over the kept filter tiles and over the FDL tiles those rows meet.
//
// The scheme is k_batch_mac's (upols_batch.hip): a lane owns one packed bin, a workgroup walks the
// partitions of its split in order with a sliding window of T FDL rows and T complex accumulators
// per bin in registers, and writes T partial spectra to part_b[c][s][j][B]. k_batch_window,
// k_batch_finish and k_batch_ola around it are the dense pass's, unchanged.
//
// What differs:
//   filter   row p comes from the channel's compacted tiles (sparse_plan.hpp) at off[c][p] +
//            popcount(bits below the lane's tile), through the channel's buffer descriptor; a lane
//            whose tile is dropped passes kSparseDrop, an offset past the descriptor, which moves
//            no data and returns zero (upols_step.hpp).
//   FDL      the row that enters the window at partition p is multiplied by the filter rows
//            p .. p + T - 1, so its tile is fetched only where the window bitmap win[c][p] (the OR
//            of those rows' bitmaps, made for kMaxBatch rows at filter setup: a superset for any
//            T) has the bit; the rows preloaded at a split's start are covered by win[c][p0].
//   MACs     a wave none of whose four tiles is kept in row p skips the row's filter load and
//            its 2 T packed FMAs with one uniform branch each; the window slides all the same,
//            since the slot renaming is static.
//   past P   a sparse handle has no zero filter rows behind P: the per-row words of partitions
//            >= P are taken as zero without a load, so those steps fetch and add nothing.
// The order of a bin's sum is fixed by (T, splits); there are no atomics: equal calls give equal
// bits.
//
// Per-row words (bitmap word, window word, tile offset) are loaded T + D rows at a time, one row per
// lane, a chunk ahead, and read with v_readlane at a static lane: no scalar load waits in the loop.
#include "sparse_plan.hpp"
#include "upols_handle.hpp"
#include "upols_step.hpp"

namespace neo_hip {

constexpr int kSbDepth = 8;  // rows in flight per lane (divides or exceeds every T)

// the channel's filter and FDL as the MAC reads them
struct sb_src {
    const uint32_t* bits;  // [P][NW] of this channel
    const uint32_t* win;   // [P][NW] of this channel
    const uint32_t* off;   // [P + 1] of this channel, tile units
    __amdgpu_buffer_rsrc_t val;  // this channel's compacted tiles
    __amdgpu_buffer_rsrc_t fdl;  // this channel's FDL ring
    int prow;                    // FDL row stride in bytes
    int P, NW;
};
// what a lane knows of its bin: tile bit, the bits below it, the wave's four tile bits, offsets
struct sb_lane {
    uint32_t bit, below, wave;
    int sub, xoff, word;
    bool bin0;
};
// lane l: the words of row (first row + l); zero for rows at or past P
struct sb_meta {
    uint32_t word, win, pre;  // pre: the row's tile offset plus the kept tiles of its words below `word`
};

template<int N>
__device__ __forceinline__ sb_meta sb_meta_load(const sb_src& sp, const sb_lane& ln, int row0, int l)
{
    sb_meta m{0u, 0u, 0u};
    const int p = row0 + l;
    if (l < N && p < sp.P) {
        const uint32_t* b = sp.bits + int64_t(p) * sp.NW;
        m.word = b[ln.word];
        m.win = sp.win[int64_t(p) * sp.NW + ln.word];
        uint32_t pre = sp.off[p];
        for (int i = 0; i < ln.word; ++i) pre += uint32_t(__builtin_popcount(b[i]));
        m.pre = pre;
    }
    return m;
}

template<bool NT>
__device__ __forceinline__ f2v sb_ld(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    const auto u = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, NT ? 2 : 0);
    return __builtin_bit_cast(f2v, u);
}

// FDL row entering the window at partition pn (write position w); pn >= P: any row, every lane drops
__device__ __forceinline__ f2v sb_ld_fdl(const sb_src& sp, const sb_lane& ln, uint32_t win, int w, int pn, int ring)
{
    int r = w - pn;
    r = r < 0 ? r + ring : r;
    r = pn < sp.P ? r : 0;
    return sb_ld<true>(sp.fdl, win & ln.bit ? ln.xoff : kSparseDrop, r * sp.prow);
}
template<bool HNT>
__device__ __forceinline__ f2v sb_ld_h(const sb_src& sp, const sb_lane& ln, uint32_t word, uint32_t pre)
{
    const int ht = int(pre + uint32_t(__builtin_popcount(word & ln.below))) * 128 + ln.sub;
    return sb_ld<HNT>(sp.val, word & ln.bit ? ht : kSparseDrop, 0);
}

// a += h x and a += h x.yx as one v_pk_fma_f32 each, the accumulator tied to its register: written
// as __builtin_elementwise_fma under the wave-uniform branch of sb_step, the accumulators were kept
// twice (one copy per side of the branch, T moves per taken step, and T = 32 spilled)
__device__ __forceinline__ void sb_fma(f2v& a, f2v h, f2v x)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a) : "v"(h), "v"(x));
}
__device__ __forceinline__ void sb_fma_yx(f2v& a, f2v h, f2v x)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,0,1]" : "+v"(a) : "v"(h), "v"(x));
}

// Step U of a T-step chunk (p = pb + U, U static): FDL row (w - p) from prefetch slot U mod D into
// window slot (T - U) mod T, the loads of partition p + D issued (its words from lane U + D of m,
// the rows pb .. pb + T + D - 1), then the MACs of all T blocks if the wave keeps a tile of row p. The
// complex product per bin is k_batch_mac's A2 form: (re, im) += (hr, hr)(xr, xi) + (-hi, hi)
// (xi, xr), the lane of the packed bin 0 with (hr, hi) and (0, 0) instead.
template<int T, int D, bool HNT, int U>
__device__ __forceinline__ void sb_step(f2v (&a)[T], f2v (&f)[T], f2v (&ph)[D], f2v (&pf)[D], uint32_t (&hw)[D],
                                        const sb_src& sp, const sb_lane& ln, const sb_meta& m, int ring, int w, int p)
{
    constexpr int slot = U % D;
    f[(T - U) % T] = pf[slot];
    const f2v hv = ph[slot];
    const uint32_t cur = hw[slot];
    {
        const uint32_t nword = uint32_t(__builtin_amdgcn_readlane(int(m.word), U + D));
        const uint32_t nwin = uint32_t(__builtin_amdgcn_readlane(int(m.win), U + D));
        const uint32_t npre = uint32_t(__builtin_amdgcn_readlane(int(m.pre), U + D));
        pf[slot] = sb_ld_fdl(sp, ln, nwin, w, p + D, ring);
        hw[slot] = nword & ln.wave;
        f2v hn = f2v(0.0f);  // (a conditional store into ph[] itself made the compiler copy the whole array)
        if (hw[slot]) hn = sb_ld_h<HNT>(sp, ln, nword, npre);
        ph[slot] = hn;
    }
    if (cur) {
        const float hr = hv.x, hi = hv.y;
        const float s = ln.bin0 ? 0.0f : hi;
        const f2v h1 = {hr, ln.bin0 ? hi : hr}, h2 = {-s, s};
        // two sweeps over the blocks, so consecutive FMAs never chain on one accumulator
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const f2v x = f[(j - U + T) % T];
                if (k == 0) sb_fma(a[j], h1, x);
                else sb_fma_yx(a[j], h2, x);
            }
    }
    __builtin_amdgcn_sched_barrier(0);  // keep each step's loads D steps ahead, not all hoisted
}

template<int T, int D, bool HNT, int... U>
__device__ __forceinline__ void sb_chunk(f2v (&a)[T], f2v (&f)[T], f2v (&ph)[D], f2v (&pf)[D], uint32_t (&hw)[D],
                                         const sb_src& sp, const sb_lane& ln, const sb_meta& m, int ring, int w, int pb,
                                         std::integer_sequence<int, U...>)
{
    (sb_step<T, D, HNT, U>(a, f, ph, pf, hw, sp, ln, m, ring, w, pb + U), ...);
}

// grid C x S x G (G = max(1, B / L) bin chunks per row), L = min(256, max(64, B)) lanes: below
// B = 64 the lanes past the row own no tile (their bits are never set) and store nothing. The
// register budget is k_batch_mac variant 3's: 2 waves per SIMD, T accumulator pairs, T window
// pairs, 2 D prefetch pairs; B only enters through G and the bitmap word, so the kernel is
// instantiated per (L, T).
template<int L, int T, int D = (T < kSbDepth ? T : kSbDepth)>
__global__ __launch_bounds__(L, 2) void k_sparse_batch_mac(const uint32_t* __restrict__ bits,
    const uint32_t* __restrict__ win, const uint32_t* __restrict__ off, const int64_t* __restrict__ base,
    const cf* __restrict__ val, const cf* __restrict__ fdl, cf* __restrict__ part, int B, int P, int ring, int S,
    int rows, int w, int64_t cstride, int64_t pstride, int pc)
{
    const int G = B > L ? B / L : 1;
    const int cs = blockIdx.x / G, gch = blockIdx.x - cs * G;
    const int bin = gch * L + threadIdx.x;  // packed bin of this lane
    const int c = cs / S, s = cs - c * S;
    const int p0 = s * rows, p1 = min(P, p0 + rows);
    const int NW = sparse_words(B);
    const uint32_t* off_c = off + int64_t(c) * (P + 1);
    // the channel's tiles and its FDL ring, each < 2 GiB (make_upols_shape)
    const sb_src sp{bits + int64_t(c) * P * NW, win + int64_t(c) * P * NW, off_c,
                    __builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(val + base[c] * kSparseTile), 0,
                                                      int(off_c[P]) * 128, 0x00020000),
                    __builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(fdl + int64_t(c) * cstride), 0,
                                                      int(int64_t(ring) * pstride * int64_t(sizeof(cf))), 0x00020000),
                    int(pstride * int64_t(sizeof(cf))), P, NW};
    const int tile = bin / kSparseTile;
    sb_lane ln;
    ln.bit = 1u << (tile & 31);
    ln.below = ln.bit - 1u;
    // a wave's 64 bins are four tiles, the bits (tile & 31) & ~3 .. + 3 of one word
    ln.wave = 0xfu << __builtin_amdgcn_readfirstlane((tile & 31) & ~3);
    ln.sub = (bin & (kSparseTile - 1)) * int(sizeof(cf));
    ln.xoff = bin * int(sizeof(cf));
    ln.word = (gch * L / kSparseTile) >> 5;  // one word per workgroup: L <= 256 bins are <= 16 tiles
    ln.bin0 = bin == 0;
    const int l = threadIdx.x & 63;

    f2v a[T], f[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        a[j] = f2v(0.0f);
        f[j] = f2v(0.0f);
    }
    sb_meta m = sb_meta_load<T + D>(sp, ln, p0, l);  // rows p0 .. p0 + T + D - 1
    {
        const uint32_t w0 = uint32_t(__builtin_amdgcn_readlane(int(m.win), 0));  // win[c][p0]
#pragma unroll
        for (int sl = 1; sl < T; ++sl) {  // rows block sl needs at p0 (entered at partition p0 - sl)
            int r = w + sl - p0;
            r = r < 0 ? r + ring : (r >= ring ? r - ring : r);
            f[sl] = sb_ld<true>(sp.fdl, w0 & ln.bit ? ln.xoff : kSparseDrop, r * sp.prow);
        }
    }
    f2v ph[D], pf[D];
    uint32_t hw[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {  // prefetch partitions p0 .. p0 + D - 1
        const uint32_t nword = uint32_t(__builtin_amdgcn_readlane(int(m.word), d));
        const uint32_t nwin = uint32_t(__builtin_amdgcn_readlane(int(m.win), d));
        const uint32_t npre = uint32_t(__builtin_amdgcn_readlane(int(m.pre), d));
        pf[d] = sb_ld_fdl(sp, ln, nwin, w, p0 + d, ring);
        hw[d] = nword & ln.wave;
        f2v hn = f2v(0.0f);
        if (hw[d]) hn = p0 + d < pc ? sb_ld_h<false>(sp, ln, nword, npre) : sb_ld_h<true>(sp, ln, nword, npre);
        ph[d] = hn;
    }
    // the two workgroups of a CU trade issue priority in slices of 2^11 s_memrealtime ticks, as in
    // k_batch_mac
    const int half = blockIdx.x >= gridDim.x / 2;
    auto share = [&]() {
        const bool mine_old = ((__builtin_amdgcn_s_memrealtime() >> 11) & 1) == 0;
        if (half ? !mine_old : mine_old) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(0);
    };
    // splits hold a multiple of T partitions; the last split's final chunk runs past P, where
    // every word is zero. Chunks starting below pc load filter tiles cacheable, the rest
    // nontemporally (k_batch_mac's two ranges). Every chunk loads the next one's words first.
    int pb = p0;
    for (; pb < p1 && pb < pc; pb += T) {
        share();
        const sb_meta mn = sb_meta_load<T + D>(sp, ln, pb + T, l);
        sb_chunk<T, D, false>(a, f, ph, pf, hw, sp, ln, m, ring, w, pb, std::make_integer_sequence<int, T>{});
        m = mn;
    }
    for (; pb < p1; pb += T) {
        share();
        const sb_meta mn = sb_meta_load<T + D>(sp, ln, pb + T, l);
        sb_chunk<T, D, true>(a, f, ph, pf, hw, sp, ln, m, ring, w, pb, std::make_integer_sequence<int, T>{});
        m = mn;
    }
    __builtin_amdgcn_s_setprio(0);

    if (bin < B) {
        cf* slab = part + (int64_t(c) * S + s) * T * B + bin;
#pragma unroll
        for (int j = 0; j < T; ++j) slab[int64_t(j) * B] = cf{a[j].x, a[j].y};
    }
}

int launch_sparse_batch_mac(const upols_t* h, int T, hipStream_t s)
{
    const int B = h->B, L = B < 64 ? 64 : B > 256 ? 256 : B;
    const unsigned grid = unsigned(h->C) * unsigned(h->shape.Sb) * unsigned(B > L ? B / L : 1);
#define NEO_SB_LAUNCH(LL, TT)                                                                                    \
    hipLaunchKernelGGL((k_sparse_batch_mac<LL, TT>), dim3(grid), dim3(LL), 0, s, h->sp_bits, h->sp_win, h->sp_off, \
                       h->sp_base, h->sp_val, h->fdl, h->part_b, B, h->P, h->ring, h->shape.Sb, h->shape.rows_b, h->wpos,      \
                       h->shape.cstride, h->shape.pstride, h->shape.pcb)
#define NEO_SB_T(TT)                                \
    case TT:                                        \
        if (L == 64) NEO_SB_LAUNCH(64, TT);         \
        else if (L == 128) NEO_SB_LAUNCH(128, TT);  \
        else NEO_SB_LAUNCH(256, TT);                \
        break;
    switch (T) {
        NEO_SB_T(2)
        NEO_SB_T(4)
        NEO_SB_T(8)
        NEO_SB_T(16)
        NEO_SB_T(32)
        default: return fail(NEO_HIP_EINVAL, "batch of %d blocks not available", T);
    }
#undef NEO_SB_T
#undef NEO_SB_LAUNCH
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

}  // namespace neo_hip
