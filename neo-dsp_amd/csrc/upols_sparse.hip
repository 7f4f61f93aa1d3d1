// upols_sparse.hip — sparse (perceptually thinned) UPOLS / UPOLA convolvers on tile-compacted
// filters: sparse_upols_convolver / sparse_upola_convolver (src/neo/convolution/
// sparse_convolver.hpp:12-17) over sparse_filter (sparse_filter.hpp:25-45), whose CSR
// multiply_add (src/neo/algorithm/multiply_add.hpp:303-324) adds exactly the kept terms.
//
// Format (sparse_plan.hpp): the unit is a 128-B tile of 16 packed bins, not a bin -- a gather of
// single 8-B bins would still move whole 128-B requests. Per filter row a bitmap of kept tiles
// and a tile offset into the channel's compacted values; the FDL stays [C][R][B] and every step
// inserts the whole new row (later partitions keep other tiles). Beside the bitmaps the setup
// makes the window bitmaps of the batched pass (upols_sparse_batch.hip).
//
// Step: k_upols_sparse_step is the dense plain step (upols_step.hpp: window r2c, FDL insert,
// acc4 accumulators, row-group fold, slabs, last-arriver tail or k_upols_finish) with the loop
// over the partitions reading only the kept tiles of the filter AND of the FDL rows. The order
// of the sums per bin is the dense order with the dropped terms left out, so with the same
// splits a sparse handle equals the dense plain step on the zeroed filter bit for bit (a 0 * x
// term leaves a float sum unchanged), up to the sign of zero.
//
// Banks: the tables and tiles of one filter are a sparse_bank (upols_handle.hpp). The setup fills the
// bank it is given (sparse_fill: one packing path), the handle's current one for the resetting filter
// calls, the spare one for a live update (upols_sparse_fade.hip has the fade step); at the end of a
// fade the two swap by pointer (sparse_fade_swap).
#include "sparse_plan.hpp"
#include "upols_handle.hpp"
#include "upols_step.hpp"

#include <algorithm>

namespace neo_hip {

// Rows in flight per lane and workgroups per CU, so that no instantiation spills: B < 128 (a wave
// spans several rows: the bitmap words and offsets are per-lane loads) 2 rows; B = 128 .. 512 4
// rows in the 64 registers of 8 waves per SIMD, as the dense step; B = 1024 (two float4 per lane
// and row) 4 rows at 4 waves per SIMD -- the dense step's 2 rows at 8 waves, with the bitmap
// arithmetic on top, spilled 6 registers; B >= 2048 as the dense step. 8 rows in flight at 4
// waves per SIMD for B = 128 .. 1024 measured no faster at any density: below a
// quarter of the tiles the step is bound by the instructions per row, not by bytes in flight.
template<int B>
constexpr int sparse_unroll() { return upols_cfg<B>::QT < 64 ? 2 : upols_cfg<B>::VPT >= 4 ? 1 : 4; }
template<int B>
constexpr int sparse_wgs() { return B < 1024 ? 8 : B == 1024 ? 4 : 2; }

template<int B, bool FUSED, bool OLA>
__global__ __launch_bounds__(256, sparse_wgs<B>()) void k_upols_sparse_step(
    const float* __restrict__ in, int64_t ld_in, float* __restrict__ out, int64_t ld_out, float* __restrict__ prev,
    const uint32_t* __restrict__ bits, const uint32_t* __restrict__ off, const int64_t* __restrict__ base,
    const float4* __restrict__ val, cf* __restrict__ fdl, cf* __restrict__ part, int* __restrict__ arrivals,
    const cf* __restrict__ twg, int P, int ring, int S, int rows, int w, int64_t cstride, int64_t pstride, int pc)
{
    __shared__ step_lds<B> L;
    const int c = blockIdx.x / S, s = blockIdx.x - c * S;
    const uint32_t* off_c = off + int64_t(c) * (P + 1);
    // the channel's tiles and its FDL ring, each < 2 GiB (make_upols_shape)
    const sparse_rows sp{bits + int64_t(c) * P * upols_cfg<B>::VPT, off_c,
                         __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(val + base[c] * 8), 0,
                                                           int(off_c[P]) * 128, 0x00020000),
                         __builtin_amdgcn_make_buffer_rsrc(fdl + int64_t(c) * cstride, 0,
                                                           int(int64_t(ring) * pstride * int64_t(sizeof(cf))), 0x00020000),
                         int(pstride * int64_t(sizeof(cf)))};
    (void)upols_step_wg<B, FUSED, OLA, false, sparse_unroll<B>(), false, sparse_rows>(
        L, c, s, in, ld_in, out, ld_out, prev, nullptr, fdl, part, arrivals, twg, P, ring, S, rows, w, cstride, pstride,
        pc, nullptr, sp);
}

// -- setup: bitmaps and counts, per-channel scan, channel bases, compaction ---------------------

// One workgroup per filter row (c, p): lane t < NT looks at the 16 mask columns of tile t (tile 0
// also at column B, the Nyquist bin packed beside DC); the wave ballots are the bitmap words.
// off[c][p] = the row's popcount (scanned by k_sparse_scan); the kept columns add up in kept_cols.
__global__ __launch_bounds__(256) void k_sparse_rows(const uint8_t* __restrict__ mask, int B, int P,
                                                     uint32_t* __restrict__ bits, uint32_t* __restrict__ off,
                                                     unsigned long long* __restrict__ kept_cols)
{
    __shared__ uint32_t wd[8];
    __shared__ int cols;
    const int tid = threadIdx.x, NT = B / kSparseTile, NW = sparse_words(B);
    const int64_t r = blockIdx.x, c = r / P, p = r - c * P;
    const uint8_t* m = mask + r * (int64_t(B) + 1);
    if (tid == 0) cols = 0;
    __syncthreads();
    int n = 0;
    if (tid < NT) {
        for (int j = 0; j < kSparseTile; ++j) n += m[tid * kSparseTile + j] != 0;
        if (tid == 0) n += m[B] != 0;
    }
    const unsigned long long bal = __ballot(n != 0);
    if ((tid & 63) == 0) {
        wd[2 * (tid >> 6)] = uint32_t(bal);
        wd[2 * (tid >> 6) + 1] = uint32_t(bal >> 32);
    }
    if (n) atomicAdd(&cols, n);
    __syncthreads();
    if (tid < NW) bits[r * NW + tid] = wd[tid];
    if (tid == 0) {
        uint32_t k = 0;
        for (int i = 0; i < NW; ++i) k += uint32_t(__popc(wd[i]));
        off[c * (int64_t(P) + 1) + p] = k;
        if (cols) atomicAdd(kept_cols, (unsigned long long)cols);
    }
}

// The window bitmaps of the batched pass (sparse_plan.hpp sparse_window_plan, window kMaxBatch):
// one lane per word, win[c][p][i] = OR of bits[c][q][i] over q in [p, min(P, p + kMaxBatch)); their
// popcounts add up in win_tiles.
__global__ __launch_bounds__(256) void k_sparse_win(const uint32_t* __restrict__ bits, int P, int NW, int64_t n,
                                                    uint32_t* __restrict__ win, unsigned long long* __restrict__ win_tiles)
{
    __shared__ int tiles;
    if (threadIdx.x == 0) tiles = 0;
    __syncthreads();
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) {
        const int64_t r = i / NW;
        const int p = int(r % P), q1 = min(P, p + kMaxBatch);
        uint32_t wv = 0;
        for (int q = p; q < q1; ++q) wv |= bits[i + int64_t(q - p) * NW];
        win[i] = wv;
        if (wv) atomicAdd(&tiles, __popc(wv));
    }
    __syncthreads();
    if (threadIdx.x == 0 && tiles) atomicAdd(win_tiles, (unsigned long long)tiles);
}

// One workgroup per channel: off[c][0..P) counts -> exclusive prefix sums, off[c][P] = the total.
// Lane t scans the rows [t chunk, (t + 1) chunk); the 256 chunk sums are scanned by lane 0.
__global__ __launch_bounds__(256) void k_sparse_scan(uint32_t* __restrict__ off, int P)
{
    __shared__ uint32_t sum[256];
    const int tid = threadIdx.x;
    uint32_t* o = off + int64_t(blockIdx.x) * (int64_t(P) + 1);
    const int chunk = (P + 255) / 256, lo = min(P, tid * chunk), hi = min(P, lo + chunk);
    uint32_t k = 0;
    for (int p = lo; p < hi; ++p) k += o[p];
    sum[tid] = k;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const uint32_t v = sum[i];
            sum[i] = run;
            run += v;
        }
        o[P] = run;
    }
    __syncthreads();
    uint32_t run = sum[tid];
    for (int p = lo; p < hi; ++p) {
        const uint32_t v = o[p];
        o[p] = run;
        run += v;
    }
}

// base[c] = channel c's first tile in the compacted values, base[C] = the total
__global__ void k_sparse_base(const uint32_t* __restrict__ off, int C, int P, int64_t* __restrict__ base)
{
    if (blockIdx.x || threadIdx.x) return;
    int64_t run = 0;
    for (int c = 0; c < C; ++c) {
        base[c] = run;
        run += off[int64_t(c) * (int64_t(P) + 1) + P];
    }
    base[C] = run;
}

// One workgroup per filter row: the kept tiles of filter [C][P][B + 1] (reference layout), packed
// (bin 0 = {DC, Nyquist}), the columns the mask drops as zero, DC and Nyquist each on its own.
__global__ __launch_bounds__(256) void k_sparse_pack(const cf* __restrict__ filter, const uint8_t* __restrict__ mask,
                                                     int B, int P, const uint32_t* __restrict__ bits,
                                                     const uint32_t* __restrict__ off, const int64_t* __restrict__ base,
                                                     cf* __restrict__ val)
{
    const int NW = sparse_words(B);
    const int64_t r = blockIdx.x, c = r / P, p = r - c * P;
    const cf* src = filter + r * (int64_t(B) + 1);
    const uint8_t* m = mask + r * (int64_t(B) + 1);
    const uint32_t* wd = bits + r * NW;
    const int64_t row0 = base[c] + off[c * (int64_t(P) + 1) + p];
    for (int k = threadIdx.x; k < B; k += 256) {
        const int t = k / kSparseTile, word = t >> 5, bit = t & 31;
        const uint32_t b = wd[word];
        if (!((b >> bit) & 1u)) continue;
        int idx = __popc(b & ((1u << bit) - 1u));
        for (int i = 0; i < word; ++i) idx += __popc(wd[i]);
        cf v;
        if (k == 0) v = cf{m[0] ? src[0].x : 0.f, m[B] ? src[B].x : 0.f};
        else v = m[k] ? src[k] : cf{0.f, 0.f};
        val[(row0 + idx) * kSparseTile + (k & (kSparseTile - 1))] = v;
    }
}

namespace {

// a bank's fixed-size tables, zeroed on s: an empty filter (no tile kept, every offset zero)
int bank_tables(const upols_t* h, sparse_bank& b, hipStream_t s)
{
    const size_t rows = size_t(h->C) * size_t(h->P), words = rows * sparse_words(h->B) * sizeof(uint32_t);
    if (dalloc(&b.bits, words) || dalloc(&b.win, words) || dalloc(&b.off, (rows + h->C) * sizeof(uint32_t)) ||
        dalloc(&b.base, size_t(h->C + 3) * sizeof(int64_t)))
        return NEO_HIP_ENOMEM;
    NEO_HIP_CHECK(hipMemsetAsync(b.bits, 0, words, s));
    NEO_HIP_CHECK(hipMemsetAsync(b.win, 0, words, s));
    NEO_HIP_CHECK(hipMemsetAsync(b.off, 0, (rows + h->C) * sizeof(uint32_t), s));
    NEO_HIP_CHECK(hipMemsetAsync(b.base, 0, size_t(h->C + 3) * sizeof(int64_t), s));
    return NEO_HIP_OK;
}

void bank_free(sparse_bank& b)
{
    dfree(b.bits);
    dfree(b.win);
    dfree(b.off);
    dfree(b.base);
    dfree(b.val);
    b = sparse_bank{};
}

// what the step reads cacheable follows the current filter's kept bytes
void cache_rows(upols_t* h)
{
    const double bytes = double(h->sp_tiles) * kSparseTile * sizeof(cf);
    h->shape.pc = sparse_cache_rows(h->P, bytes, kCacheBudgetBytes);
    h->shape.pcb = sparse_cache_rows(h->P, bytes, kBatchCacheBudgetBytes);
}

}  // namespace

int sparse_alloc(upols_t* h)
{
    sparse_bank b;
    const int rc = bank_tables(h, b, h->stream);
    sparse_put(h, b);  // (a partial allocation too: the handle's destroy gives it back)
    return rc;
}

void sparse_free(upols_t* h)
{
    sparse_bank b = sparse_cur(h);
    bank_free(b);
    sparse_put(h, b);
    bank_free(h->sp2);
}

// The one packing path: filter and mask [C][P][B + 1] (device) into bank b, on s. The call waits on
// s for the three counts (kept tiles, kept columns, window tiles), never on the device; that wait
// also covers whatever earlier work on s read the bank's old tiles, which go back to the pool after
// it, before the new ones are allocated.
int sparse_fill(upols_t* h, sparse_bank& b, const cf* filter, const uint8_t* mask, hipStream_t s)
{
    const int64_t rows = int64_t(h->C) * h->P;
    if (rows > 0x7fffffff) return fail(NEO_HIP_EINVAL, "too many partitions");
    unsigned long long* cols = reinterpret_cast<unsigned long long*>(b.base + h->C + 1);  // and the window tiles
    NEO_HIP_CHECK(hipMemsetAsync(cols, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_sparse_rows, dim3(unsigned(rows)), dim3(256), 0, s, mask, h->B, h->P, b.bits, b.off, cols);
    NEO_HIP_LAUNCH_CHECK();
    const int64_t words = rows * sparse_words(h->B);
    hipLaunchKernelGGL(k_sparse_win, dim3(unsigned((words + 255) / 256)), dim3(256), 0, s, b.bits, h->P,
                       sparse_words(h->B), words, b.win, cols + 1);
    NEO_HIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sparse_scan, dim3(unsigned(h->C)), dim3(256), 0, s, b.off, h->P);
    NEO_HIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sparse_base, dim3(1), dim3(64), 0, s, b.off, h->C, h->P, b.base);
    NEO_HIP_LAUNCH_CHECK();
    int64_t tot[3] = {0, 0, 0};  // kept tiles, kept columns, window tiles: all that comes back to the host
    NEO_HIP_CHECK(hipMemcpyAsync(tot, b.base + h->C, sizeof tot, hipMemcpyDeviceToHost, s));
    NEO_HIP_CHECK(hipStreamSynchronize(s));  // the call's stream, never the device
    dfree(b.val);
    b.val = nullptr;
    b.tiles = tot[0];
    b.bins = tot[1];
    b.wtiles = tot[2];
    if (!b.tiles) return NEO_HIP_OK;
    if (int rc = dalloc(&b.val, size_t(b.tiles) * kSparseTile * sizeof(cf))) return rc;
    hipLaunchKernelGGL(k_sparse_pack, dim3(unsigned(rows)), dim3(256), 0, s, filter, mask, h->B, h->P, b.bits, b.off,
                       b.base, b.val);
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

// the resetting filter call's store: the caller joined every stream this handle's steps ran on, so
// the old tiles and a retired or cancelled spare bank's tiles are free to go
int sparse_set_filter(upols_t* h, const cf* filter, const uint8_t* mask, hipStream_t s)
{
    sparse_release_spare(h);
    sparse_bank b = sparse_cur(h);
    dfree(b.val);
    b.val = nullptr;
    b.tiles = b.bins = b.wtiles = 0;
    const int rc = sparse_fill(h, b, filter, mask, s);
    sparse_put(h, b);
    cache_rows(h);
    return rc;
}

// A live update's fixed-size buffers, at the first update, kept until the handle goes: the spare
// bank's tables, the fade step's slabs [C][S][2][B] (the plain step's splits, upols_fade_split) and,
// overlap-add, bank B's tails [C][B].
int sparse_fade_buffers(upols_t* h, hipStream_t s)
{
    if (h->sp2.bits) return NEO_HIP_OK;
    const upols_fade_plan f = upols_fade_split(h->shape);
    sparse_bank b;
    cf* slabs = nullptr;
    float* tails = nullptr;
    int rc = bank_tables(h, b, s);
    if (!rc && (dalloc(&slabs, size_t(f.slab_bytes)) || (h->ola && dalloc(&tails, size_t(h->C) * h->B * sizeof(float)))))
        rc = NEO_HIP_ENOMEM;
    if (rc) {
        bank_free(b);
        dfree(slabs);
        dfree(tails);
        return rc == NEO_HIP_ENOMEM ? fail(NEO_HIP_ENOMEM, "filter update: allocation of the second sparse bank failed") : rc;
    }
    h->sp2 = b;
    h->part_f = slabs;
    h->ovl2 = tails;
    h->fade_S = f.S;
    h->fade_rows = f.rows;
    return NEO_HIP_OK;
}

void sparse_fade_swap(upols_t* h)
{
    const sparse_bank a = sparse_cur(h);
    sparse_put(h, h->sp2);
    h->sp2 = a;  // retired: its tiles stay until a wait covers the last fade step (sparse_release_spare, sparse_fill)
    cache_rows(h);
}

void sparse_release_spare(upols_t* h)
{
    dfree(h->sp2.val);
    h->sp2.val = nullptr;
    h->sp2.tiles = h->sp2.bins = h->sp2.wtiles = 0;
}

int64_t sparse_spare_bytes(const upols_t* h)
{
    if (!h->sp2.bits) return 0;
    const int64_t rows = int64_t(h->C) * h->P;
    return (2 * rows * sparse_words(h->B) + rows + h->C) * int64_t(sizeof(uint32_t)) + int64_t(h->C + 3) * int64_t(sizeof(int64_t)) +
           (h->sp2.val ? h->sp2.tiles * int64_t(kSparseTile * sizeof(cf)) : 0);
}

int launch_sparse_mac(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s)
{
    const unsigned grid = unsigned(h->C) * unsigned(h->shape.S);
#define NEO_SPARSE_STEP(FU)                                                                                             \
    NEO_UPOLS_DISPATCH_OLA(h->B, h->ola,                                                                                \
                           hipLaunchKernelGGL((k_upols_sparse_step<BB, FU, OL>), dim3(grid), dim3(256), 0, s, in, ld_in, \
                                              out, ld_out, h->prev, h->sp_bits, h->sp_off, h->sp_base,                  \
                                              reinterpret_cast<const float4*>(h->sp_val), h->fdl, h->part, h->arrivals, \
                                              h->tw, h->P, h->ring, h->shape.S, h->shape.rows, h->wpos,                 \
                                              h->shape.cstride, h->shape.pstride, h->shape.pc))
    if (h->shape.fused) NEO_SPARSE_STEP(true) else NEO_SPARSE_STEP(false)
#undef NEO_SPARSE_STEP
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

}  // namespace neo_hip
