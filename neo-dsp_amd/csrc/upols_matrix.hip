// upols_matrix.hip — matrix (multi-input, multi-output) partitioned convolver: output o is the sum
// over its routes (o, i) of what upols_convolver / upola_convolver gives for (x_i, h[o][i])
// (src/neo/convolution/uniform_partitioned_convolver.hpp:13-65 applied route by route). The
// reference has no such class (its plugin runs one convolver per channel); the structure it saves
// is the frequency-domain one: ONE delay line per input serves every output, the sum over the
// inputs is taken on spectra, so there is ONE inverse transform per output.
//
// Device layout (HBM), packed rows of B complex with bin 0 = {DC, Nyquist} as in upols.hip:
//   H    [nroutes][P][B]  the routes' filters, in the caller's route order
//   FDL  [I][R][B]        one ring per input, R = P rows, write position w
//   prev [I][B]           overlap-save: the input's previous block
//   ovl  [O][B]           overlap-add: the output's overlap tail
//   part [O][S][B]        per-split partial spectra; arrivals [tiles]
//   tab                   k_matrix_step's tile table, behind it the per-output route table of the
//                         offline MAC and the fade step (matrix_plan.hpp): one upload with the filter
//
// A block step is two launches:
//   k_matrix_window  one workgroup per input: window update, packed r2c, FDL row w. Every read of
//                    the caller's input happens here, so `in` and `out` may overlap.
//   k_matrix_step    grid tiles x S. A tile is up to OT consecutive outputs; its row list is the
//                    union of their inputs (ascending) x partitions 0..P-1, cut into S splits at
//                    equal row counts (matrix_plan.hpp). Per row (i, p) a lane loads the FDL row
//                    (w - p) mod R of input i ONCE and one filter row per output of the tile. An
//                    output without a route from i reads through a buffer descriptor of size zero:
//                    the load moves no data, and a uniform branch leaves its accumulators alone.
//                    Splits publish a slab per output; the tile's last split to arrive (FUSED) or
//                    k_upols_finish sums them in the order s = 0..S-1 and runs the c2r tails.
//
// A batched pass (neo_hip_matrix_set_batch: T = 2 .. 32 blocks of a call share one pass over every
// route's filter) needs R >= P + 31 rows, so turning batching on re-lays the ring. Its launches:
//   k_batch_window      (upols_batch.hip) grid I x T: block j into FDL row (w + j) mod R. Every
//                       read of the T blocks of `in` happens here and in
//   k_matrix_save_prev  overlap-save: block T - 1 of every input becomes its previous block,
//   k_matrix_batch_mac  (upols_matrix_batch.hip) slabs part_b [O][Sb][T][B],
//   k_batch_finish      grid O x T, without its save of the previous block (that state is per
//                       input here), and k_batch_ola for overlap-add: the first writes of `out`.
//
// An offline pass (neo_hip_matrix_set_offline: one or two windows of 128 blocks, 256-point transforms
// along the block axis; upols_matrix_offline.hip) needs R >= 128 (ceil(P / 128) + 2) + 1 rows. Its
// launches: k_batch_window and k_matrix_save_prev as above, k_lvf_filter (the routes' segment
// spectra, after a filter change only), k_matrix_off_fwd (per input), k_matrix_off_mac (per
// output), then k_batch_finish on its one slab and k_batch_ola.
//
// A live filter update (neo_hip_matrix_update_filter / _update_impulse; upols_matrix_fade.hip) packs
// the new filter into a second bank H2 and crossfades to it over fade_blocks blocks without touching
// any state: while the fade has blocks left a block is k_matrix_window, k_matrix_fade_step (both
// banks against the same FDL rows) and k_matrix_fade_finish (two c2r, the time-domain mix), whatever
// set_batch / set_offline say; after the last one the banks swap (pointers) and the call goes on in
// passes as before. Overlap-add keeps a tail per bank; bank B's tail of the block before the update
// is formed at the update call by one MAC at write position w - 1 (its rows are all intact).
//
// Window levels (neo_hip_matrix_set_levels; upols_matrix_levels.hip, the plan in matrix_plan.hpp) are
// the gear for long filters with ONE block per call: a single step is then k_matrix_window,
// k_matrix_step unfused over the head, partitions [0, 2 T0), of a compact bank H_head
// [nroutes][2 T0][B], per level one k_matrix_lvl_mac launch (part n mod T of the window after this
// block's, into that window's half of the level's slabs part_l [2][O][S][T][B]) and
// k_matrix_lvl_finish (the head's slabs, row n mod T of every level's current window, the c2r tail).
// n (nblk) counts the blocks since the last reset on every path; whatever advances it without the
// parts leaves the slabs stale and the next level step primes them. The ring stays at P rows.
//
// Host side: the buffers of batching, offline windows, updates and levels are four groups of one shape
// (matrix_group), each taken whole at its first use after a filter and freed with it; the four
// filter calls are two loaders (matrix_load_filter, matrix_load_impulse: a bank, a stream, no wait)
// followed by matrix_set_end (reset, complete on return) or matrix_update_end (the fade armed).
#include "matrix_fade.hpp"
#include "matrix_plan.hpp"
#include "upols_handle.hpp"
#include "upols_step.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

struct neo_hip_matrix {
    int device = 0, I = 0, O = 0, B = 0, P = 0, ring = 0;
    bool ola = false;
    int o_fused = -1, o_split = 0, o_tile = 0;  // the options as given (the plan follows the routes)
    hipStream_t stream = nullptr;
    neo_hip::cf* tw = nullptr;
    neo_hip::cf* fdl = nullptr;  // [I][R][B]
    float* prev = nullptr;       // [I][B]
    float* ovl = nullptr;        // [O][B]
    int wpos = 0;
    // with the filter (set_filter / set_impulse)
    bool ready = false;
    neo_hip::matrix_plan plan;
    neo_hip::cf* H = nullptr;     // [nroutes][P][B]
    neo_hip::cf* part = nullptr;  // [O][S][B]
    int* arrivals = nullptr;      // [tiles]
    int* tab = nullptr;           // tiles [ntiles][4] {first, count, inputs, offset into uni}, uni, rt [O][I]
    const int* rtab = nullptr;    // behind them in tab: off [O + 1], then {input, route} per route, inputs ascending per output
    // batched passes (neo_hip_matrix_set_batch; upols_matrix_batch.hip)
    bool batch = false;
    int b_split = 0;                   // the workgroup target as given (0 auto)
    neo_hip::matrix_batch_plan bplan;  // with the filter, for passes of kMatrixBatch blocks
    neo_hip::cf* part_b = nullptr;     // [O][Sb][32][B]; these three from the first batched pass on
    float* tail = nullptr;             // [O][32][B] overlap-add tails of a pass
    int* btab = nullptr;               // bplan's run_off, runs
    // offline windows (neo_hip_matrix_set_offline; upols_matrix_offline.hip)
    bool offline = false;
    int off_wp = 0;                    // windows per pass as given (0 auto)
    bool off_dirty = true;             // off_hf follows the filter: recomputed at the next offline pass
    neo_hip::cf* off_tw = nullptr;     // the 256-point table (shared); the rest from the first offline pass on
    neo_hip::cf* off_hf = nullptr;     // [routes][nseg][256][B] (+ one row per route) segment spectra
    neo_hip::cf* off_xf = nullptr;     // [I][nseg + 1][256][B] a pass's pair spectra
    neo_hip::cf* off_y = nullptr;      // [O][256][B] a pass's output spectra
    float* off_tail = nullptr;         // [O][256][B] overlap-add tails of a pass
    // live filter updates (neo_hip_matrix_update_filter; upols_matrix_fade.hip): from the first update after a filter on
    neo_hip::cf* H2 = nullptr;     // the spare bank [nroutes][P][B]: bank B while a fade runs
    neo_hip::cf* part2 = nullptr;  // [O][fade_S][2][B] the fade step's slabs
    float* ovl2 = nullptr;         // [O][B] bank B's overlap-add tails
    int fade_S = 1;
    int fade_left = 0, fade_total = 0, fade_curve = 0;  // blocks left of the running fade (0: none)
    // window levels (neo_hip_matrix_set_levels; upols_matrix_levels.hip)
    int64_t nblk = 0;                  // blocks since the last reset, counted on every path
    bool levels = false;
    std::vector<int> lv_windows;       // the windows as given (empty: the default)
    int lv_split = 0;                  // the workgroup target of a part as given (0 auto)
    neo_hip::matrix_level_plan lplan;  // with the filter
    neo_hip::cf* H_head = nullptr;     // [nroutes][head][B] the head's bank; these five from the first level step on
    neo_hip::cf* part_h = nullptr;     // [O][head splits][B]
    neo_hip::cf* part_l = nullptr;     // per level [2][O][S][T][B], level l at lplan.levels[l].slab_off rows
    int* htab = nullptr;               // the head plan's tile table
    int* ltab = nullptr;               // the levels' run tables, level l at lv_tab[l]
    std::vector<int> lv_tab;
    bool head_dirty = true;            // H_head follows the filter: copied at the next level step
    bool lv_primed = false;            // the slabs hold the current windows and the due parts of the next
    neo_hip::stream_set used;
};

namespace neo_hip {

using matrix_t = neo_hip_matrix;

// rows in flight per lane and workgroups per CU: one output per workgroup is the dense plain step
// (U rows, 2 loads each = 8 loads in flight, 8 waves per SIMD up to B = 1024); more outputs keep
// OT + 1 loads per row (9, 10 or 12 in flight) and OT accumulator sets. Those kernels are pinned to
// 4 waves per SIMD (amdgpu_waves_per_eu(4, 4)): a launch bound alone is a lower bound on occupancy,
// and left to itself the compiler took 62-68 registers for 7-8 waves and issued the loads of a
// row group three at a time with a wait between them.
template<int B, int OT>
constexpr int matrix_unroll()
{
    using K = upols_cfg<B>;
    if (OT == 1) return K::U;
    return K::VPT >= 2 ? 2 : OT == 2 ? 3 : 2;
}
template<int B, int OT>
constexpr int matrix_wgs() { return B > 1024 ? 2 : OT == 1 ? 8 : 4; }

template<int B, bool OLA>
__global__ __launch_bounds__(256) void k_matrix_window(const float* __restrict__ in, int64_t ld_in,
                                                       float* __restrict__ prev, cf* __restrict__ fdl,
                                                       const cf* __restrict__ twg, int ring, int w)
{
    using K = upols_cfg<B>;
    __shared__ cf fft[K::LL];
    __shared__ cf tw[K::TW1 + K::TW2];
    const int tid = threadIdx.x, i = blockIdx.x;
    const float* in_i = in + int64_t(i) * ld_in;
    float* prev_i = prev + int64_t(i) * B;
    window_fft<B, OLA>(prev_i, in_i, fft, tw, tid, twg);
    cf* row = fdl + (int64_t(i) * ring + w) * B;
    for (int k = tid; k < B; k += 256) row[k] = r2c_split<B>(fft, tw + K::TW1, k);
    if constexpr (!OLA) {  // the window's second half becomes the next call's first half
        for (int k = tid; k < B / 4; k += 256)
            reinterpret_cast<float4*>(prev_i)[k] = reinterpret_cast<const float4*>(in_i)[k];
    }
}

template<int B, int OT, bool FUSED, bool OLA>
__global__ __launch_bounds__(256, (matrix_wgs<B, OT>()))
__attribute__((amdgpu_waves_per_eu(matrix_wgs<B, OT>(), OT > 1 ? 4 : 8))) void k_matrix_step(
    float* __restrict__ out, int64_t ld_out, float* __restrict__ ovl, const cf* __restrict__ H,
    const cf* __restrict__ fdl, cf* __restrict__ part, int* __restrict__ arrivals, const cf* __restrict__ twg,
    const int* __restrict__ tab, int ntiles, int I, int P, int ring, int S, int w)
{
    using K = upols_cfg<B>;
    constexpr int UNROLL = matrix_unroll<B, OT>();
    __shared__ step_lds<B> L;
    const int tid = threadIdx.x;
    const int t = blockIdx.x / S, s = blockIdx.x - t * S;
    const int first = tab[4 * t], count = tab[4 * t + 1], nuni = tab[4 * t + 2];
    const int* uni = tab + 4 * ntiles + tab[4 * t + 3];
    const int* rt = tab + 4 * ntiles + tab[4 * (ntiles - 1) + 3] + tab[4 * (ntiles - 1) + 2];
    const int n = nuni * P, per = (n + S - 1) / S;
    const int r0 = min(n, s * per), r1 = min(n, r0 + per);

    const int rs = tid / K::QT, q0 = tid - rs * K::QT;
    acc4 a[OT][2 * K::VPT];
#pragma unroll
    for (int o = 0; o < OT; ++o)
#pragma unroll
        for (int v = 0; v < 2 * K::VPT; ++v) a[o][v] = {0.f, 0.f, 0.f, 0.f};

    const int rowbytes = B * int(sizeof(cf));
    // the rows of one input at a time: the input and the tile's routes from it are uniform
    for (int seg = r1 > r0 ? r0 / P : nuni; seg < nuni && seg * P < r1; ++seg) {
        const int i = uni[seg];
        const int pbeg = max(r0, seg * P) - seg * P, pend = min(r1, (seg + 1) * P) - seg * P;
        // a route's filter and an input's ring each span < 2 GiB (make_matrix_plan); no route: a
        // descriptor of size zero, every load through it is out of range and moves no data, and the
        // output's accumulators are left alone (a uniform branch after the loads: 0 * x would carry
        // an Inf or NaN of input i into an output it does not feed)
        __amdgpu_buffer_rsrc_t hd[OT];
        bool has[OT];
#pragma unroll
        for (int o = 0; o < OT; ++o) {
            const int r = o < count ? rt[int64_t(first + o) * I + i] : -1;
            has[o] = r >= 0;
            hd[o] = __builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(H + int64_t(r >= 0 ? r : 0) * P * B), 0,
                                                      r >= 0 ? P * rowbytes : 0, 0x00020000);
        }
        const __amdgpu_buffer_rsrc_t fd = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<cf*>(fdl + int64_t(i) * ring * B), 0, ring * rowbytes, 0x00020000);
        auto rows = [&]<int N>(int p) {
            float4 xv[N][K::VPT], hv[OT][N][K::VPT];
#pragma unroll
            for (int u = 0; u < N; ++u) {
                const int pp = p + u * K::RPI;
                const int fr = w >= pp ? w - pp : w - pp + ring;  // fdl_index.hpp:28-31 ring
#pragma unroll
                for (int v = 0; v < K::VPT; ++v) {
                    const int q = q0 + v * K::QT;
                    xv[u][v] = buf_ld4<false>(fd, fr * rowbytes + q * 16);
#pragma unroll
                    for (int o = 0; o < OT; ++o) hv[o][u][v] = buf_ld4<true>(hd[o], pp * rowbytes + q * 16);
                }
            }
#pragma unroll
            for (int o = 0; o < OT; ++o) {
                if (!has[o]) continue;  // uniform
#pragma unroll
                for (int u = 0; u < N; ++u)
#pragma unroll
                    for (int v = 0; v < K::VPT; ++v) mac2(a[o][2 * v], a[o][2 * v + 1], hv[o][u][v], xv[u][v]);
            }
        };
        int p = pbeg + rs;
        for (; p + (UNROLL - 1) * K::RPI < pend; p += UNROLL * K::RPI) rows.template operator()<UNROLL>(p);
        for (; p < pend; p += K::RPI) rows.template operator()<1>(p);
    }

    // fold the row groups into group 0 (fixed order), one output at a time, and publish the slabs
#pragma unroll
    for (int o = 0; o < OT; ++o) {
        if (o >= count) break;  // uniform
        if constexpr (K::RPI > 1) {
            if (o) __syncthreads();  // the fold of the output before has read red
#pragma unroll
            for (int v = 0; v < K::VPT; ++v) {
                L.red[(tid * K::VPT + v) * 2 + 0] = make_float4(a[o][2 * v].rr, a[o][2 * v].ii, a[o][2 * v].ri, a[o][2 * v].ir);
                L.red[(tid * K::VPT + v) * 2 + 1] =
                    make_float4(a[o][2 * v + 1].rr, a[o][2 * v + 1].ii, a[o][2 * v + 1].ri, a[o][2 * v + 1].ir);
            }
            __syncthreads();
            if (rs == 0) {
#pragma unroll 4
                for (int g = 1; g < K::RPI; ++g) {
#pragma unroll
                    for (int v = 0; v < K::VPT; ++v) {
                        const int idx = ((g * K::QT + q0) * K::VPT + v) * 2;
                        const float4 x0 = L.red[idx], x1 = L.red[idx + 1];
                        a[o][2 * v].rr += x0.x; a[o][2 * v].ii += x0.y; a[o][2 * v].ri += x0.z; a[o][2 * v].ir += x0.w;
                        a[o][2 * v + 1].rr += x1.x; a[o][2 * v + 1].ii += x1.y; a[o][2 * v + 1].ri += x1.z; a[o][2 * v + 1].ir += x1.w;
                    }
                }
            }
        }
        float4* slab = reinterpret_cast<float4*>(part + (int64_t(first + o) * S + s) * B);
        if (rs == 0) {
#pragma unroll
            for (int v = 0; v < K::VPT; ++v) {
                const int q = q0 + v * K::QT;
                const cf b0 = finish(a[o][2 * v], q == 0), b1 = finish(a[o][2 * v + 1], false);
                slab[q] = make_float4(b0.x, b0.y, b1.x, b1.y);
            }
        }
    }
    if constexpr (!FUSED) return;  // k_upols_finish sums the slabs in the next launch
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its stores
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // keep the release's wait (upols_step.hpp)
        const int before = __hip_atomic_fetch_add(arrivals + t, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        L.last = before == S - 1;
    }
    __syncthreads();
    if (!L.last) return;  // uniform per workgroup
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(arrivals + t, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next step
    }
    for (int k = tid; k < K::TW1 + K::TW2; k += 256) L.tw[k] = twg[k];
    __syncthreads();
    auto tail = [&](int o) {
        // sum the S slabs of the output in order s = 0..S-1, 4 loads in flight
        const float4* p4 = reinterpret_cast<const float4*>(part + int64_t(first + o) * S * B);
        for (int q = tid; q < K::Q; q += 256) {
            float4 sum = p4[q];
            int u0 = 1;
            for (; u0 + 3 < S; u0 += 4) {
                float4 r[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = p4[(u0 + u) * K::Q + q];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    sum.x += r[u].x; sum.y += r[u].y; sum.z += r[u].z; sum.w += r[u].w;
                }
            }
            for (; u0 < S; ++u0) {
                const float4 r = p4[u0 * K::Q + q];
                sum.x += r.x; sum.y += r.y; sum.z += r.z; sum.w += r.w;
            }
            reinterpret_cast<float4*>(L.xnew)[q] = sum;
        }
        __syncthreads();
        c2r_tail<B, OLA, (B / 4 <= 256 ? 4 : B / 256)>(L.xnew, L.fft, L.tw, out + int64_t(first + o) * ld_out,
                                                       ovl + int64_t(first + o) * B, tid);
        __syncthreads();  // the tail's reads of xnew and fft done before the next output's
    };
    // one output: no loop (the c2r's loop invariants, hoisted out of one, do not fit 64 registers)
    if constexpr (OT == 1) {
        tail(0);
    } else {
#pragma unroll 1
        for (int o = 0; o < count; ++o) tail(o);
    }
}

// overlap-save after a batched pass's windows: block T - 1 of input i is the next call's previous
// block (grid I; launched before the pass's first write of `out`, which may alias `in`)
__global__ __launch_bounds__(256) void k_matrix_save_prev(const float* __restrict__ in, int64_t ld_in,
                                                          float* __restrict__ prev, int B, int T)
{
    const float4* x4 = reinterpret_cast<const float4*>(in + int64_t(blockIdx.x) * ld_in + int64_t(T - 1) * B);
    float4* p4 = reinterpret_cast<float4*>(prev + int64_t(blockIdx.x) * B);
    for (int k = threadIdx.x; k < B / 4; k += 256) p4[k] = x4[k];
}

// filter [nroutes][P][B + 1] (reference layout) -> packed [nroutes][P][B]
__global__ void k_matrix_pack(const cf* __restrict__ in, cf* __restrict__ out, int B, int64_t rows)
{
    const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= rows * B) return;
    const int64_t r = gid / B, k = gid - r * B;
    const cf* src = in + r * (B + 1);
    out[gid] = k == 0 ? cf{src[0].x, src[B].x} : src[k];
}

namespace {

int matrix_reset_state(matrix_t* m, hipStream_t s)
{
    NEO_HIP_CHECK(hipMemsetAsync(m->fdl, 0, size_t(m->I) * m->ring * m->B * sizeof(cf), s));
    NEO_HIP_CHECK(hipMemsetAsync(m->prev, 0, size_t(m->I) * m->B * sizeof(float), s));
    NEO_HIP_CHECK(hipMemsetAsync(m->ovl, 0, size_t(m->O) * m->B * sizeof(float), s));
    if (m->arrivals) NEO_HIP_CHECK(hipMemsetAsync(m->arrivals, 0, size_t(m->plan.ntiles) * sizeof(int), s));
    if (m->part_l) NEO_HIP_CHECK(hipMemsetAsync(m->part_l, 0, size_t(m->lplan.partial_bytes), s));
    m->wpos = 0;
    m->nblk = 0;
    m->lv_primed = true;  // every row before block 0 is zero, so window 0's slabs are
    return NEO_HIP_OK;
}

template<class... T>
void drop(T*&... p)  // dfree, and the pointers are null again
{
    ((dfree(p), p = nullptr), ...);
}

// The lazily allocated groups (batch, offline, fade) have one shape: matrix_*_buffers takes the whole
// group at its first use after a filter, or through matrix_group none of it; matrix_free_* gives it
// back (the caller joined every stream that used it).
int matrix_group(matrix_t* m, int rc, void (*release)(matrix_t*), const char* what)
{
    if (!rc) return NEO_HIP_OK;
    release(m);
    return fail(rc, "matrix %s buffers: device allocation or table copy failed", what);
}

void matrix_free_batch(matrix_t* m) { drop(m->part_b, m->tail, m->btab); }  // they follow the batch plan

void matrix_free_offline(matrix_t* m)  // they follow the filter
{
    drop(m->off_hf, m->off_xf, m->off_y, m->off_tail);
    m->off_dirty = true;
}

void matrix_free_fade(matrix_t* m)  // they follow the route list; a running fade ends with them
{
    drop(m->H2, m->part2, m->ovl2);
    m->fade_left = m->fade_total = 0;
}

void matrix_free_levels(matrix_t* m)  // they follow the level plan
{
    drop(m->H_head, m->part_h, m->part_l, m->htab, m->ltab);
    m->head_dirty = true;
}

int64_t matrix_offline_bytes(const matrix_t* m)
{
    if (!m->off_hf) return 0;
    const int nseg = matrix_offline_segments(m->P);
    const int64_t spec = int64_t(2 * kMatrixOffWindow) * m->B;
    return (int64_t(m->plan.nroutes) * lvf_spec_stride(nseg, m->B) + int64_t(m->I) * (nseg + kMatrixOffMaxWP - 1) * spec +
            int64_t(m->O) * spec) * int64_t(sizeof(cf)) +
           (m->ola ? int64_t(m->O) * spec * int64_t(sizeof(float)) : 0);
}

void matrix_free_filter(matrix_t* m)
{
    matrix_free_batch(m);
    matrix_free_offline(m);
    matrix_free_fade(m);
    matrix_free_levels(m);
    drop(m->H, m->part, m->arrivals, m->tab);
    m->rtab = nullptr;
    m->ready = false;
}

void matrix_destroy(matrix_t* m)
{
    if (!m) return;
    matrix_free_filter(m);
    drop(m->fdl, m->prev, m->ovl);
    delete m;  // the stream is one of the device's shared four (dmem.hip)
}

// a host table in device memory, complete on return: the vector may be a local
int matrix_upload(int** out, const std::vector<int>& tab, hipStream_t s)
{
    if (int rc = dalloc(out, tab.size() * sizeof(int))) return rc;
    if (hipMemcpyAsync(*out, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail(NEO_HIP_ERUNTIME, "matrix convolver: table copy failed");
    return NEO_HIP_OK;
}

// a setup call runs after every step of this handle, on whatever stream it ran
int matrix_join(matrix_t* m, bool device_input)
{
    if (int rc = m->used.join()) return rc;
    if (device_input)
        if (int rc = null_join()) return rc;
    NEO_HIP_CHECK(hipStreamSynchronize(m->stream));
    return NEO_HIP_OK;
}

// a checked plan (make_matrix_plan with the handle's shape and options) and the buffers that follow
// it, both device tables in one upload; the filter rows are the caller's to fill
int matrix_adopt(matrix_t* m, matrix_plan&& pl)
{
    matrix_free_filter(m);  // the caller joined every stream that used them
    m->plan = std::move(pl);
    // (refused only for a ring that set_batch refuses too: batching is off then)
    if (make_matrix_batch_plan(m->plan, kMatrixBatch, m->b_split, m->bplan)) m->bplan = matrix_batch_plan{};
    // (the windows were checked by set_levels)
    if (make_matrix_level_plan(m->plan, m->lv_windows.empty() ? nullptr : m->lv_windows.data(), int(m->lv_windows.size()),
                               m->lv_split, m->lplan))
        m->lplan = matrix_level_plan{};
    const matrix_plan& p = m->plan;
    std::vector<int> tab = matrix_tile_table(p);
    const size_t ntile = tab.size();
    const std::vector<int> routes = matrix_route_table(p);
    tab.insert(tab.end(), routes.begin(), routes.end());
    const size_t rowbytes = size_t(m->B) * sizeof(cf);
    int rc = dalloc(&m->H, size_t(p.nroutes) * m->P * rowbytes);
    if (!rc) rc = dalloc(&m->part, size_t(m->O) * p.S * rowbytes);
    if (!rc) rc = dalloc(&m->arrivals, size_t(p.ntiles) * sizeof(int));
    if (!rc) rc = matrix_upload(&m->tab, tab, m->stream);
    if (rc) {
        matrix_free_filter(m);
        return rc;
    }
    m->rtab = m->tab + ntile;
    return NEO_HIP_OK;
}

// the ring row d rows after the write position (d < 0: before it; |d| <= ring)
int matrix_row(const matrix_t* m, int d) { return (m->wpos + d + m->ring) % m->ring; }  // fdl_index.hpp:28-37

// the window launch of one block: every read of `in` (k_matrix_window)
int matrix_window(matrix_t* m, const float* in, int64_t ld_in, hipStream_t s)
{
    NEO_UPOLS_DISPATCH_OLA(m->B, m->ola, hipLaunchKernelGGL((k_matrix_window<BB, OL>), dim3(unsigned(m->I)), dim3(256), 0, s,
                                                            in, ld_in, m->prev, m->fdl, m->tw, m->ring, m->wpos))
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

// the windows of a pass of T blocks (k_batch_window: block j into row (w + j) mod R) and, for
// overlap-save, its last block as every input's previous block: every read of `in`
int matrix_pass_windows(matrix_t* m, const float* in, int64_t ld_in, int T, hipStream_t s)
{
    if (int rc = launch_batch_window(m->I, m->B, T, m->ola, in, ld_in, m->prev, m->fdl, m->tw, m->ring, m->wpos, s)) return rc;
    if (!m->ola) {
        hipLaunchKernelGGL(k_matrix_save_prev, dim3(unsigned(m->I)), dim3(256), 0, s, in, ld_in, m->prev, m->B, T);
        NEO_HIP_LAUNCH_CHECK();
    }
    return NEO_HIP_OK;
}

// k_matrix_step at the write position for a plan over the first P partitions of the bank H [nroutes][P][B]
// (the handle's own, or the head of the window levels: unfused, so out, ovl and arrivals are not touched)
int matrix_step_launch(matrix_t* m, const matrix_plan& p, const cf* H, cf* part, int* arrivals, const int* tab, int P,
                       float* out, int64_t ld_out, hipStream_t s)
{
    const unsigned grid = unsigned(p.ntiles) * unsigned(p.S);
#define NEO_MATRIX_STEP(OT_, FU)                                                                                     \
    hipLaunchKernelGGL((k_matrix_step<BB, OT_, FU, OL>), dim3(grid), dim3(256), 0, s, out, ld_out, m->ovl, H, m->fdl, \
                       part, arrivals, m->tw, tab, p.ntiles, m->I, P, m->ring, p.S, m->wpos)
#define NEO_MATRIX_STEP_T(FU)                                                          \
    NEO_UPOLS_DISPATCH_OLA(m->B, m->ola, {                                             \
        constexpr int CAP = matrix_max_tile(BB);                                       \
        if (CAP >= 4 && p.OT == 4) NEO_MATRIX_STEP((CAP >= 4 ? 4 : 1), FU);            \
        else if (CAP >= 2 && p.OT == 2) NEO_MATRIX_STEP((CAP >= 2 ? 2 : 1), FU);       \
        else NEO_MATRIX_STEP(1, FU);                                                   \
    })
    if (p.fused) NEO_MATRIX_STEP_T(true) else NEO_MATRIX_STEP_T(false)
#undef NEO_MATRIX_STEP_T
#undef NEO_MATRIX_STEP
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

int matrix_step(matrix_t* m, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s)
{
    const matrix_plan& p = m->plan;
    if (int rc = matrix_window(m, in, ld_in, s)) return rc;
    if (int rc = matrix_step_launch(m, p, m->H, m->part, m->arrivals, m->tab, m->P, out, ld_out, s)) return rc;
    if (!p.fused) {
        // k_upols_finish: one workgroup per output sums its slabs [S][B] in order and runs the c2r
        // (overlap-add: the output's tail)
        if (int rc = launch_finish_slabs(m->O, m->B, p.S, m->ola, m->part, out, ld_out, m->ovl, m->tw, s)) return rc;
    }
    m->wpos = matrix_row(m, 1);
    return NEO_HIP_OK;
}

// the slabs, the overlap-add tails and the run table, at the first batched pass after a filter or
// a set_batch
int matrix_batch_buffers(matrix_t* m, hipStream_t s)
{
    if (m->part_b) return NEO_HIP_OK;
    const matrix_batch_plan& bp = m->bplan;
    std::vector<int> tab(bp.run_off);
    tab.insert(tab.end(), bp.runs.begin(), bp.runs.end());
    int rc = dalloc(&m->part_b, size_t(m->O) * bp.Sb * kMatrixBatch * m->B * sizeof(cf));
    if (!rc && m->ola) rc = dalloc(&m->tail, size_t(m->O) * kMatrixBatch * m->B * sizeof(float));
    if (!rc) rc = matrix_upload(&m->btab, tab, s);
    return matrix_group(m, rc, matrix_free_batch, "batch");
}

// T = 2 .. 32 blocks in one pass over every route's filter (the ring has P + 31 rows: set_batch)
int matrix_batch(matrix_t* m, const float* in, int64_t ld_in, float* out, int64_t ld_out, int T, hipStream_t s)
{
    if (int rc = matrix_batch_buffers(m, s)) return rc;
    if (int rc = matrix_pass_windows(m, in, ld_in, T, s)) return rc;
    if (int rc = launch_matrix_batch_mac(m->H, m->fdl, m->part_b, m->btab, m->B, m->P, m->ring, m->O, m->bplan.Sb, T,
                                         m->wpos, s))
        return rc;
    if (int rc = launch_batch_finish(m->O, m->B, m->bplan.Sb, T, m->ola, m->part_b, nullptr, 0, out, ld_out, nullptr, m->tail, m->ovl,
                                            m->tw, s))
        return rc;
    m->wpos = matrix_row(m, T);
    return NEO_HIP_OK;
}

// the spectra and the overlap-add tails of the offline windows, at the first offline pass after a
// filter; a failure leaves batched passes and single steps as they were
int matrix_offline_buffers(matrix_t* m)
{
    if (m->off_hf) return NEO_HIP_OK;
    if (!m->off_tw)
        if (int rc = shared_far_tw(&m->off_tw)) return rc;
    const int nseg = matrix_offline_segments(m->P);
    const size_t spec = size_t(2 * kMatrixOffWindow) * m->B;
    int rc = dalloc(&m->off_hf, size_t(m->plan.nroutes) * size_t(lvf_spec_stride(nseg, m->B)) * sizeof(cf));
    if (!rc) rc = dalloc(&m->off_xf, size_t(m->I) * (nseg + kMatrixOffMaxWP - 1) * spec * sizeof(cf));
    if (!rc) rc = dalloc(&m->off_y, size_t(m->O) * spec * sizeof(cf));
    if (!rc && m->ola) rc = dalloc(&m->off_tail, size_t(m->O) * spec * sizeof(float));
    return matrix_group(m, rc, matrix_free_offline, "offline");  // (off_dirty is set: matrix_free_offline)
}

// wp windows of 128 blocks in one pass (the ring has 128 (nseg + 2) + 1 rows or more: set_offline, so
// the rows the pass writes are none it reads): every read of `in` is in the first two launches,
// every write of `out` in the last two
int matrix_offline(matrix_t* m, const float* in, int64_t ld_in, float* out, int64_t ld_out, int wp, hipStream_t s)
{
    if (int rc = matrix_offline_buffers(m)) return rc;
    matrix_offline_plan op;
    if (const char* why = make_matrix_offline_plan(m->I, m->O, m->B, m->P, m->plan.nroutes, wp, m->wpos, m->ring, op))
        return fail(NEO_HIP_EINVAL, "matrix offline pass: %s", why);
    if (int rc = matrix_pass_windows(m, in, ld_in, op.T, s)) return rc;
    if (m->off_dirty) {  // the routes stand in for channels: stride P B, one partition per row
        if (int rc = launch_lvf_filter(m->H, m->off_hf, m->off_tw, m->plan.nroutes, m->B, m->P, op.nseg,
                                       int64_t(m->P) * m->B, m->B, 0, s))
            return rc;
        m->off_dirty = false;
    }
    // (pair k's rows: matrix_offline_pair_row, the function op.pair_row was filled from)
    if (int rc = launch_matrix_off_fwd(m->fdl, m->off_xf, m->off_tw, m->I, m->B, op.ring, op.npairs, op.WP, m->wpos, s)) return rc;
    if (int rc = launch_matrix_off_mac(m->off_xf, m->off_hf, m->off_y, m->off_tw, m->rtab, m->O, m->B, op.nseg, op.WP,
                                       lvf_spec_stride(op.nseg, m->B), s))
        return rc;
    if (int rc = launch_batch_finish(m->O, m->B, 1, op.T, m->ola, m->off_y, nullptr, 0, out, ld_out, nullptr, m->off_tail, m->ovl,
                                     m->tw, s))
        return rc;
    m->wpos = matrix_row(m, op.T);
    return NEO_HIP_OK;
}

// the spare bank, the fade step's slabs and bank B's overlap-add tails, at the first update after a
// filter (no host-side wait); a failure leaves the handle as it was
int matrix_fade_buffers(matrix_t* m)
{
    if (m->H2) return NEO_HIP_OK;
    m->fade_S = matrix_fade_splits(m->plan, m->o_split, matrix_fade_chunks(m->B));
    const size_t rowbytes = size_t(m->B) * sizeof(cf);
    int rc = dalloc(&m->H2, size_t(m->plan.nroutes) * m->P * rowbytes);
    if (!rc) rc = dalloc(&m->part2, size_t(m->O) * m->fade_S * 2 * rowbytes);
    if (!rc && m->ola) rc = dalloc(&m->ovl2, size_t(m->O) * m->B * sizeof(float));
    return matrix_group(m, rc, matrix_free_fade, "update");
}

// what every update checks before it touches anything
int matrix_update_check(const matrix_t* m, int fade_blocks, int curve)
{
    if (!m->ready) return fail(NEO_HIP_EINVAL, "matrix update: no filter set (neo_hip_matrix_set_filter)");
    if (fade_blocks < 1 || fade_blocks > kMatrixFadeMaxBlocks)
        return fail(NEO_HIP_EINVAL, "matrix update: fade_blocks must be in [1, %d]", kMatrixFadeMaxBlocks);
    if (curve < 0 || curve >= kMatrixFadeCurves)
        return fail(NEO_HIP_EINVAL, "matrix update: curve must be 0 (linear) or 1 (raised cosine)");
    if (m->fade_left > 0) return fail(NEO_HIP_EINVAL, "matrix update: a fade is still running (%d blocks left)", m->fade_left);
    return NEO_HIP_OK;
}

// bank B (H2) is written on s: overlap-add's tail of the block before (the rows (w - 1 - p) mod
// ring, p < P, are all intact: a step writes row w alone), then the fade is armed
int matrix_fade_arm(matrix_t* m, int fade_blocks, int curve, hipStream_t s)
{
    if (m->ola) {
        if (int rc = launch_matrix_fade_mac(m->H, m->H2, m->fdl, m->part2, m->rtab, m->B, m->P, m->ring, m->O, m->fade_S,
                                            matrix_row(m, -1), s))
            return rc;
        if (int rc = launch_matrix_fade_finish(m->part2, nullptr, 0, m->ovl, m->ovl2, m->tw, m->B, m->O, m->fade_S, true, true,
                                               0, 1, 0, s))
            return rc;
    }
    m->fade_left = m->fade_total = fade_blocks;
    m->fade_curve = curve;
    return NEO_HIP_OK;
}

// the end of a fade: bank B is the filter (pointers swap, no copy), the offline segment spectra follow it
void matrix_fade_swap(matrix_t* m)
{
    std::swap(m->H, m->H2);
    if (m->ola) std::swap(m->ovl, m->ovl2);
    m->fade_left = m->fade_total = 0;
    m->off_dirty = true;
    m->head_dirty = true;
}

// one block of a running fade: the window launch as ever, then both banks against the same FDL rows
int matrix_fade_step(matrix_t* m, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s)
{
    if (int rc = matrix_window(m, in, ld_in, s)) return rc;
    if (int rc = launch_matrix_fade_mac(m->H, m->H2, m->fdl, m->part2, m->rtab, m->B, m->P, m->ring, m->O, m->fade_S, m->wpos, s))
        return rc;
    const int64_t n0 = int64_t(m->fade_total - m->fade_left) * m->B;
    if (int rc = launch_matrix_fade_finish(m->part2, out, ld_out, m->ovl, m->ovl2, m->tw, m->B, m->O, m->fade_S, m->ola, false,
                                           n0, int64_t(m->fade_total) * m->B, m->fade_curve, s))
        return rc;
    m->wpos = matrix_row(m, 1);
    if (--m->fade_left == 0) matrix_fade_swap(m);
    return NEO_HIP_OK;
}

// the head's bank and slabs, the levels' slabs (zero: window 0's after a reset) and the tables, at the
// first level step after a filter or a set_levels
int matrix_level_buffers(matrix_t* m, hipStream_t s)
{
    if (m->part_l) return NEO_HIP_OK;
    const matrix_level_plan& lp = m->lplan;
    std::vector<int> tab;
    m->lv_tab.clear();
    for (const matrix_level& lv : lp.levels) {
        m->lv_tab.push_back(int(tab.size()));
        const std::vector<int> t = matrix_level_table(lv);
        tab.insert(tab.end(), t.begin(), t.end());
    }
    const size_t rowbytes = size_t(m->B) * sizeof(cf);
    int rc = dalloc(&m->H_head, size_t(lp.head_bank_bytes));
    if (!rc) rc = dalloc(&m->part_h, size_t(m->O) * lp.hplan.S * rowbytes);
    if (!rc) rc = dalloc(&m->part_l, size_t(lp.partial_bytes));
    if (!rc) rc = matrix_upload(&m->htab, matrix_tile_table(lp.hplan), s);
    if (!rc) rc = matrix_upload(&m->ltab, tab, s);
    if (!rc && hipMemsetAsync(m->part_l, 0, size_t(lp.partial_bytes), s) != hipSuccess) rc = NEO_HIP_ERUNTIME;
    m->head_dirty = true;
    m->lv_primed = m->nblk == 0;  // fresh slabs are window 0's after a reset, stale after any block
    return matrix_group(m, rc, matrix_free_levels, "level");
}

// One block with window levels on (matrix_plan.hpp, "window levels"): the window launch, the head
// (the ordinary step, unfused, on the compact bank), per level part n mod T of window n / T + 1 into
// that window's half of the slabs, then the finish over the head's slabs and row n mod T of every
// level's current window. Stale slabs (any block that ran without the parts, a changed filter) are
// primed first: the current window whole, and the next window's parts already due in the same launch
// as this block's part (a part is a range of workgroups, each of which computes what it computes in
// any launch: the bits are those of the parts run in their turn).
int matrix_level_step(matrix_t* m, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s)
{
    const matrix_level_plan& lp = m->lplan;
    if (int rc = matrix_level_buffers(m, s)) return rc;
    const size_t rowbytes = size_t(m->B) * sizeof(cf);
    if (m->head_dirty) {  // rows [0, head) of every route (the bank was written on this stream or is complete)
        NEO_HIP_CHECK(hipMemcpy2DAsync(m->H_head, lp.head * rowbytes, m->H, m->P * rowbytes, lp.head * rowbytes,
                                       size_t(m->plan.nroutes), hipMemcpyDeviceToDevice, s));
        m->head_dirty = false;
    }
    if (int rc = matrix_window(m, in, ld_in, s)) return rc;
    if (int rc = matrix_step_launch(m, lp.hplan, m->H_head, m->part_h, nullptr, m->htab, lp.head, out, ld_out, s)) return rc;
    matrix_lvl_rows rows{};
    for (size_t l = 0; l < lp.levels.size(); ++l) {
        const matrix_level& lv = lp.levels[l];
        const int T = lv.T, k = int(m->nblk % T);
        const int64_t W = m->nblk / T, half = int64_t(m->O) * lv.S * T * m->B;
        cf* cur = m->part_l + lv.slab_off * m->B + (W & 1) * half;
        cf* next = m->part_l + lv.slab_off * m->B + ((W + 1) & 1) * half;
        const int* tab = m->ltab + m->lv_tab[l];
        if (!m->lv_primed)
            if (int rc = launch_matrix_lvl_mac(m->H, m->fdl, cur, tab, m->B, m->P, m->ring, m->O, lv.S, T, matrix_row(m, -k), 0,
                                               lv.nwg, s))
                return rc;
        if (int rc = launch_matrix_lvl_mac(m->H, m->fdl, next, tab, m->B, m->P, m->ring, m->O, lv.S, T, matrix_row(m, T - k),
                                           lv.part_cut[size_t(m->lv_primed ? k : 0)], lv.part_cut[size_t(k) + 1], s))
            return rc;
        rows.row[l] = cur + int64_t(k) * m->B;
        rows.S[l] = lv.S, rows.T[l] = T;
    }
    rows.n = int(lp.levels.size());
    if (int rc = launch_matrix_lvl_finish(m->O, m->B, m->ola, m->part_h, lp.hplan.S, rows, out, ld_out, m->ovl, m->tw, s))
        return rc;
    m->wpos = matrix_row(m, 1);
    ++m->nblk;
    m->lv_primed = true;
    return NEO_HIP_OK;
}

// T blocks ran without the levels' parts: their slabs are stale
void matrix_advanced(matrix_t* m, int T)
{
    m->nblk += T;
    m->lv_primed = false;
}

// the blocks of a call: while a fade has blocks left single fade steps; with offline windows on
// passes of 256 (two windows, if allowed) and 128 blocks while that many are left; then with batching
// on the largest power-of-two passes <= 32 of the blocks left, then single steps: level steps with
// window levels on (and a filter long enough to have a level), else plain steps
int matrix_blocks(matrix_t* m, const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t nblocks, hipStream_t s)
{
    for (int64_t t = 0; t < nblocks;) {
        if (m->fade_left > 0) {
            if (int rc = matrix_fade_step(m, in + t * m->B, ld_in, out + t * m->B, ld_out, s)) return rc;
            matrix_advanced(m, 1);
            ++t;
            continue;
        }
        if (m->offline && nblocks - t >= kMatrixOffWindow) {
            const int wp = m->off_wp != 1 && nblocks - t >= 2 * kMatrixOffWindow ? 2 : 1;
            if (int rc = matrix_offline(m, in + t * m->B, ld_in, out + t * m->B, ld_out, wp, s)) return rc;
            matrix_advanced(m, wp * kMatrixOffWindow);
            t += wp * kMatrixOffWindow;
            continue;
        }
        int T = 1;
        if (m->batch) {
            T = kMatrixBatch;
            while (T > nblocks - t) T >>= 1;
        }
        if (T == 1 && m->levels && !m->lplan.levels.empty()) {
            if (int rc = matrix_level_step(m, in + t * m->B, ld_in, out + t * m->B, ld_out, s)) return rc;
            ++t;
            continue;
        }
        const int rc = T > 1 ? matrix_batch(m, in + t * m->B, ld_in, out + t * m->B, ld_out, T, s)
                             : matrix_step(m, in + t * m->B, ld_in, out + t * m->B, ld_out, s);
        if (rc) return rc;
        matrix_advanced(m, T);
        t += T;
    }
    return NEO_HIP_OK;
}

// the ring of R rows re-laid in one of `rows` > R: the R live rows in time order as rows 0 .. R - 1
// (row w is the oldest), the write position R, the rest zero; partition p still pairs with row
// (w - p) mod rows. The caller joined the handle's streams.
int matrix_grow_ring(matrix_t* m, int rows)
{
    const size_t rowbytes = size_t(m->B) * sizeof(cf);
    cf* fresh = nullptr;
    if (dalloc(&fresh, size_t(m->I) * rows * rowbytes))
        return fail(NEO_HIP_ENOMEM, "device allocation of %zu bytes failed", size_t(m->I) * rows * rowbytes);
    const int R = m->ring, w = m->wpos;
    hipError_t e = hipMemsetAsync(fresh, 0, size_t(m->I) * rows * rowbytes, m->stream);
    if (e == hipSuccess)  // old rows w .. R - 1 -> 0 .. R - w - 1
        e = hipMemcpy2DAsync(fresh, rows * rowbytes, m->fdl + size_t(w) * m->B, R * rowbytes, (R - w) * rowbytes,
                             size_t(m->I), hipMemcpyDeviceToDevice, m->stream);
    if (e == hipSuccess && w)  // old rows 0 .. w - 1 -> R - w .. R - 1
        e = hipMemcpy2DAsync(fresh + size_t(R - w) * m->B, rows * rowbytes, m->fdl, R * rowbytes, w * rowbytes,
                             size_t(m->I), hipMemcpyDeviceToDevice, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) {
        dfree(fresh);
        return fail(NEO_HIP_ERUNTIME, "matrix convolver: re-laying the ring failed: %s", hipGetErrorString(e));
    }
    dfree(m->fdl);
    m->fdl = fresh;
    m->ring = rows;
    m->wpos = R;
    return NEO_HIP_OK;
}

// -- the filter calls: set_* = check, join, adopt, load into H on the handle's stream, matrix_set_end;
// update_* = check, the fade's buffers, load into H2 on the call's stream, matrix_update_end ---------

neo_hip_matrix_opts matrix_opts(const neo_hip_matrix_opts* opts) { return opts ? *opts : neo_hip_matrix_opts{-1, 0, 0}; }

// device memory: the caller's stream; host memory: the handle's own unless one is given
hipStream_t matrix_stream(const matrix_t* m, int is_device, void* stream)
{
    return is_device || stream ? as_stream(stream) : m->stream;
}

// a set call's route list against the handle's shape and options
const char* matrix_check_routes(const matrix_t* m, const int* route_out, const int* route_in, int nroutes, matrix_plan& p)
{
    return make_matrix_plan(m->I, m->O, m->B, m->P, route_out, route_in, nroutes, m->o_fused, m->o_split, m->o_tile, p);
}

int matrix_check_impulse(const matrix_t* m, const float* ir, int64_t length)
{
    if (!m || !ir || length < 1) return fail(NEO_HIP_EINVAL, "null handle/ir or empty impulse");
    if (partitions_for(length, m->B) != m->P)
        return fail(NEO_HIP_EINVAL, "impulse of %lld taps gives %lld partitions, convolver has %d", (long long)length,
                    (long long)partitions_for(length, m->B), m->P);
    return NEO_HIP_OK;
}

// scratch of the loaders: stream-ordered (hipFreeAsync on the same stream), so a load never waits
template<class T>
int matrix_scratch(T** out, size_t bytes, hipStream_t s)
{
    if (hipMallocAsync(reinterpret_cast<void**>(out), bytes, s) == hipSuccess) return NEO_HIP_OK;
    (void)hipGetLastError();
    return fail(NEO_HIP_ENOMEM, "device allocation of %zu bytes failed", bytes);
}

// The caller's filter [nroutes][P][B + 1] (reference layout), in host or device memory, packed into
// `bank` [nroutes][P][B] on s. No host-side wait; host memory is staged, the caller synchronises s.
int matrix_load_filter(matrix_t* m, const void* filter, bool is_device, cf* bank, hipStream_t s)
{
    const int64_t rows = int64_t(m->plan.nroutes) * m->P;
    const size_t bytes = size_t(rows) * size_t(m->B + 1) * sizeof(cf);
    const cf* src = static_cast<const cf*>(filter);
    cf* tmp = nullptr;
    int rc = NEO_HIP_OK;
    if (!is_device) {
        if ((rc = matrix_scratch(&tmp, bytes, s))) return rc;
        if (hipMemcpyAsync(tmp, filter, bytes, hipMemcpyHostToDevice, s) != hipSuccess)
            rc = fail(NEO_HIP_ERUNTIME, "filter copy failed");
        src = tmp;
    }
    if (!rc) {
        hipLaunchKernelGGL(k_matrix_pack, dim3(unsigned((rows * m->B + 255) / 256)), dim3(256), 0, s, src, bank, m->B, rows);
        if (hipGetLastError() != hipSuccess) rc = fail(NEO_HIP_ERUNTIME, "pack launch failed");
    }
    if (tmp && hipFreeAsync(tmp, s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "filter scratch free failed");
    return rc;
}

// The same from impulse responses [nroutes][length]: one normalisation factor over all routes' rows,
// as the dense setup takes it over channels (normalize_impulse.hpp:21-30), then uniform_partition.
int matrix_load_impulse(matrix_t* m, const float* ir, int64_t length, bool normalize, bool is_device, cf* bank,
                        hipStream_t s)
{
    const int nroutes = m->plan.nroutes;
    const size_t bytes = size_t(nroutes) * size_t(length) * sizeof(float);
    float* d = nullptr;
    if (int rc = matrix_scratch(&d, bytes, s)) return rc;
    int rc = NEO_HIP_OK;
    if (hipMemcpyAsync(d, ir, bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s) != hipSuccess)
        rc = fail(NEO_HIP_ERUNTIME, "impulse copy failed");
    if (!rc && normalize) rc = normalize_device(d, nroutes, length, s);
    if (!rc) rc = partition_device(d, nroutes, length, m->B, true, bank, m->tw, s, int64_t(m->P) * m->B, m->B);
    if (hipFreeAsync(d, s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "impulse scratch free failed");
    return rc;
}

// a set call after its load (rc): all state reset, complete on return
int matrix_set_end(matrix_t* m, int rc)
{
    if (!rc) rc = matrix_reset_state(m, m->stream);
    if (hipStreamSynchronize(m->stream) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    m->ready = !rc;
    return rc;
}

// the call's stream noted; a host filter's call is synchronous, so it also comes after the handle's
// earlier steps on every stream: they write the delay lines and tails the fade is armed from
// (overlap-add), and the last step of an earlier fade may still read the spare bank
int matrix_update_begin(matrix_t* m, bool is_device, hipStream_t s)
{
    if (!is_device)
        if (int rc = m->used.join()) return rc;
    return m->used.note(s);
}

// an update call after its load (rc): the fade armed; host memory: complete on return
int matrix_update_end(matrix_t* m, int rc, bool is_device, int fade_blocks, int curve, hipStream_t s)
{
    if (!rc) rc = matrix_fade_arm(m, fade_blocks, curve, s);
    if (!is_device && hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    if (rc) m->fade_left = m->fade_total = 0;
    return rc;
}

}  // namespace
}  // namespace neo_hip

using namespace neo_hip;

extern "C" {

NEO_HIP_API int neo_hip_matrix_plan(int inputs, int outputs, int block, int partitions, const int* route_out,
                                    const int* route_in, int nroutes, const neo_hip_matrix_opts* opts,
                                    neo_hip_matrix_plan_info* plan, int* tile_first, int* tile_count, int* tile_rows,
                                    int* union_off, int* union_in, int* cuts)
{
    const neo_hip_matrix_opts o = matrix_opts(opts);
    matrix_plan p;
    if (const char* why = make_matrix_plan(inputs, outputs, block, partitions, route_out, route_in, nroutes, o.fused,
                                           o.split_workgroups, o.out_tile, p))
        return fail(NEO_HIP_EINVAL, "matrix_plan: %s", why);
    if (plan) {
        plan->out_tile = p.OT;
        plan->fused = p.fused ? 1 : 0;
        plan->splits = p.S;
        plan->tiles = p.ntiles;
        plan->fdl_row_loads = p.fdl_loads;
        plan->filter_row_loads = p.filter_loads;
    }
    for (int t = 0; t < p.ntiles; ++t) {
        if (tile_first) tile_first[t] = p.tile_first[size_t(t)];
        if (tile_count) tile_count[t] = p.tile_count[size_t(t)];
        if (tile_rows) tile_rows[t] = p.rows(t);
        if (union_off) union_off[t] = p.uni_off[size_t(t)];
        if (cuts)
            for (int s = 0; s <= p.S; ++s) cuts[int64_t(t) * (kMatrixMaxSplits + 1) + s] = p.cut(t, s);
    }
    if (union_off) union_off[p.ntiles] = p.uni_off[size_t(p.ntiles)];
    if (union_in) std::copy(p.uni.begin(), p.uni.end(), union_in);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_create(int inputs, int outputs, int block, int partitions, int device, int method,
                                      const neo_hip_matrix_opts* opts, neo_hip_matrix** out)
{
    if (!out) return fail(NEO_HIP_EINVAL, "handle pointer is null");
    *out = nullptr;
    if (method < 0 || method > 1)
        return fail(NEO_HIP_EINVAL, "matrix convolvers: method must be 0 (upols) or 1 (upola); whole blocks only");
    const neo_hip_matrix_opts o = matrix_opts(opts);
    {  // the shape and the options, before a device is touched (a one-route list stands in)
        const int zero = 0;
        matrix_plan p;
        if (const char* why = make_matrix_plan(inputs, outputs, block, partitions, &zero, &zero, 1, o.fused,
                                               o.split_workgroups, o.out_tile, p))
            return fail(NEO_HIP_EINVAL, "matrix convolver: %s", why);
    }
    device_guard g(device);
    if (g.rc) return g.rc;
    auto* m = new matrix_t{};
    (void)hipGetDevice(&m->device);
    m->I = inputs, m->O = outputs, m->B = block, m->P = partitions;
    m->ring = partitions;  // one block per step: row w is written before the step's launch reads it
    m->ola = method == 1;
    m->o_fused = o.fused, m->o_split = o.split_workgroups, m->o_tile = o.out_tile;
    auto bail = [&](int code) {
        matrix_destroy(m);
        return code;
    };
    if (int rc = shared_stream(&m->stream)) return bail(rc);
    const size_t rowbytes = size_t(block) * sizeof(cf);
    if (dalloc(&m->fdl, size_t(inputs) * m->ring * rowbytes) || dalloc(&m->prev, size_t(inputs) * block * sizeof(float)) ||
        dalloc(&m->ovl, size_t(outputs) * block * sizeof(float)))
        return bail(fail(NEO_HIP_ENOMEM, "device allocation of %zu bytes failed", size_t(inputs) * m->ring * rowbytes));
    if (int rc = shared_tw(&m->tw, block)) return bail(rc);
    if (int rc = matrix_reset_state(m, m->stream)) return bail(rc);
    if (hipStreamSynchronize(m->stream) != hipSuccess) return bail(fail(NEO_HIP_ERUNTIME, "sync failed"));
    *out = m;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_destroy(neo_hip_matrix* m)
{
    if (!m) return NEO_HIP_OK;
    device_guard g(m->device);
    (void)matrix_join(m, false);
    matrix_destroy(m);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_set_filter(neo_hip_matrix* m, const void* filter, const int* route_out,
                                          const int* route_in, int nroutes, int is_device)
{
    if (!m || !filter) return fail(NEO_HIP_EINVAL, "null handle or filter");
    matrix_plan p;  // a refused route list leaves the handle as it was
    if (const char* why = matrix_check_routes(m, route_out, route_in, nroutes, p))
        return fail(NEO_HIP_EINVAL, "matrix set_filter: %s", why);
    device_guard g(m->device);
    if (g.rc) return g.rc;
    if (int rc = matrix_join(m, is_device != 0)) return rc;
    if (int rc = matrix_adopt(m, std::move(p))) return rc;
    return matrix_set_end(m, matrix_load_filter(m, filter, is_device != 0, m->H, m->stream));
}

NEO_HIP_API int neo_hip_matrix_set_impulse(neo_hip_matrix* m, const float* ir, int64_t length, const int* route_out,
                                           const int* route_in, int nroutes, int normalize, int is_device)
{
    if (int rc = matrix_check_impulse(m, ir, length)) return rc;
    matrix_plan p;
    if (const char* why = matrix_check_routes(m, route_out, route_in, nroutes, p))
        return fail(NEO_HIP_EINVAL, "matrix set_impulse: %s", why);
    device_guard g(m->device);
    if (g.rc) return g.rc;
    if (int rc = matrix_join(m, is_device != 0)) return rc;
    if (int rc = matrix_adopt(m, std::move(p))) return rc;
    return matrix_set_end(m, matrix_load_impulse(m, ir, length, normalize != 0, is_device != 0, m->H, m->stream));
}

NEO_HIP_API int neo_hip_matrix_process(neo_hip_matrix* m, const float* in, int64_t ld_in, float* out, int64_t ld_out,
                                       int64_t nblocks, int is_device, void* stream)
{
    if (!m || !in || !out) return fail(NEO_HIP_EINVAL, "null handle or buffer");
    if (!m->ready) return fail(NEO_HIP_EINVAL, "matrix process: no filter set (neo_hip_matrix_set_filter)");
    if (nblocks < 0 || nblocks > (int64_t(1) << 40) / m->B) return fail(NEO_HIP_EINVAL, "bad block count");
    const int64_t n = nblocks * m->B;
    if (ld_in < n || ld_out < n) return fail(NEO_HIP_EINVAL, "leading dimension smaller than nblocks * block");
    if (is_device && !io_aligned(in, out, ld_in, ld_out))
        return fail(NEO_HIP_EINVAL, "device I/O must be 16-byte aligned (ld multiple of 4)");
    if (!nblocks) return NEO_HIP_OK;
    device_guard g(m->device);
    if (g.rc) return g.rc;
    hipStream_t s = matrix_stream(m, is_device, stream);
    if (int rc = m->used.note(s)) return rc;
    if (is_device) return matrix_blocks(m, in, ld_in, out, ld_out, nblocks, s);
    // host memory: staged ([I][n] in, [O][n] out), synchronous
    float* din = nullptr;
    float* dout = nullptr;
    if (dalloc(&din, size_t(m->I) * n * sizeof(float)) || dalloc(&dout, size_t(m->O) * n * sizeof(float))) {
        dfree(din);
        return fail(NEO_HIP_ENOMEM, "staging allocation failed");
    }
    int rc = NEO_HIP_OK;
    if (hipMemcpy2DAsync(din, size_t(n) * sizeof(float), in, size_t(ld_in) * sizeof(float), size_t(n) * sizeof(float),
                         size_t(m->I), hipMemcpyHostToDevice, s) != hipSuccess)
        rc = fail(NEO_HIP_ERUNTIME, "input copy failed");
    if (!rc) rc = matrix_blocks(m, din, n, dout, n, nblocks, s);
    if (!rc && hipMemcpy2DAsync(out, size_t(ld_out) * sizeof(float), dout, size_t(n) * sizeof(float),
                                size_t(n) * sizeof(float), size_t(m->O), hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(NEO_HIP_ERUNTIME, "output copy failed");
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    dfree(din);
    dfree(dout);
    return rc;
}

NEO_HIP_API int neo_hip_matrix_reset(neo_hip_matrix* m)
{
    if (!m) return fail(NEO_HIP_EINVAL, "null handle");
    device_guard g(m->device);
    if (g.rc) return g.rc;
    if (int rc = matrix_join(m, false)) return rc;
    if (m->fade_left > 0) matrix_fade_swap(m);  // a running fade completes: the new filter is the filter
    if (int rc = matrix_reset_state(m, m->stream)) return rc;
    NEO_HIP_CHECK(hipStreamSynchronize(m->stream));
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_update_filter(neo_hip_matrix* m, const void* filter, int is_device, int fade_blocks,
                                             int curve, void* stream)
{
    if (!m || !filter) return fail(NEO_HIP_EINVAL, "null handle or filter");
    if (int rc = matrix_update_check(m, fade_blocks, curve)) return rc;
    device_guard g(m->device);
    if (g.rc) return g.rc;
    hipStream_t s = matrix_stream(m, is_device, stream);
    if (int rc = matrix_update_begin(m, is_device != 0, s)) return rc;
    if (int rc = matrix_fade_buffers(m)) return rc;
    return matrix_update_end(m, matrix_load_filter(m, filter, is_device != 0, m->H2, s), is_device != 0, fade_blocks, curve, s);
}

NEO_HIP_API int neo_hip_matrix_update_impulse(neo_hip_matrix* m, const float* ir, int64_t length, int normalize,
                                              int is_device, int fade_blocks, int curve, void* stream)
{
    if (int rc = matrix_check_impulse(m, ir, length)) return rc;
    if (int rc = matrix_update_check(m, fade_blocks, curve)) return rc;
    device_guard g(m->device);
    if (g.rc) return g.rc;
    hipStream_t s = matrix_stream(m, is_device, stream);
    if (int rc = matrix_update_begin(m, is_device != 0, s)) return rc;
    if (int rc = matrix_fade_buffers(m)) return rc;
    return matrix_update_end(m, matrix_load_impulse(m, ir, length, normalize != 0, is_device != 0, m->H2, s), is_device != 0,
                             fade_blocks, curve, s);
}

NEO_HIP_API int neo_hip_matrix_fade_info(neo_hip_matrix* m, int* remaining_blocks, int* fade_blocks, int64_t* bank_bytes)
{
    if (!m) return fail(NEO_HIP_EINVAL, "null handle");
    if (remaining_blocks) *remaining_blocks = m->fade_left;
    if (fade_blocks) *fade_blocks = m->fade_total;
    if (bank_bytes) *bank_bytes = m->H2 ? int64_t(m->plan.nroutes) * m->P * m->B * int64_t(sizeof(cf)) : 0;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_set_batch(neo_hip_matrix* m, int enable, int split_workgroups)
{
    if (!m) return fail(NEO_HIP_EINVAL, "null handle");
    if (enable < 0 || enable > 1 || split_workgroups < 0)
        return fail(NEO_HIP_EINVAL, "matrix set_batch: enable must be 0 or 1, split_workgroups >= 0");
    const int rows = m->P + kMatrixBatch - 1;
    if (enable && int64_t(rows) * m->B * int64_t(sizeof(cf)) >= (int64_t(1) << 31))
        return fail(NEO_HIP_EINVAL, "matrix set_batch: an input's ring of P + 31 rows must span < 2 GiB");
    matrix_batch_plan bp;
    if (m->ready)
        if (const char* why = make_matrix_batch_plan(m->plan, kMatrixBatch, split_workgroups, bp))
            return fail(NEO_HIP_EINVAL, "matrix set_batch: %s", why);
    device_guard g(m->device);
    if (g.rc) return g.rc;
    if (int rc = matrix_join(m, false)) return rc;
    if (enable && m->ring < rows)
        if (int rc = matrix_grow_ring(m, rows)) return rc;  // (the state is as it was)
    m->batch = enable != 0;  // off: the larger ring stays, single steps read the same rows in the same order
    m->b_split = split_workgroups;
    if (m->ready) {
        m->bplan = std::move(bp);
        matrix_free_batch(m);  // sized by the plan; the next batched pass allocates them
    }
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_batch_info(neo_hip_matrix* m, int* blocks_per_pass, int* splits, int* ring_rows)
{
    if (!m) return fail(NEO_HIP_EINVAL, "null handle");
    if (blocks_per_pass) *blocks_per_pass = m->batch ? kMatrixBatch : 1;
    if (splits) *splits = m->batch && m->ready ? m->bplan.Sb : 0;
    if (ring_rows) *ring_rows = m->ring;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_set_offline(neo_hip_matrix* m, int enable, int windows_per_pass)
{
    if (!m) return fail(NEO_HIP_EINVAL, "null handle");
    if (enable < 0 || enable > 1 || windows_per_pass < 0 || windows_per_pass > kMatrixOffMaxWP)
        return fail(NEO_HIP_EINVAL, "matrix set_offline: enable must be 0 or 1, windows_per_pass 0 (automatic), 1 or 2");
    const int rows = matrix_offline_ring(m->P);
    if (enable && int64_t(std::max(rows, m->ring)) * m->B * int64_t(sizeof(cf)) >= (int64_t(1) << 31))
        return fail(NEO_HIP_EINVAL, "matrix set_offline: an input's ring of %d rows must span < 2 GiB", rows);
    device_guard g(m->device);
    if (g.rc) return g.rc;
    if (int rc = matrix_join(m, false)) return rc;
    if (enable && m->ring < rows)
        if (int rc = matrix_grow_ring(m, rows)) return rc;  // (the state is as it was)
    m->offline = enable != 0;  // off: the larger ring stays, the other passes read the same rows in the same order
    m->off_wp = windows_per_pass;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_offline_info(neo_hip_matrix* m, int* blocks_per_pass, int* segments, int* ring_rows,
                                            int64_t* spectra_bytes)
{
    if (!m) return fail(NEO_HIP_EINVAL, "null handle");
    if (blocks_per_pass) *blocks_per_pass = m->offline ? kMatrixOffWindow * (m->off_wp == 1 ? 1 : kMatrixOffMaxWP) : 0;
    if (segments) *segments = matrix_offline_segments(m->P);
    if (ring_rows) *ring_rows = m->ring;
    if (spectra_bytes)
        *spectra_bytes = m->off_hf ? int64_t(m->plan.nroutes) * matrix_offline_segments(m->P) * 2 * kMatrixOffWindow * m->B *
                                         int64_t(sizeof(cf))
                                   : 0;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_offline_plan(int inputs, int outputs, int block, int partitions, const int* route_out,
                                            const int* route_in, int nroutes, int windows, int write_pos, int ring_rows,
                                            neo_hip_matrix_offline_plan_info* plan, int* pair_row, int* pair_of)
{
    matrix_plan p;
    if (const char* why = make_matrix_plan(inputs, outputs, block, partitions, route_out, route_in, nroutes, -1, 0, 1, p))
        return fail(NEO_HIP_EINVAL, "matrix_offline_plan: %s", why);
    matrix_offline_plan op;
    if (const char* why = make_matrix_offline_plan(inputs, outputs, block, partitions, nroutes, windows, write_pos, ring_rows, op))
        return fail(NEO_HIP_EINVAL, "matrix_offline_plan: %s", why);
    if (plan) {
        plan->segments = op.nseg;
        plan->windows = op.WP;
        plan->blocks_per_pass = op.T;
        plan->pairs = op.npairs;
        plan->min_ring_rows = op.min_ring;
        plan->ring_rows = op.ring;
        plan->hf_bytes = op.hf_bytes;
        plan->xf_bytes = op.xf_bytes;
        plan->spectrum_rows = op.spec_rows;
        plan->pair_cache_rows = op.cache_rows;
        plan->fdl_rows = op.fdl_rows;
        plan->pair_rows_written = op.xf_rows;
        plan->output_rows = op.y_rows;
        plan->bytes = op.bytes;
        plan->cache_bytes = op.cache_bytes;
    }
    if (pair_row) std::copy(op.pair_row.begin(), op.pair_row.end(), pair_row);
    if (pair_of)  // row `window` of [2][segments]
        for (int w = 0; w < op.WP; ++w)
            for (int q = 0; q < op.nseg; ++q) pair_of[int64_t(w) * op.nseg + q] = matrix_offline_pair_of(op.WP, w, q);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_batch_plan(int inputs, int outputs, int block, int partitions, const int* route_out,
                                          const int* route_in, int nroutes, int blocks, int split_workgroups,
                                          neo_hip_matrix_batch_plan_info* plan, int* out_rows, int* run_off, int* run_in,
                                          int* run_first, int* run_last)
{
    matrix_plan p;
    if (const char* why = make_matrix_plan(inputs, outputs, block, partitions, route_out, route_in, nroutes, -1, 0, 1, p))
        return fail(NEO_HIP_EINVAL, "matrix_batch_plan: %s", why);
    matrix_batch_plan bp;
    if (const char* why = make_matrix_batch_plan(p, blocks, split_workgroups, bp))
        return fail(NEO_HIP_EINVAL, "matrix_batch_plan: %s", why);
    if (plan) {
        plan->blocks = bp.T;
        plan->splits = bp.Sb;
        plan->chunks = bp.G;
        plan->runs = bp.nruns();
        plan->filter_row_loads = bp.filter_rows;
        plan->fdl_row_loads = bp.fdl_rows;
        plan->slab_rows = bp.slab_rows;
        plan->bytes = bp.bytes;
    }
    if (out_rows) std::copy(bp.rows.begin(), bp.rows.end(), out_rows);
    if (run_off)  // row 65 o + s, as neo_hip_matrix_plan's cuts
        for (int o = 0; o < outputs; ++o)
            for (int s = 0; s <= bp.Sb; ++s) run_off[int64_t(o) * (kMatrixMaxSplits + 1) + s] = bp.run_off[size_t(o) * bp.Sb + s];
    for (int k = 0; k < bp.nruns(); ++k) {
        if (run_in) run_in[k] = bp.runs[size_t(4) * k];
        if (run_first) run_first[k] = bp.runs[size_t(4) * k + 2];
        if (run_last) run_last[k] = bp.runs[size_t(4) * k + 3];
    }
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_set_levels(neo_hip_matrix* m, int enable, const int* windows, int nwindows,
                                          int split_workgroups)
{
    if (!m) return fail(NEO_HIP_EINVAL, "null handle");
    if (enable < 0 || enable > 1 || split_workgroups < 0 || (windows && nwindows < 1))
        return fail(NEO_HIP_EINVAL, "matrix set_levels: enable must be 0 or 1, split_workgroups >= 0, nwindows >= 1");
    matrix_level_plan lp;  // refused windows leave the handle as it was
    {
        const int zero = 0;
        matrix_plan one;  // without a filter a one-route list stands in: the windows are checked all the same
        if (!m->ready) (void)make_matrix_plan(m->I, m->O, m->B, m->P, &zero, &zero, 1, -1, 0, 0, one);
        if (const char* why = make_matrix_level_plan(m->ready ? m->plan : one, windows, nwindows, split_workgroups, lp))
            return fail(NEO_HIP_EINVAL, "matrix set_levels: %s", why);
    }
    device_guard g(m->device);
    if (g.rc) return g.rc;
    if (int rc = matrix_join(m, false)) return rc;
    if (enable && m->ring < lp.ring)  // (never today: the schedule's ring is the plain step's, P rows)
        if (int rc = matrix_grow_ring(m, lp.ring)) return rc;
    m->levels = enable != 0;  // off: plain steps; the next level step primes
    m->lv_windows.assign(windows, windows + (windows ? nwindows : 0));
    m->lv_split = split_workgroups;
    matrix_free_levels(m);  // sized by the plan; the next level step allocates them
    m->lplan = m->ready ? std::move(lp) : matrix_level_plan{};
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_levels_info(neo_hip_matrix* m, neo_hip_matrix_levels_desc* d)
{
    if (!m || !d) return fail(NEO_HIP_EINVAL, "null handle or descriptor");
    std::memset(d, 0, sizeof *d);
    d->enabled = m->levels ? 1 : 0;
    d->ring_rows = m->ring;
    if (!m->ready) return NEO_HIP_OK;
    const matrix_level_plan& lp = m->lplan;
    d->levels = int(lp.levels.size());
    d->head = lp.head;
    for (size_t l = 0; l < lp.levels.size(); ++l)
        d->window[l] = lp.levels[l].T, d->first[l] = lp.levels[l].a, d->last[l] = lp.levels[l].b, d->splits[l] = lp.levels[l].S;
    d->primed = m->levels && d->levels && m->lv_primed && (m->part_l || m->nblk == 0) ? 1 : 0;
    d->partial_bytes = lp.partial_bytes;
    d->head_bank_bytes = lp.head_bank_bytes;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_level_plan(int inputs, int outputs, int block, int partitions, const int* route_out,
                                          const int* route_in, int nroutes, const int* windows, int nwindows,
                                          int split_workgroups, neo_hip_matrix_level_plan_info* plan, int* part_cut,
                                          int* run_off, int* run_in, int* run_first, int* run_last)
{
    static_assert(NEO_HIP_MATRIX_MAX_LEVELS == kMatrixMaxLevels && kMatrixLevelMaxSplits == 64 && kMatrixBatch == 32);
    matrix_plan p;
    if (const char* why = make_matrix_plan(inputs, outputs, block, partitions, route_out, route_in, nroutes, -1, 0, 0, p))
        return fail(NEO_HIP_EINVAL, "matrix_level_plan: %s", why);
    if (windows && nwindows < 1) return fail(NEO_HIP_EINVAL, "matrix_level_plan: nwindows must be >= 1");
    matrix_level_plan lp;
    if (const char* why = make_matrix_level_plan(p, windows, nwindows, split_workgroups, lp))
        return fail(NEO_HIP_EINVAL, "matrix_level_plan: %s", why);
    if (plan) {
        std::memset(plan, 0, sizeof *plan);
        plan->levels = int(lp.levels.size());
        plan->head = lp.head, plan->ring_rows = lp.ring, plan->chunks = lp.G;
        if (plan->levels) {
            plan->head_splits = lp.hplan.S, plan->head_out_tile = lp.hplan.OT;
            plan->head_filter_rows = lp.hplan.filter_loads, plan->head_fdl_rows = lp.hplan.fdl_loads;
        }
        plan->partial_bytes = lp.partial_bytes, plan->head_bank_bytes = lp.head_bank_bytes, plan->bytes = lp.bytes;
    }
    const int64_t run_cap = int64_t(nroutes) + int64_t(kMatrixLevelMaxSplits - 1) * outputs;
    for (size_t l = 0; l < lp.levels.size(); ++l) {
        const matrix_level& lv = lp.levels[l];
        if (plan) {
            plan->window[l] = lv.T, plan->first[l] = lv.a, plan->last[l] = lv.b, plan->splits[l] = lv.S;
            plan->workgroups[l] = lv.nwg, plan->runs[l] = lv.nruns();
            plan->filter_rows[l] = lv.filter_rows, plan->fdl_rows[l] = lv.fdl_rows;
        }
        if (part_cut) std::copy(lv.part_cut.begin(), lv.part_cut.end(), part_cut + l * (kMatrixBatch + 1));
        if (run_off) std::copy(lv.run_off.begin(), lv.run_off.end(), run_off + l * (size_t(kMatrixLevelMaxSplits) * outputs + 1));
        for (int k = 0; k < lv.nruns(); ++k) {
            if (run_in) run_in[int64_t(l) * run_cap + k] = lv.runs[size_t(4) * k];
            if (run_first) run_first[int64_t(l) * run_cap + k] = lv.runs[size_t(4) * k + 2];
            if (run_last) run_last[int64_t(l) * run_cap + k] = lv.runs[size_t(4) * k + 3];
        }
    }
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_matrix_info(neo_hip_matrix* m, neo_hip_matrix_desc* d)
{
    if (!m || !d) return fail(NEO_HIP_EINVAL, "null handle or descriptor");
    std::memset(d, 0, sizeof *d);
    d->inputs = m->I, d->outputs = m->O, d->block = m->B, d->partitions = m->P;
    d->method = m->ola ? 1 : 0;
    d->fdl_bytes = int64_t(m->I) * m->ring * m->B * int64_t(sizeof(cf));
    if (m->ready) {
        d->routes = m->plan.nroutes, d->tiles = m->plan.ntiles, d->out_tile = m->plan.OT, d->splits = m->plan.S;
        d->fused = m->plan.fused ? 1 : 0;
        d->filter_bytes = int64_t(m->plan.nroutes) * m->P * m->B * int64_t(sizeof(cf));
        d->offline_bytes = matrix_offline_bytes(m);
    }
    return NEO_HIP_OK;
}

}  // extern "C"
