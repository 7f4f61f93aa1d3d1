// upols_matrix_levels.hip — window levels of a matrix convolver (upols_matrix.hip): long filters
// block by block. The block step reads every partition of every route's filter on every block; with
// window levels on (neo_hip_matrix_set_levels) only the head, partitions [0, 2 T0), is read per
// block, and a level with window length T reads its band of partitions [2 T, ...) once per T blocks:
// the batched pass's MAC (upols_matrix_batch.hip) aimed at the NEXT window, whose T partial spectra
// per output and split are summed into the block's output spectrum T blocks later (matrix_plan.hpp,
// "window levels": the schedule, the parts and the ring).
//
//   k_matrix_lvl_mac     k_matrix_batch_mac's walk (matrix_batch_device.hpp) with three additions:
//            first   the grid is a PART, the workgroups [first, first + gridDim) of the level's
//                    O x S x G, so T launches of one window do the work of one batched pass;
//            w       the ring row of block 0 of the future window, (wpos + T - n mod T) mod ring;
//            part    that window's half of the level's double-buffered slabs [2][O][S][T][B].
//            What it keeps: a step past a run's end is skipped with one uniform branch, its loads
//            clamped inside both descriptors; an output without a route in the band has no run and
//            writes zeros; an input reaches only the outputs whose runs hold it; the order of a
//            bin's sum is fixed by the plan; no atomics.
//   k_matrix_lvl_finish  one workgroup per output: the head's slabs (s ascending), then per level (T
//            ascending) row n mod T of the current window's slabs (split ascending), 8 loads in
//            flight, then the c2r tail as k_upols_finish runs it.
#include "matrix_batch_device.hpp"
#include "matrix_plan.hpp"

namespace neo_hip {

// grid: a part of O x S x G (G bin chunks per row), L = min(256, max(64, B)) lanes. tab: run_off
// [nsplit + 1] (nsplit = O S), then the runs, 4 ints each (matrix_level). Registers as
// k_matrix_batch_mac: T accumulator pairs, T window pairs, 2 D prefetch pairs.
template<int L, int T, int D = (T < kMbDepth ? T : kMbDepth)>
__global__ __launch_bounds__(L, 2) void k_matrix_lvl_mac(const cf* __restrict__ H, const cf* __restrict__ fdl,
                                                        cf* __restrict__ part, const int* __restrict__ tab, int B, int P,
                                                        int ring, int w, int nsplit, int first)
{
    const int G = B > L ? B / L : 1;
    const int wg = first + int(blockIdx.x);
    const int os = wg / G, gch = wg - os * G;  // os = o S + s
    if (os >= nsplit) return;                  // (uniform; the launcher never asks for it)
    const int bin = gch * L + threadIdx.x;     // packed bin of this lane
    const int* run_off = tab;
    const int* runs = tab + nsplit + 1;
    const int rowbytes = B * int(sizeof(cf));

    f2v a[T], f[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        a[j] = f2v(0.0f);
        f[j] = f2v(0.0f);
    }
    const int k1 = run_off[os + 1];
    for (int k = run_off[os]; k < k1; ++k) {
        const int i = runs[4 * k], r = runs[4 * k + 1], pa = runs[4 * k + 2], pb = runs[4 * k + 3];
        // a route's filter and an input's ring each span < 2 GiB (make_matrix_plan)
        const mb_src sp{__builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(H + int64_t(r) * P * B), 0, P * rowbytes, 0x00020000),
                        __builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(fdl + int64_t(i) * ring * B), 0, ring * rowbytes,
                                                          0x00020000),
                        bin < B ? bin * int(sizeof(cf)) : kSparseDrop, rowbytes, P, ring, w, bin == 0};
#pragma unroll
        for (int sl = 1; sl < T; ++sl) {  // rows block sl needs at pa (entered at partition pa - sl)
            int row = w + sl - pa;        // in (-P, ring + T): one wrap either way (ring >= P > T)
            row = row < 0 ? row + ring : (row >= ring ? row - ring : row);
            f[sl] = mb_ld(sp.f, sp.voff, row * rowbytes);
        }
        f2v ph[D], pf[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {  // prefetch partitions pa .. pa + D - 1
            const int p = min(pa + d, P - 1);
            pf[d] = mb_ld(sp.f, sp.voff, sp.frow(p) * rowbytes);
            ph[d] = mb_ld(sp.h, sp.voff, p * rowbytes);
        }
        for (int p0 = pa; p0 < pb; p0 += T) mb_chunk<T, D>(a, f, ph, pf, sp, p0, pb, std::make_integer_sequence<int, T>{});
    }

    if (bin < B) {
        cf* slab = part + int64_t(os) * T * B + bin;
#pragma unroll
        for (int j = 0; j < T; ++j) slab[int64_t(j) * B] = cf{a[j].x, a[j].y};
    }
}

// workgroups [wg0, wg1) of a level's grid O x S x G for the window whose block 0 is ring row w
int launch_matrix_lvl_mac(const cf* H, const cf* fdl, cf* part, const int* tab, int B, int P, int ring, int O, int S, int T,
                          int w, int wg0, int wg1, hipStream_t s)
{
    const int L = B < 64 ? 64 : B > 256 ? 256 : B;
    const int nsplit = O * S, nwg = nsplit * matrix_batch_chunks(B);
    if (wg0 < 0 || wg1 > nwg || ring < P || P <= 2 * T || w < 0 || w >= ring)
        return fail(NEO_HIP_EINVAL, "matrix levels: workgroups [%d, %d) of %d, ring %d, P %d, T %d, row %d", wg0, wg1, nwg, ring,
                    P, T, w);
    if (wg0 >= wg1) return NEO_HIP_OK;  // a part without a workgroup
    const unsigned grid = unsigned(wg1 - wg0);
#define NEO_ML_LAUNCH(LL, TT)                                                                                          \
    hipLaunchKernelGGL((k_matrix_lvl_mac<LL, TT>), dim3(grid), dim3(LL), 0, s, H, fdl, part, tab, B, P, ring, w, nsplit, \
                       wg0)
#define NEO_ML_T(TT)                                \
    case TT:                                        \
        if (L == 64) NEO_ML_LAUNCH(64, TT);         \
        else if (L == 128) NEO_ML_LAUNCH(128, TT);  \
        else NEO_ML_LAUNCH(256, TT);                \
        break;
    switch (T) {
        NEO_ML_T(2)
        NEO_ML_T(4)
        NEO_ML_T(8)
        NEO_ML_T(16)
        NEO_ML_T(32)
        default: return fail(NEO_HIP_EINVAL, "window of %d blocks not available", T);
    }
#undef NEO_ML_T
#undef NEO_ML_LAUNCH
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

// one workgroup per output: head slabs [O][Sh][B], then the levels' rows; X = the block's spectrum
template<int B, bool OLA>
__global__ __launch_bounds__(256) void k_matrix_lvl_finish(const cf* __restrict__ head, int Sh, matrix_lvl_rows lv,
                                                           float* __restrict__ out, int64_t ld_out,
                                                           float* __restrict__ ovl, const cf* __restrict__ twg)
{
    using K = upols_cfg<B>;
    __shared__ __attribute__((aligned(16))) cf X[B];
    __shared__ cf fft[K::LL];
    __shared__ cf tw[K::TW1 + K::TW2];
    const int tid = threadIdx.x, o = blockIdx.x;
    for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];
    for (int q = tid; q < K::Q; q += 256) {
        float4 sum = {0.f, 0.f, 0.f, 0.f};
        // n rows of `stride` float4 apart, in order, 8 loads in flight
        auto add = [&](const float4* p4, int n, int64_t stride) {
            int t = 0;
            for (; t + 7 < n; t += 8) {
                float4 r[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) r[u] = p4[(t + u) * stride + q];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    sum.x += r[u].x; sum.y += r[u].y; sum.z += r[u].z; sum.w += r[u].w;
                }
            }
            for (; t < n; ++t) {
                const float4 r = p4[t * stride + q];
                sum.x += r.x; sum.y += r.y; sum.z += r.z; sum.w += r.w;
            }
        };
        add(reinterpret_cast<const float4*>(head + int64_t(o) * Sh * B), Sh, K::Q);
        for (int l = 0; l < lv.n; ++l)  // uniform
            add(reinterpret_cast<const float4*>(lv.row[l] + int64_t(o) * lv.S[l] * lv.T[l] * B), lv.S[l], int64_t(lv.T[l]) * K::Q);
        reinterpret_cast<float4*>(X)[q] = sum;
    }
    __syncthreads();
    c2r_tail<B, OLA, NEO_FINISH_E(B)>(X, fft, tw, out + int64_t(o) * ld_out, ovl + int64_t(o) * B, tid);
}

int launch_matrix_lvl_finish(int O, int B, bool ola, const cf* head, int Sh, const matrix_lvl_rows& lv, float* out,
                             int64_t ld_out, float* ovl, const cf* tw, hipStream_t s)
{
    if (lv.n < 0 || lv.n > kMatrixMaxLevels || Sh < 1) return fail(NEO_HIP_EINVAL, "matrix levels: %d levels, %d head slabs", lv.n, Sh);
    NEO_UPOLS_DISPATCH_OLA(B, ola, hipLaunchKernelGGL((k_matrix_lvl_finish<BB, OL>), dim3(unsigned(O)), dim3(256), 0, s, head, Sh,
                                                      lv, out, ld_out, ovl, tw))
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

}  // namespace neo_hip
