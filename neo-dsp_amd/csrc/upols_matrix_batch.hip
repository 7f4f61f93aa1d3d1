// upols_matrix_batch.hip — the MAC of a batched pass of a matrix convolver (upols_matrix.hip): T
// consecutive blocks share ONE pass over every route's filter.
//
// The scheme is k_batch_mac's A2 form (upols_batch.hip): a lane owns one packed bin, keeps T complex
// accumulators and a sliding window of T FDL rows in registers, a prefetch ring of D rows runs
// ahead, and each complex product is two v_pk_fma_f32. Block j of the pass is FDL row (w + j) mod R
// of its input's ring (R >= P + T - 1) and reads rows (w + j - p) mod R.
//
// What differs:
//   one output per workgroup   workgroup (o, s, bin chunk) walks split s of output o's row list
//            (matrix_plan.hpp: the output's inputs ascending x partitions, flattened) and writes T
//            partial spectra to part[o][s][j][B]. The accumulators persist across the inputs: the
//            sum over the inputs is taken on spectra.
//   runs     a split is a list of runs (input, route, partitions [pa, pb)). At a run's start the
//            descriptors of the input's ring and of the route's filter are built, the T - 1 window
//            rows for pa are reloaded and the prefetch restarts.
//   the end  a step with p >= pb (the last chunk of a run, P no multiple of T, P < T) is skipped
//            with one uniform branch, not multiplied by zero: the filter has no zero rows behind P
//            and the ring holds rows older than the filter reaches, whose Inf or NaN must not come
//            back. The loads of such steps are clamped to row P - 1 and their values never used.
//   no route an output without one has no run and writes zeros; an input reaches only the outputs
//            whose row lists hold it.
// The order of a bin's sum is fixed by (T, the plan); there are no atomics: equal calls give equal
// bits, and a route list in another order gives the same plan, hence the same bits.
#include "matrix_batch_device.hpp"
#include "matrix_plan.hpp"

namespace neo_hip {

// grid O x S x G (G = max(1, B / L) bin chunks per row), L = min(256, max(64, B)) lanes; below
// B = 64 the lanes past the row load nothing and store nothing. tab: run_off [O S + 1], then the
// runs, 4 ints each (matrix_batch_plan). 2 waves per SIMD: T accumulator pairs, T window pairs, 2 D
// prefetch pairs; B enters through G only, so the kernel is instantiated per (L, T).
template<int L, int T, int D = (T < kMbDepth ? T : kMbDepth)>
__global__ __launch_bounds__(L, 2) void k_matrix_batch_mac(const cf* __restrict__ H, const cf* __restrict__ fdl,
                                                          cf* __restrict__ part, const int* __restrict__ tab, int B,
                                                          int P, int ring, int w)
{
    const int G = B > L ? B / L : 1;
    const int os = blockIdx.x / G, gch = blockIdx.x - os * G;  // os = o S + s
    const int nsplit = gridDim.x / G;
    const int bin = gch * L + threadIdx.x;  // packed bin of this lane
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
        // a route's filter and an input's ring each span < 2 GiB (make_matrix_batch_plan)
        const mb_src sp{__builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(H + int64_t(r) * P * B), 0, P * rowbytes, 0x00020000),
                        __builtin_amdgcn_make_buffer_rsrc(const_cast<cf*>(fdl + int64_t(i) * ring * B), 0, ring * rowbytes,
                                                          0x00020000),
                        bin < B ? bin * int(sizeof(cf)) : kSparseDrop, rowbytes, P, ring, w, bin == 0};
#pragma unroll
        for (int sl = 1; sl < T; ++sl) {  // rows block sl needs at pa (entered at partition pa - sl)
            int row = w + sl - pa;        // in (-P, ring + T): one wrap either way (ring >= T)
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

int launch_matrix_batch_mac(const cf* H, const cf* fdl, cf* part, const int* tab, int B, int P, int ring, int O, int Sb,
                            int T, int w, hipStream_t s)
{
    const int L = B < 64 ? 64 : B > 256 ? 256 : B;
    if (ring < P + T - 1 || ring < T) return fail(NEO_HIP_EINVAL, "matrix batch: ring of %d rows for P %d, T %d", ring, P, T);
    const unsigned grid = unsigned(O) * unsigned(Sb) * unsigned(matrix_batch_chunks(B));
#define NEO_MB_LAUNCH(LL, TT) \
    hipLaunchKernelGGL((k_matrix_batch_mac<LL, TT>), dim3(grid), dim3(LL), 0, s, H, fdl, part, tab, B, P, ring, w)
#define NEO_MB_T(TT)                                \
    case TT:                                        \
        if (L == 64) NEO_MB_LAUNCH(64, TT);         \
        else if (L == 128) NEO_MB_LAUNCH(128, TT);  \
        else NEO_MB_LAUNCH(256, TT);                \
        break;
    switch (T) {
        NEO_MB_T(2)
        NEO_MB_T(4)
        NEO_MB_T(8)
        NEO_MB_T(16)
        NEO_MB_T(32)
        default: return fail(NEO_HIP_EINVAL, "batch of %d blocks not available", T);
    }
#undef NEO_MB_T
#undef NEO_MB_LAUNCH
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

}  // namespace neo_hip
