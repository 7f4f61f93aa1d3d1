// matrix_batch_device.hpp — the walk of the matrix convolver's batched MAC, shared by its two kernels:
// k_matrix_batch_mac (upols_matrix_batch.hip: T blocks of a call at the write position) and
// k_matrix_lvl_mac (upols_matrix_levels.hip: the T blocks of a future window over a band of partitions).
#pragma once

#include "upols_handle.hpp"
#include "upols_step.hpp"

#include <utility>

namespace neo_hip {

constexpr int kMbDepth = 8;  // rows in flight per lane (divides or exceeds every T)

// what a run reads: the input's ring, the route's filter, the lane's place in a row
struct mb_src {
    __amdgpu_buffer_rsrc_t h, f;
    int voff;      // the lane's byte offset in a row; kSparseDrop for a lane past the row (B < lanes)
    int rowbytes;
    int P, ring, w;
    bool bin0;
    // FDL row of partition p for block 0 (p < P <= ring)
    __device__ __forceinline__ int frow(int p) const
    {
        const int r = w - p;
        return r < 0 ? r + ring : r;
    }
};

__device__ __forceinline__ f2v mb_ld(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    const auto u = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
    return __builtin_bit_cast(f2v, u);
}

// a += h x and a += h x.yx as one v_pk_fma_f32 each, the accumulator tied to its register: under
// the uniform branch of mb_step the builtin form keeps the accumulators twice (upols_sparse_batch.hip)
__device__ __forceinline__ void mb_fma(f2v& a, f2v h, f2v x)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a) : "v"(h), "v"(x));
}
__device__ __forceinline__ void mb_fma_yx(f2v& a, f2v h, f2v x)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,0,1]" : "+v"(a) : "v"(h), "v"(x));
}

// Step U of a T-step chunk (p = pb0 + U, U static): FDL row (w - p) and filter row p from prefetch
// slot U mod D, the FDL row into window slot (T - U) mod T, the loads of partition p + D issued
// (clamped to P - 1: inside both descriptors), then the MACs of all T blocks if p is in the run;
// block j reads window slot (j - U) mod T. (re, im) += (hr, hr)(xr, xi) + (-hi, hi)(xi, xr); the
// lane of the packed bin 0 takes (hr, hi) and (0, 0), so DC and Nyquist stay two real products.
template<int T, int D, int U>
__device__ __forceinline__ void mb_step(f2v (&a)[T], f2v (&f)[T], f2v (&ph)[D], f2v (&pf)[D], const mb_src& sp, int p,
                                        int pend)
{
    constexpr int slot = U % D;
    f[(T - U) % T] = pf[slot];
    const f2v hv = ph[slot];
    {
        const int pn = min(p + D, sp.P - 1);
        pf[slot] = mb_ld(sp.f, sp.voff, sp.frow(pn) * sp.rowbytes);
        ph[slot] = mb_ld(sp.h, sp.voff, pn * sp.rowbytes);
    }
    if (p < pend) {  // uniform
        const float hr = hv.x, hi = hv.y;
        const float s = sp.bin0 ? 0.0f : hi;
        const f2v h1 = {hr, sp.bin0 ? hi : hr}, h2 = {-s, s};
        // two sweeps over the blocks, so consecutive FMAs never chain on one accumulator
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const f2v x = f[(j - U + T) % T];
                if (k == 0) mb_fma(a[j], h1, x);
                else mb_fma_yx(a[j], h2, x);
            }
    }
    __builtin_amdgcn_sched_barrier(0);  // keep each step's loads D steps ahead, not all hoisted
}

template<int T, int D, int... U>
__device__ __forceinline__ void mb_chunk(f2v (&a)[T], f2v (&f)[T], f2v (&ph)[D], f2v (&pf)[D], const mb_src& sp, int p0,
                                         int pend, std::integer_sequence<int, U...>)
{
    (mb_step<T, D, U>(a, f, ph, pf, sp, p0 + U, pend), ...);
}

}  // namespace neo_hip
