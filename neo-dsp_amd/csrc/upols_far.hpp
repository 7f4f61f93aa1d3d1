// upols_far.hpp — device helpers of the 256-point transforms along the block axis, shared by the
// far level and the offline windows of dense handles (upols_levels.hip) and the offline windows of
// matrix handles (upols_matrix_offline.hip): the column transform, the packed complex MAC, the
// real-FFT packing of bin 0, buffer loads and stores.
#pragma once

#include "upols_device.hpp"
#include "upols_handle.hpp"

namespace neo_hip {

// kFN (the transform length) and the padded strides of the level buffers (slab_cs, ff_cs, spec_cs):
// levels_plan.hpp

// 256-point transforms of NC columns held by lanes (a, cp), a < 16, cp < NC: on entry
// v[n2] = x[a + 16 n2], on exit v[k1] = X[16 k1 + a] (16-point DFTs in registers, twiddle,
// LDS transpose, 16-point DFTs). Every lane of the workgroup calls it (barriers inside);
// lanes with active = false only take part in the barriers.
template<int DIR, int NC>
__device__ __forceinline__ void col_fft(cf (&v)[16], cf* lds, const cf* tw, int a, int cp, bool active)
{
    if (active) {
        dft<16, DIR>(v);
#pragma unroll
        for (int k = 1; k < 16; ++k) v[k] = cmul(v[k], twiddle<kFN, DIR>(tw, a * k));
#pragma unroll
        for (int k = 0; k < 16; ++k) lds[(k * 16 + a) * NC + cp] = v[k];
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int n = 0; n < 16; ++n) v[n] = lds[(a * 16 + n) * NC + cp];
    }
    __syncthreads();
    if (active) dft<16, DIR>(v);
}

// packed complex MAC: acc = (re, im) += h x as (hr, hr)(xr, xi) + (-hi, hi)(xi, xr), two
// v_pk_fma_f32; the packed bin 0 (DC, Nyquist: two real products) takes (hr, hi)(xr, xi)
struct pk_coef {
    f2v h1, h2;
    __device__ __forceinline__ pk_coef(cf h, bool bin0)
    {
        const float s = bin0 ? 0.f : h.y;
        h1 = f2v{h.x, bin0 ? h.y : h.x};
        h2 = f2v{-s, s};
    }
    __device__ __forceinline__ void mac(f2v& acc, cf x) const
    {
        const f2v xv = {x.x, x.y};
        acc = __builtin_elementwise_fma(h1, xv, acc);
        acc = __builtin_elementwise_fma(h2, xv.yx, acc);
    }
};

// buffer loads / stores: 32-bit lane offsets, uniform offsets in SGPRs (fewer VGPRs than
// 64-bit addresses); offsets past the size read 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, int64_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, int(bytes), 0x00020000);
}

__device__ __forceinline__ cf buf_ld(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    return __builtin_bit_cast(cf, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 2 /* streaming */));
}

__device__ __forceinline__ void buf_st(cf v, __amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    typedef unsigned u2v __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, v), r, voff, soff, 0);
}

// Packed bin 0 holds two real sequences (DC and Nyquist): its spectra along the block axis are
// stored packed the real-FFT way, W[f] = X_dc[f] (f <= 128) and W[256 - f] = X_ny[f]
// (0 < f < 128), with W[0] = (X_dc[0], X_ny[0]) and W[128] = (X_dc[128], X_ny[128]) real pairs.

// Z = DFT(x_dc + i x_ny) -> packed W (real-FFT packing of X_dc, X_ny) at f, from Z[f], Z[-f]
__device__ __forceinline__ cf pack_bin0(cf zf, cf zm, int f)
{
    if (f == 0 || f == kFN / 2) return zf;  // (Re, Im) = (X_dc, X_ny), both real here
    if (f < kFN / 2) return cscale(cadd(zf, cconj(zm)), 0.5f);  // X_dc[f]
    const cf d = csub(zm, cconj(zf));                            // f > 128: X_ny[256 - f] = (Z[-f] - conj Z[f]) / 2i
    return cf{0.5f * d.y, -0.5f * d.x};
}

// packed W of bin 0 -> Y = Y_dc + i Y_ny at f, from W[f], W[-f]
__device__ __forceinline__ cf unpack_bin0(cf wf, cf wm, int f)
{
    if (f == 0 || f == kFN / 2) return wf;
    // f < 128: Y_dc[f] + i Y_ny[f] = W[f] + i W[256 - f]; f > 128: conj(W[256 - f]) + i conj(W[f])
    const cf dc = f < kFN / 2 ? wf : cconj(wm);
    const cf ny = f < kFN / 2 ? wm : cconj(wf);
    return cf{dc.x - ny.y, dc.y + ny.x};
}

// bin 0 (column 0, lanes cp == 0) of a spectrum held with v[i] at f = a + 16 i: pack or unpack
// through LDS z; every lane calls (barrier inside)
template<bool PACK>
__device__ __forceinline__ void bin0_exchange(cf (&v)[16], cf* z, int a, int cp)
{
    if (cp == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) z[a + 16 * i] = v[i];
    }
    __syncthreads();
    if (cp == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int f = a + 16 * i;
            const cf m = z[(kFN - f) & (kFN - 1)];
            v[i] = PACK ? pack_bin0(v[i], m, f) : unpack_bin0(v[i], m, f);
        }
    }
}

}  // namespace neo_hip
