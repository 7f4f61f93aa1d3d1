// upols_matrix_offline.hip — offline windows of the matrix convolver (upols_matrix.hip): the dense
// handle's offline windows (k_off_mac, upols_levels.hip: 256-point transforms along the block axis
// applied to EVERY partition) combined with the matrix handle's saving. Per bin and per window of
// 128 blocks starting at block t_W
//   Y_o[t_W + j] = samples 128 + j of IDFT256( sum over routes (o, i), segments q < nseg of
//                  DFT256(FDL_i rows t_W - 128 (q + 1) ... + 255) . DFT256(h_(o,i),q) )
// so the forward transforms are per INPUT (k_matrix_off_fwd), the inverse transforms per OUTPUT, and
// the only per-route work is nseg pointwise products of 256-point spectra (k_matrix_off_mac).
//   off_hf [routes][nseg][256][B]  the routes' segment spectra (k_lvf_filter, C := routes)
//   off_xf [I][pairs][256][B]      the pass's pair spectra; a PAIR is 256 consecutive ring rows, pair
//                                  k of a pass starts at matrix_offline_pair_row (matrix_plan.hpp)
//   off_y  [O][128 WP][B]          the windows' output spectra, block by block (one slab of
//                                  k_batch_finish)
// Both kernels hold a 16-column unit in col_fft's layout: lane (a, cp) has f = a + 16 i of column
// cp; the unit with column 0 keeps packed bin 0 (DC, Nyquist) in the real-FFT packing (upols_far.hpp).
#include "matrix_plan.hpp"
#include "upols_far.hpp"

namespace neo_hip {

// pair spectra: the default cache policy (every output of a unit re-reads them: L2 / Infinity Cache)
__device__ __forceinline__ cf buf_ld_cached(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    return __builtin_bit_cast(cf, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}

// grid I x pairs x B/16: pair k of input i -> its 256-point spectrum (packed bin 0 in unit 0)
__global__ __launch_bounds__(256) void k_matrix_off_fwd(const cf* __restrict__ fdl, cf* __restrict__ xf,
                                                        const cf* __restrict__ twf, int B, int ring, int npairs, int wp,
                                                        int w)
{
    __shared__ cf lds[16 * 16 * 16];  // col_fft transposes
    __shared__ cf z[kFN];              // bin-0 exchange
    __shared__ cf tws[kFN];
    const int t = threadIdx.x, a = t >> 4, cp = t & 15;
    const int gpc = B / 16, g = blockIdx.x % gpc, ik = blockIdx.x / gpc, k = ik % npairs, i = ik / npairs;
    const int rowbytes = B * int(sizeof(cf)), ko = (g * 16 + cp) * int(sizeof(cf));
    tws[t] = twf[t];
    // an input's ring spans < 2 GiB (neo_hip_matrix_set_offline)
    const __amdgpu_buffer_rsrc_t fres = buf_rsrc(fdl + int64_t(i) * ring * B, int64_t(ring) * rowbytes);
    const int r0 = matrix_offline_pair_row(w, wp, k, ring) + a;  // ring > 256: one wrap at most
    cf x[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) {
        const int r = r0 + 16 * n;
        x[n] = buf_ld(fres, (r >= ring ? r - ring : r) * rowbytes + ko, 0);
    }
    __syncthreads();  // twiddles
    col_fft<-1, 16>(x, lds, tws, a, cp, true);
    if (g == 0) bin0_exchange<true>(x, z, a, cp);  // uniform per workgroup
    const __amdgpu_buffer_rsrc_t ores = buf_rsrc(xf + int64_t(ik) * kFN * B, int64_t(kFN) * rowbytes);
#pragma unroll
    for (int m = 0; m < 16; ++m) buf_st(x[m], ores, a * rowbytes + ko, 16 * m * rowbytes);
}

// grid O x B/16: output o's routes in ascending input order x segments 0 .. nseg - 1, WP windows
// sharing every spectrum load; tab = off [O + 1], then per list entry {input, route}
template<int WP>
__global__ __launch_bounds__(256) void k_matrix_off_mac(const cf* __restrict__ xf, const cf* __restrict__ hf,
                                                        cf* __restrict__ y, const cf* __restrict__ twf,
                                                        const int* __restrict__ tab, int O, int B, int nseg, int64_t hcs)
{
    __shared__ cf lds[16 * 16 * 16];  // col_fft transposes
    __shared__ cf z[kFN];              // bin-0 exchange
    __shared__ cf tws[kFN];
    const int t = threadIdx.x, a = t >> 4, cp = t & 15;
    const int gpc = B / 16, o = blockIdx.x / gpc, g = blockIdx.x - o * gpc;
    const bool unit0 = g == 0;  // uniform per workgroup: the unit holding packed bin 0
    const int rowbytes = B * int(sizeof(cf)), spec = kFN * rowbytes;
    const int vo = a * rowbytes + (g * 16 + cp) * int(sizeof(cf));
    const int npairs = nseg + WP - 1;
    tws[t] = twf[t];
    auto z0 = [&](int i) { return unit0 && cp == 0 && ((a + 16 * i) & (kFN / 2 - 1)) == 0; };
    auto load = [&]<bool NT>(cf* dst, const cf* base) {
        const __amdgpu_buffer_rsrc_t res = buf_rsrc(base, spec);
#pragma unroll
        for (int i = 0; i < 16; ++i) dst[i] = NT ? buf_ld(res, vo, 16 * i * rowbytes) : buf_ld_cached(res, vo, 16 * i * rowbytes);
    };
    f2v acc[WP][16];
#pragma unroll
    for (int w = 0; w < WP; ++w)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[w][i] = f2v(0.f);
    const int* list = tab + O + 1;
    for (int e = tab[o]; e < tab[o + 1]; ++e) {  // uniform per workgroup
        const cf* xi = xf + int64_t(list[2 * e]) * npairs * kFN * B;
        const cf* hr = hf + int64_t(list[2 * e + 1]) * hcs;
        // window 1's pair of segment q is window 0's pair of segment q - 1
        cf xp[WP > 1 ? 16 : 1];
        if constexpr (WP > 1) load.template operator()<false>(xp, xi);
        for (int q = 0; q < nseg; ++q) {
            cf hv[16], x[16];
            load.template operator()<true>(hv, hr + int64_t(q) * kFN * B);
            load.template operator()<false>(x, xi + int64_t(matrix_offline_pair_of(WP, 0, q)) * kFN * B);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const pk_coef h(hv[i], z0(i));
                h.mac(acc[0][i], x[i]);
                if constexpr (WP > 1) h.mac(acc[1][i], xp[i]);
            }
            if constexpr (WP > 1) {
#pragma unroll
                for (int i = 0; i < 16; ++i) xp[i] = x[i];
            }
        }
    }
    constexpr float sc = 1.0f / kFN;
#pragma unroll
    for (int w = 0; w < WP; ++w) {
        cf v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = cf{acc[w][i].x, acc[w][i].y};
        __syncthreads();  // twiddles; the window before's reads of z / lds are done
        if (unit0) bin0_exchange<false>(v, z, a, cp);  // uniform per workgroup
        col_fft<1, 16>(v, lds, tws, a, cp, true);
        const __amdgpu_buffer_rsrc_t ores =
            buf_rsrc(y + (int64_t(o) * WP + w) * kFarT * B, int64_t(kFarT) * rowbytes);
#pragma unroll
        for (int m = 8; m < 16; ++m)  // n = 16 m + a >= 128: block n - 128 of window w
            buf_st(cscale(v[m], sc), ores, vo, 16 * (m - 8) * rowbytes);
    }
}

int launch_matrix_off_fwd(const cf* fdl, cf* xf, const cf* twf, int I, int B, int ring, int npairs, int wp, int w,
                          hipStream_t s)
{
    if (wp < 1 || wp > kMatrixOffMaxWP || npairs < wp || ring <= kFN || w < 0 || w >= ring)
        return fail(NEO_HIP_EINVAL, "matrix offline: %d pairs, %d windows, ring %d, row %d", npairs, wp, ring, w);
    const unsigned grid = unsigned(I) * unsigned(npairs) * unsigned(B / 16);
    hipLaunchKernelGGL(k_matrix_off_fwd, dim3(grid), dim3(256), 0, s, fdl, xf, twf, B, ring, npairs, wp, w);
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

int launch_matrix_off_mac(const cf* xf, const cf* hf, cf* y, const cf* twf, const int* tab, int O, int B, int nseg,
                          int wp, int64_t hcs, hipStream_t s)
{
    const unsigned grid = unsigned(O) * unsigned(B / 16);
    if (wp == 2) hipLaunchKernelGGL(k_matrix_off_mac<2>, dim3(grid), dim3(256), 0, s, xf, hf, y, twf, tab, O, B, nseg, hcs);
    else if (wp == 1) hipLaunchKernelGGL(k_matrix_off_mac<1>, dim3(grid), dim3(256), 0, s, xf, hf, y, twf, tab, O, B, nseg, hcs);
    else return fail(NEO_HIP_EINVAL, "matrix offline: %d windows per pass", wp);
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

}  // namespace neo_hip
