// upols_f64.hip — double-precision UPOLS / UPOLA convolvers (neo_hip_upols64): C instances of the
// reference's upols_convolver<complex<double>> / upola_convolver<complex<double>>
// (uniform_partitioned_convolver.hpp:13-65 over overlap_save.hpp:84-112 / overlap_add.hpp:76-106 with
// Float = double), and the setup path in double (uniform_partition.hpp:12-26,
// normalize_impulse.hpp:11-33). A handle type of its own: no float path is touched.
//   cfg64                     per-B geometry (upols_f64_handle.hpp, with the handle itself)
//   k_upols64_step            launch 1, grid C x S: split 0 window r2c + FDL insert; every split its MAC
//   k_upols64_finish          launch 2, one workgroup per channel: slabs in order, c2r, output
//   k_partition64, k_pack64   IR -> filter rows; reference layout [C][P][B+1] -> packed rows
//   k_energy64, k_scale_min64 normalize_impulse
//   neo_hip_upols64           the handle; the plan is an upols64_shape (upols_f64_plan.hpp, host only)
// A block is the plain two-launch step: no last-arriver fusion, no atomics; equal calls give equal bits.
// With batching on (neo_hip_upols64_set_batch, upols_f64_batch.hip) a call's whole passes of T blocks
// go first and its remainder runs as plain steps, on the same ring and prev; with offline windows on
// (neo_hip_upols64_set_offline, upols_f64_offline.hip) its whole windows of 128 blocks go before both.
#include "upols_f64_handle.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

namespace neo_hip {

struct acc4d {  // 4 partial products per bin keep the packed bin 0 exact (DC and Nyquist are real products)
    double rr, ii, ri, ir;
};
__device__ __forceinline__ void mac1(acc4d& a, cd h, cd x)
{
    a.rr = fma(h.x, x.x, a.rr);
    a.ii = fma(h.y, x.y, a.ii);
    a.ri = fma(h.x, x.y, a.ri);
    a.ir = fma(h.y, x.x, a.ir);
}
__device__ __forceinline__ cd finish64(const acc4d& a, bool bin0)
{
    return bin0 ? cd{a.rr, a.ii} : cd{a.rr - a.ii, a.ri + a.ir};
}

// Workgroup (c, s) accumulates partitions [s rows, min(P, (s + 1) rows)) of channel c into slab
// [c][s], ascending p per lane. Split 0 first builds the window (overlap-save: prev | block, then
// the block becomes prev; overlap-add: block | zeros), runs the B-point complex Stockham and the r2c
// split in LDS, stores the spectrum as FDL row w and uses it from registers for p = 0. Rows
// (w - p) mod P, p >= 1, are other rows of the ring, so no split reads what split 0 writes.
template<int B, bool OLA>
__global__ __launch_bounds__(256) void k_upols64_step(const double* __restrict__ in, int64_t ld_in,
                                                      double* __restrict__ prev, const cd* __restrict__ H,
                                                      cd* __restrict__ fdl, cd* __restrict__ part,
                                                      const cd* __restrict__ twg, int P, int S, int rows, int w)
{
    using K = cfg64<B>;
    __shared__ cd fft[K::LL];
    __shared__ cd tw[K::TW1 + K::TW2];
    __shared__ acc4d red[K::RPI > 1 ? 256 : 1];
    const int tid = threadIdx.x, c = blockIdx.x, s = blockIdx.y;
    const int p0 = s * rows, p1 = min(P, p0 + rows);
    const int64_t crow = int64_t(c) * P * B;  // channel base in H / FDL (complex units)

    if (s == 0) {
        constexpr int E = K::EW, T = B / E;
        static_assert(T <= 256 && B % E == 0, "window FFT must fit one 256-lane workgroup");
        const bool active = tid < T;
        for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];
        const cd* iz = reinterpret_cast<const cd*>(in + int64_t(c) * ld_in);  // z[n] = w[2n] + i w[2n+1]
        cd* pz = reinterpret_cast<cd*>(prev + int64_t(c) * B);
        cd v[E];
        if (active) {
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int n = tid + m * T;
                if constexpr (OLA) v[m] = n < B / 2 ? iz[n] : cd{0.0, 0.0};
                else v[m] = n < B / 2 ? pz[n] : iz[n - B / 2];
            }
        }
        __syncthreads();
        stockham<B, E, -1>(v, fft, tw, tid, active);
        if (active) {
#pragma unroll
            for (int m = 0; m < E; ++m) fft[lpad(tid + m * T)] = v[m];
        }
        __syncthreads();
        if constexpr (!OLA) {  // every lane's reads of prev lie before the barriers above
            for (int i = tid; i < B / 2; i += 256) pz[i] = iz[i];
        }
    }

    const int rs = tid / K::QT, q0 = tid - rs * K::QT;
    const cd* Hc = H + crow;
    cd* Fc = fdl + crow;
    cd* slab = part + (int64_t(c) * S + s) * B;
#pragma unroll 1
    for (int ch = 0; ch < K::NCH; ++ch) {
        const int qb = ch * K::QT * K::VPT + q0;  // this lane's bins: qb + v QT
        acc4d a[K::VPT];
#pragma unroll
        for (int v = 0; v < K::VPT; ++v) a[v] = {0.0, 0.0, 0.0, 0.0};
        int pstart = p0;
        if (s == 0) {  // p = 0: the fresh spectrum, from LDS through registers into row w and the MAC
            if (rs == 0) {
#pragma unroll
                for (int v = 0; v < K::VPT; ++v) {
                    const int q = qb + v * K::QT;
                    const cd x = r2c_split<B>(fft, tw + K::TW1, q);
                    Fc[int64_t(w) * B + q] = x;
                    mac1(a[v], Hc[q], x);
                }
            }
            pstart = 1;
        }
        int p = pstart + rs;
        for (; p + (K::U - 1) * K::RPI < p1; p += K::U * K::RPI) {
            cd hv[K::U][K::VPT], xv[K::U][K::VPT];
#pragma unroll
            for (int u = 0; u < K::U; ++u) {
                const int pp = p + u * K::RPI;
                const int fr = w >= pp ? w - pp : w - pp + P;  // fdl_index.hpp:28-31 ring
#pragma unroll
                for (int v = 0; v < K::VPT; ++v) {
                    const int q = qb + v * K::QT;
                    hv[u][v] = Hc[int64_t(pp) * B + q];
                    xv[u][v] = ld_nt(Fc + int64_t(fr) * B + q);
                }
            }
#pragma unroll
            for (int u = 0; u < K::U; ++u)
#pragma unroll
                for (int v = 0; v < K::VPT; ++v) mac1(a[v], hv[u][v], xv[u][v]);
        }
        for (; p < p1; p += K::RPI) {
            const int fr = w >= p ? w - p : w - p + P;
#pragma unroll
            for (int v = 0; v < K::VPT; ++v) {
                const int q = qb + v * K::QT;
                mac1(a[v], Hc[int64_t(p) * B + q], ld_nt(Fc + int64_t(fr) * B + q));
            }
        }
        if constexpr (K::RPI > 1) {  // fold the row groups into group 0, fixed order
            red[tid] = a[0];
            __syncthreads();
            if (rs == 0) {
                for (int g = 1; g < K::RPI; ++g) {
                    const acc4d r = red[g * K::QT + q0];
                    a[0].rr += r.rr; a[0].ii += r.ii; a[0].ri += r.ri; a[0].ir += r.ir;
                }
            }
        }
        if (rs == 0) {
#pragma unroll
            for (int v = 0; v < K::VPT; ++v) {
                const int q = qb + v * K::QT;
                slab[q] = finish64(a[v], q == 0);
            }
        }
    }
}

// One workgroup per channel: the S slabs summed in the order s = 0..S-1, the c2r join, the inverse
// Stockham, the double scale 1/(2B) (overlap_save.hpp:107-108 / overlap_add.hpp:98) and the output
// (overlap-save: window samples [B, 2B); overlap-add: [0, B) + tail, [B, 2B) is the new tail). The
// summed spectrum lies in the transform's own LDS tile (unpadded) until every lane has joined its
// elements, so B = 4096 takes 68 KiB + twiddles.
template<int B, bool OLA>
__global__ __launch_bounds__(256) void k_upols64_finish(const cd* __restrict__ part, double* __restrict__ out,
                                                        int64_t ld_out, double* __restrict__ ovl,
                                                        const cd* __restrict__ twg, int S)
{
    using K = cfg64<B>;
    constexpr int E = K::EF, T = B / E;
    static_assert(T <= 256 && B % E == 0, "c2r must fit one 256-lane workgroup");
    __shared__ cd fft[K::LL];
    __shared__ cd tw[K::TW1 + K::TW2];
    const int tid = threadIdx.x, c = blockIdx.x;
    for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];
    const cd* pc = part + int64_t(c) * S * B;
    for (int k = tid; k < B; k += 256) {
        cd sum = pc[k];
        int t = 1;
        for (; t + 3 < S; t += 4) {
            cd r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = pc[int64_t(t + u) * B + k];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                sum.x += r[u].x;
                sum.y += r[u].y;
            }
        }
        for (; t < S; ++t) {
            const cd r = pc[int64_t(t) * B + k];
            sum.x += r.x;
            sum.y += r.y;
        }
        fft[k] = sum;
    }
    __syncthreads();
    const bool active = tid < T;
    cd v[E];
    if (active) {
        const cd x0 = fft[0];
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int k = tid + m * T;
            v[m] = k == 0 ? c2r_join<B>(cd{x0.x, 0.0}, cd{x0.y, 0.0}, tw + K::TW1, 0)
                          : c2r_join<B>(fft[k], fft[B - k], tw + K::TW1, k);
        }
    }
    __syncthreads();  // the spectrum is in registers: the tile is the transform's from here
    stockham<B, E, +1>(v, fft, tw, tid, active);
    if (active) {
        const double scale = 1.0 / double(2 * B);
        cd* o = reinterpret_cast<cd*>(out + int64_t(c) * ld_out);
        if constexpr (OLA) {
            cd* ov = reinterpret_cast<cd*>(ovl + int64_t(c) * B);
            // the same lane reads overlap[n] (m < E/2) before writing it (m >= E/2: n - B/2)
#pragma unroll
            for (int m = 0; m < E / 2; ++m) {
                const int n = tid + m * T;
                const cd old = ov[n];
                o[n] = cd{v[m].x * scale + old.x, v[m].y * scale + old.y};
            }
#pragma unroll
            for (int m = E / 2; m < E; ++m) {
                const int n = tid + m * T;
                ov[n - B / 2] = cd{v[m].x * scale, v[m].y * scale};
            }
        } else {
#pragma unroll
            for (int m = E / 2; m < E; ++m) {
                const int n = tid + m * T;
                o[n - B / 2] = cd{v[m].x * scale, v[m].y * scale};
            }
        }
    }
}

// uniform_partition in double (uniform_partition.hpp:12-26 -> stft.hpp:56-99): partition p of channel
// c = rfft_2B(ir[c][pB : pB + B] zero-padded to 2B), straight into packed rows [C][P][B] (a handle's
// filter) or unpacked [C][P][B + 1] (the reference's layout).
template<int B, bool PACKED>
__global__ __launch_bounds__(256) void k_partition64(const double* __restrict__ ir, int64_t L, int P,
                                                     cd* __restrict__ out, const cd* __restrict__ twg)
{
    using K = cfg64<B>;
    constexpr int E = K::EW, T = B / E;
    __shared__ cd fft[K::LL];
    __shared__ cd tw[K::TW1 + K::TW2];
    const int tid = threadIdx.x;
    const int64_t cp = blockIdx.x;
    const int64_t c = cp / P, p = cp - c * P;
    for (int i = tid; i < K::TW1 + K::TW2; i += 256) tw[i] = twg[i];
    const bool active = tid < T;
    const double* seg = ir + c * L + p * B;
    const int64_t cnt = min(int64_t(B), L - p * B);
    cd v[E];
    if (active) {
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int n = tid + m * T;  // z[n] = (w[2n], w[2n+1]); w = segment | zeros
            const double a = 2 * n < cnt ? seg[2 * n] : 0.0;
            const double b = 2 * n + 1 < cnt ? seg[2 * n + 1] : 0.0;
            v[m] = {a, b};
        }
    }
    __syncthreads();
    stockham<B, E, -1>(v, fft, tw, tid, active);
    if (active) {
#pragma unroll
        for (int m = 0; m < E; ++m) fft[lpad(tid + m * T)] = v[m];
    }
    __syncthreads();
    cd* row = out + cp * (PACKED ? B : B + 1);
    for (int k = tid; k < B; k += 256) {
        const cd x = r2c_split<B>(fft, tw + K::TW1, k);
        if (PACKED || k != 0) {
            row[k] = x;
        } else {
            row[0] = {x.x, 0.0};
            row[B] = {x.y, 0.0};
        }
    }
}

// filter [C][P][B+1] (reference layout) -> packed [C][P][B]
__global__ void k_pack64(const cd* __restrict__ in, cd* __restrict__ out, int B, int64_t rows)
{
    const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= rows * B) return;
    const int64_t r = gid / B, k = gid - r * B;
    const cd* src = in + r * (B + 1);
    out[gid] = k == 0 ? cd{src[0].x, src[B].x} : src[k];
}

// normalize_energy_factor (normalize_energy.hpp:17-44) in double, one workgroup per channel: lane t
// sums x^2 over i = t, t + 256, ... in that order, then the 256 partial sums fold as a fixed tree.
// The order depends on L alone, never on the launch; it is not the reference's sequential order
// (the two differ near 1e-13 relative, far below the 1e-12 bar).
__global__ __launch_bounds__(256) void k_energy64(const double* __restrict__ ir, int64_t L, double* __restrict__ factor)
{
    __shared__ double part[256];
    const int t = threadIdx.x;
    const double* x = ir + int64_t(blockIdx.x) * L;
    double e = 0.0;
    for (int64_t i = t; i < L; i += 256) e = fma(x[i], x[i], e);
    part[t] = e;
    __syncthreads();
    for (int h = 128; h >= 1; h /= 2) {
        if (t < h) part[t] += part[t + h];
        __syncthreads();
    }
    if (t == 0) factor[blockIdx.x] = part[0] == 0.0 ? 1.0 : 1.0 / sqrt(part[0]);
}

// normalize_impulse.hpp:21-30: min factor over channels, then scale everything
__global__ void k_scale_min64(double* __restrict__ ir, int64_t n, const double* __restrict__ factor, int C)
{
    __shared__ double fmin_s;
    if (threadIdx.x == 0) {
        double f = factor[0];
        for (int c = 1; c < C; ++c) f = fmin(f, factor[c]);
        fmin_s = f;
    }
    __syncthreads();
    const double f = fmin_s;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
        ir[i] = ir[i] * f;
}

}  // namespace neo_hip

using namespace neo_hip;

namespace neo_hip {

// order a setup call after every step of this handle (the streams its step calls ran on, its own
// stream) and, device_input, after work on the null stream that produced a device-resident input
int setup_join64(neo_hip_upols64* h, bool device_input)
{
    if (int rc = h->used.join()) return rc;
    if (device_input)
        if (int rc = null_join()) return rc;
    NEO_HIP_CHECK(hipStreamSynchronize(h->stream));
    return NEO_HIP_OK;
}

// the double twiddle tables of block B (B-point, then 2B-point) on the current device, shared by every
// handle and setup call there, never freed
int shared_tw64(const cd** out, int B)
{
    static std::mutex mu;
    static std::map<std::pair<int, int>, cd*> tables;
    int dev = 0;
    NEO_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (auto it = tables.find({dev, B}); it != tables.end()) {
        *out = it->second;
        return NEO_HIP_OK;
    }
    std::vector<cd> t = make_twiddle_table<cd>(B);
    const std::vector<cd> t2 = make_twiddle_table<cd>(2 * int64_t(B));
    t.insert(t.end(), t2.begin(), t2.end());
    cd* d = nullptr;
    NEO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d), t.size() * sizeof(cd)));
    NEO_HIP_CHECK(hipMemcpy(d, t.data(), t.size() * sizeof(cd), hipMemcpyHostToDevice));
    tables.emplace(std::make_pair(dev, B), d);
    *out = d;
    return NEO_HIP_OK;
}

}  // namespace neo_hip

namespace {

using upols64_t = neo_hip_upols64;

int partition64(const double* d_ir, int C, int64_t L, int B, bool packed, cd* out, const cd* tw, hipStream_t s)
{
    const int64_t P = partitions_for(L, B);
    const int64_t blocks = int64_t(C) * P;
    if (blocks > 0x7fffffff) return fail(NEO_HIP_EINVAL, "too many partitions");
    if (packed) {
        NEO_UPOLS_DISPATCH(B, hipLaunchKernelGGL((k_partition64<BB, true>), dim3(unsigned(blocks)), dim3(256), 0, s, d_ir,
                                                 L, int(P), out, tw))
    } else {
        NEO_UPOLS_DISPATCH(B, hipLaunchKernelGGL((k_partition64<BB, false>), dim3(unsigned(blocks)), dim3(256), 0, s, d_ir,
                                                 L, int(P), out, tw))
    }
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

// factor: pooled scratch of C doubles, the caller's to give back once s is joined
int normalize64(double* d_ir, int C, int64_t L, double* factor, hipStream_t s)
{
    hipLaunchKernelGGL(k_energy64, dim3(unsigned(C)), dim3(256), 0, s, d_ir, L, factor);
    NEO_HIP_LAUNCH_CHECK();
    const int64_t n = int64_t(C) * L;
    const unsigned blocks = unsigned(std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_scale_min64, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, s, d_ir, n, factor, C);
    NEO_HIP_LAUNCH_CHECK();
    return NEO_HIP_OK;
}

int reset_state64(upols64_t* h, hipStream_t s)
{
    NEO_HIP_CHECK(hipMemsetAsync(h->fdl, 0, size_t(h->shape.fdl_bytes), s));
    NEO_HIP_CHECK(hipMemsetAsync(h->prev, 0, size_t(h->shape.prev_bytes), s));
    h->wpos = 0;
    return NEO_HIP_OK;
}

void destroy64(upols64_t* h)
{
    if (!h) return;
    dfree(h->H);
    dfree(h->fdl);
    dfree(h->part);
    dfree(h->prev);
    batch_free64(h);
    offline_free64(h);
    dfree(h->samples_dev);
    hfree(h->samples_host);
    delete h;  // h->stream is shared (dmem.hip)
}

// a filter call's last steps, rc its body's result: the state is rebuilt as the reference's filter()
// does (uniform_partitioned_convolver.hpp:37-45), the stream is joined and the scratch goes back
int set_end64(upols64_t* h, int rc, std::initializer_list<void*> scratch)
{
    h->ospectra_stale = true;  // the offline windows' segment spectra: rebuilt by the next window pass
    if (!rc) rc = reset_state64(h, h->stream);
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    for (void* p : scratch) dfree(p);
    return rc;
}

// one block of every channel: the step pair on s
int launch_step64(upols64_t* h, const double* in, int64_t ld_in, double* out, int64_t ld_out, hipStream_t s)
{
    const upols64_shape& sh = h->shape;
    const dim3 grid(unsigned(sh.C), unsigned(sh.S));
    if (sh.ola) {
        NEO_UPOLS_DISPATCH(sh.B, hipLaunchKernelGGL((k_upols64_step<BB, true>), grid, dim3(256), 0, s, in, ld_in, h->prev,
                                                    h->H, h->fdl, h->part, h->tw, sh.P, sh.S, sh.rows, h->wpos))
    } else {
        NEO_UPOLS_DISPATCH(sh.B, hipLaunchKernelGGL((k_upols64_step<BB, false>), grid, dim3(256), 0, s, in, ld_in, h->prev,
                                                    h->H, h->fdl, h->part, h->tw, sh.P, sh.S, sh.rows, h->wpos))
    }
    NEO_HIP_LAUNCH_CHECK();
    if (sh.ola) {
        NEO_UPOLS_DISPATCH(sh.B, hipLaunchKernelGGL((k_upols64_finish<BB, true>), dim3(unsigned(sh.C)), dim3(256), 0, s,
                                                    h->part, out, ld_out, h->prev, h->tw, sh.S))
    } else {
        NEO_UPOLS_DISPATCH(sh.B, hipLaunchKernelGGL((k_upols64_finish<BB, false>), dim3(unsigned(sh.C)), dim3(256), 0, s,
                                                    h->part, out, ld_out, h->prev, h->tw, sh.S))
    }
    NEO_HIP_LAUNCH_CHECK();
    h->wpos = (h->wpos + 1) % sh.P;
    return NEO_HIP_OK;
}

// n = k B samples of every channel on s, no host wait in between: with offline windows on, the
// whole windows of 128 blocks first; with batching on, the whole passes of T blocks next; what is
// left (all of it with both off), one step pair per block
int process64(upols64_t* h, const double* in, int64_t ld_in, double* out, int64_t ld_out, int64_t n, hipStream_t s)
{
    if (int rc = h->used.note(s)) return rc;
    int64_t done = 0;
    if (h->offline)
        for (const int64_t pass = int64_t(kOff64W) * h->shape.B; done + pass <= n; done += pass)
            if (int rc = launch_window64(h, in + done, ld_in, out + done, ld_out, s)) return rc;
    if (h->batch.T > 1)
        for (const int64_t pass = int64_t(h->batch.T) * h->shape.B; done + pass <= n; done += pass)
            if (int rc = launch_pass64(h, in + done, ld_in, out + done, ld_out, s)) return rc;
    for (; done < n; done += h->shape.B)
        if (int rc = launch_step64(h, in + done, ld_in, out + done, ld_out, s)) return rc;
    return NEO_HIP_OK;
}

}  // namespace

extern "C" {

NEO_HIP_API int neo_hip_upols64_plan(int channels, int block, int partitions, int split_workgroups, int* splits,
                                     int* rows, int64_t* state_bytes)
{
    upols64_shape sh;
    if (const char* why = make_upols64_shape(channels, block, partitions, 0, split_workgroups, sh))
        return fail(NEO_HIP_EINVAL, "%s", why);
    if (splits) *splits = sh.S;
    if (rows) *rows = sh.rows;
    if (state_bytes) *state_bytes = sh.state_bytes;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols64_create(int channels, int block, int partitions, int device, int method,
                                       int split_workgroups, neo_hip_upols64** out)
{
    if (!out) return fail(NEO_HIP_EINVAL, "handle pointer is null");
    *out = nullptr;
    upols64_shape sh;
    if (const char* why = make_upols64_shape(channels, block, partitions, method, split_workgroups, sh))
        return fail(NEO_HIP_EINVAL, "%s", why);
    device_guard g(device);
    if (g.rc) return g.rc;
    auto* h = new upols64_t{};
    h->shape = sh;
    h->split_workgroups = split_workgroups;
    auto bail = [&](int code) {
        destroy64(h);
        return code;
    };
    (void)hipGetDevice(&h->device);
    if (int rc = shared_stream(&h->stream)) return bail(rc);
    if (dalloc(&h->H, size_t(sh.filter_bytes)) || dalloc(&h->fdl, size_t(sh.fdl_bytes)) ||
        dalloc(&h->part, size_t(sh.slab_bytes)) || dalloc(&h->prev, size_t(sh.prev_bytes)))
        return bail(fail(NEO_HIP_ENOMEM, "device allocation of %lld bytes failed", (long long)sh.state_bytes));
    if (int rc = shared_tw64(&h->tw, block)) return bail(rc);
    // stream-ordered zeroing, one wait at the end (the caller's later work may run on any stream)
    if (hipMemsetAsync(h->H, 0, size_t(sh.filter_bytes), h->stream) != hipSuccess)
        return bail(fail(NEO_HIP_ERUNTIME, "memset failed"));
    if (int rc = reset_state64(h, h->stream)) return bail(rc);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return bail(fail(NEO_HIP_ERUNTIME, "sync failed"));
    *out = h;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols64_destroy(neo_hip_upols64* h)
{
    if (!h) return NEO_HIP_OK;
    device_guard g(h->device);
    (void)setup_join64(h, false);
    destroy64(h);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols64_info(neo_hip_upols64* h, int* splits, int* rows, int64_t* state_bytes)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    if (splits) *splits = h->shape.S;
    if (rows) *rows = h->shape.rows;
    if (state_bytes) *state_bytes = h->shape.state_bytes;
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols64_reset(neo_hip_upols64* h)
{
    if (!h) return fail(NEO_HIP_EINVAL, "null handle");
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = setup_join64(h, false)) return rc;
    if (int rc = reset_state64(h, h->stream)) return rc;
    NEO_HIP_CHECK(hipStreamSynchronize(h->stream));
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_upols64_set_filter(neo_hip_upols64* h, const void* filter, int is_device)
{
    if (!h || !filter) return fail(NEO_HIP_EINVAL, "null handle or filter");
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = setup_join64(h, is_device != 0)) return rc;
    const upols64_shape& sh = h->shape;
    const int64_t rows = int64_t(sh.C) * sh.P, total = rows * sh.B;
    cd* tmp = nullptr;
    const cd* src = nullptr;
    int rc = stage_in(static_cast<const cd*>(filter), size_t(rows) * size_t(sh.B + 1) * sizeof(cd), is_device != 0, false,
                      h->stream, &tmp, &src);
    if (!rc) {
        hipLaunchKernelGGL(k_pack64, dim3(unsigned((total + 255) / 256)), dim3(256), 0, h->stream, src, h->H, sh.B, rows);
        if (hipGetLastError() != hipSuccess) rc = fail(NEO_HIP_ERUNTIME, "filter pack launch failed");
    }
    return set_end64(h, rc, {tmp});
}

NEO_HIP_API int neo_hip_upols64_set_impulse(neo_hip_upols64* h, const double* ir, int64_t length, int normalize,
                                            int is_device)
{
    if (!h || !ir || length < 1) return fail(NEO_HIP_EINVAL, "null handle/ir or empty impulse");
    const upols64_shape& sh = h->shape;
    if (partitions_for(length, sh.B) != sh.P)
        return fail(NEO_HIP_EINVAL, "impulse of %lld taps gives %lld partitions, convolver has %d", (long long)length,
                    (long long)partitions_for(length, sh.B), sh.P);
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (int rc = setup_join64(h, is_device != 0)) return rc;
    double *tmp = nullptr, *factor = nullptr;
    const double* d = nullptr;
    // a copy of the impulse when it is normalized (the caller's stays as it is)
    int rc = stage_in(ir, size_t(sh.C) * size_t(length) * sizeof(double), is_device != 0, normalize != 0, h->stream, &tmp, &d);
    if (!rc && normalize) {
        if (dalloc(&factor, size_t(sh.C) * sizeof(double))) rc = fail(NEO_HIP_ENOMEM, "allocation failed");
        if (!rc) rc = normalize64(tmp, sh.C, length, factor, h->stream);
    }
    if (!rc) rc = partition64(d, sh.C, length, sh.B, true, h->H, h->tw, h->stream);
    return set_end64(h, rc, {tmp, factor});
}

NEO_HIP_API int neo_hip_upols64_process_samples(neo_hip_upols64* h, const double* in, int64_t ld_in, double* out,
                                                int64_t ld_out, int64_t num_samples, int is_device, void* stream)
{
    if (!h || !in || !out) return fail(NEO_HIP_EINVAL, "null handle or buffer");
    if (const char* why = upols64_io_refusal(h->shape.B, num_samples, ld_in, ld_out)) return fail(NEO_HIP_EINVAL, "%s", why);
    if (is_device && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15))
        return fail(NEO_HIP_EINVAL, "I/O must be 16-byte aligned (ld multiple of 2 doubles)");
    if (num_samples == 0) return NEO_HIP_OK;
    device_guard g(h->device);
    if (g.rc) return g.rc;
    if (is_device) return process64(h, in, ld_in, out, ld_out, num_samples, as_stream(stream));
    hipStream_t s = stream ? as_stream(stream) : h->stream;
    // host I/O: pinned staging (grown on demand), 1-D copies, synchronous
    const int C = h->shape.C;
    const size_t count = size_t(C) * size_t(num_samples);
    if (count > h->samples_cap) {
        NEO_HIP_CHECK(hipStreamSynchronize(s));  // no queued work on the old staging
        dfree(h->samples_dev);
        hfree(h->samples_host);
        h->samples_dev = nullptr;
        h->samples_host = nullptr;
        h->samples_cap = 0;
        if (int rc = dalloc(&h->samples_dev, count * sizeof(double))) return rc;
        void* dmap = nullptr;  // not used: the samples go by DMA
        if (int rc = halloc(reinterpret_cast<void**>(&h->samples_host), &dmap, count * sizeof(double))) return rc;
        h->samples_cap = count;
    }
    for (int c = 0; c < C; ++c)
        std::copy(in + c * ld_in, in + c * ld_in + num_samples, h->samples_host + size_t(c) * num_samples);
    NEO_HIP_CHECK(hipMemcpyAsync(h->samples_dev, h->samples_host, count * sizeof(double), hipMemcpyHostToDevice, s));
    if (int rc = process64(h, h->samples_dev, num_samples, h->samples_dev, num_samples, num_samples, s)) return rc;
    NEO_HIP_CHECK(hipMemcpyAsync(h->samples_host, h->samples_dev, count * sizeof(double), hipMemcpyDeviceToHost, s));
    NEO_HIP_CHECK(hipStreamSynchronize(s));
    for (int c = 0; c < C; ++c)
        std::copy(h->samples_host + size_t(c) * num_samples, h->samples_host + size_t(c + 1) * num_samples,
                  out + c * ld_out);
    return NEO_HIP_OK;
}

NEO_HIP_API int neo_hip_uniform_partition_f64(const double* ir, int channels, int64_t length, int block, void* out,
                                              int is_device, int device)
{
    if (!ir || !out || channels < 1 || length < 1) return fail(NEO_HIP_EINVAL, "bad arguments");
    if (!valid_block(block)) return fail(NEO_HIP_EINVAL, "block must be a power of two in [16, 4096], got %d", block);
    device_guard g(device);
    if (g.rc) return g.rc;
    const int64_t P = partitions_for(length, block);
    const size_t in_bytes = size_t(channels) * size_t(length) * sizeof(double);
    const size_t out_bytes = size_t(channels) * size_t(P) * size_t(block + 1) * sizeof(cd);
    hipStream_t s = nullptr;
    if (is_device)
        if (int rc = null_join()) return rc;  // after its producer (common.hpp: null_join)
    if (int rs = shared_stream(&s)) return rs;
    const cd* tw = nullptr;
    const double* d_ir = nullptr;
    double* tmp_in = nullptr;
    cd* d_out = static_cast<cd*>(out);
    int rc = shared_tw64(&tw, block);
    if (!rc) rc = stage_in(ir, in_bytes, is_device != 0, false, s, &tmp_in, &d_ir);
    if (!rc && !is_device && dalloc(&d_out, out_bytes)) rc = fail(NEO_HIP_ENOMEM, "allocation failed");
    if (!rc) rc = partition64(d_ir, channels, length, block, false, d_out, tw, s);
    if (!rc && !is_device && hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(NEO_HIP_ERUNTIME, "copy back failed");
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    dfree(tmp_in);  // the stream was joined above
    if (!is_device) dfree(d_out);
    return rc;
}

NEO_HIP_API int neo_hip_normalize_impulse_f64(double* ir, int channels, int64_t length, int is_device, int device)
{
    if (!ir || channels < 0 || length < 0) return fail(NEO_HIP_EINVAL, "bad arguments");
    if (channels == 0 || length == 0) return NEO_HIP_OK;
    device_guard g(device);
    if (g.rc) return g.rc;
    hipStream_t s = nullptr;
    if (is_device)
        if (int rc = null_join()) return rc;  // after its producer (common.hpp: null_join)
    if (int rs = shared_stream(&s)) return rs;
    const size_t bytes = size_t(channels) * size_t(length) * sizeof(double);
    double *tmp = nullptr, *factor = nullptr;
    const double* src = nullptr;
    int rc = stage_in(ir, bytes, is_device != 0, false, s, &tmp, &src);
    double* d = is_device ? ir : tmp;
    if (!rc && dalloc(&factor, size_t(channels) * sizeof(double))) rc = fail(NEO_HIP_ENOMEM, "allocation failed");
    if (!rc) rc = normalize64(d, channels, length, factor, s);
    if (!rc && !is_device && hipMemcpyAsync(ir, d, bytes, hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(NEO_HIP_ERUNTIME, "copy back failed");
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail(NEO_HIP_ERUNTIME, "sync failed");
    dfree(tmp);  // the stream was joined above
    dfree(factor);
    return rc;
}

}  // extern "C"
