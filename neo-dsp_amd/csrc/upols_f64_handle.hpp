// upols_f64_handle.hpp — what the two translation units of the double-precision UPOLS / UPOLA
// convolvers share: the per-B geometry, the handle and the calls across the file boundaries.
//   upols_f64.hip          the plain two-launch step, the setup path, the C ABI of the handle
//   upols_f64_batch.hip    batched passes: T blocks per read of the filter and the delay line
//   upols_f64_offline.hip  offline windows: 128 blocks per pass, 256-point transforms along the blocks
#pragma once

#include "common.hpp"
#include "fft_device_real.hpp"
#include "upols_f64_plan.hpp"
#include "upols_handle.hpp"

namespace neo_hip {

// Rows are B complex doubles, 16 bytes each: a lane loads one bin per value (global_load_dwordx4),
// QT lanes cover (a chunk of) a row, RPI rows per iteration where a row is shorter than the
// workgroup. Above 512 bins a workgroup walks the row in NCH chunks of 512 bins, the loop over the
// partitions inside, so the accumulators (8 VGPRs per bin) and the loads in flight (U rows x VPT
// bins x 2 values x 4 VGPRs = 32) do not grow with B.
template<int B>
struct cfg64 {
    static constexpr int QT = B < 256 ? B : 256;
    static constexpr int RPI = 256 / QT;
    static constexpr int VPT = B / QT >= 2 ? 2 : 1;
    static constexpr int NCH = B / (QT * VPT);
    static constexpr int U = 4 / VPT;
    static constexpr int EW = B / 8 <= 256 ? 8 : B / 256;  // window transform: elements per lane
    static constexpr int EF = B / 4 <= 256 ? 4 : B / 256;  // tail transform
    static constexpr int TW1 = twiddle_len<B>();
    static constexpr int TW2 = twiddle_len<2 * B>();
    static constexpr int LL = lds_len(B);
    static_assert(RPI == 1 || NCH == 1, "row groups fold through LDS once");
};

}  // namespace neo_hip

struct neo_hip_upols64 {
    neo_hip::upols64_shape shape;  // the plan (upols_f64_plan.hpp)
    int device = 0;
    hipStream_t stream = nullptr;  // one of the device's shared setup streams
    neo_hip::cd* H = nullptr;      // [C][P][B]
    neo_hip::cd* fdl = nullptr;    // [C][P][B], ring of P rows
    neo_hip::cd* part = nullptr;   // slabs [C][S][B]
    double* prev = nullptr;        // [C][B]
    const neo_hip::cd* tw = nullptr;  // twiddles of B and 2B
    int wpos = 0;                  // FDL write position (fdl_index.hpp:35-37), host-side
    double* samples_dev = nullptr;   // host-pointer process_samples: device side
    double* samples_host = nullptr;  // and pinned staging
    size_t samples_cap = 0;
    neo_hip::stream_set used;  // streams the step calls ran on since the last setup call
    // batched passes (upols_f64_batch.hip): off until set_batch; the buffers hold nothing between passes
    int split_workgroups = 0;            // as given at create: the passes' split rule reads it too
    neo_hip::upols64_batch_shape batch;  // batch.T == 1: off
    neo_hip::cd* bscratch = nullptr;     // fresh spectra N [C][T][B]
    neo_hip::cd* bpart = nullptr;        // slabs [C][S_b][T][B]
    double* btail = nullptr;             // overlap-add: tails [C][T][B]
    // offline windows (upols_f64_offline.hip): off until set_offline; only the spectra outlive a pass
    bool offline = false;
    bool ospectra_stale = true;             // the filter changed since k_upols64_ohf last ran
    neo_hip::upols64_offline_shape oshape;  // nseg == 0: off
    neo_hip::cd* ospectra = nullptr;        // HF [C][nseg][256][B]
    neo_hip::cd* oscratch = nullptr;        // fresh spectra N [C][128][B]
    neo_hip::cd* oy = nullptr;              // Y [C][128][B], the one slab of k_upols64_bfinish
    double* otail = nullptr;                // overlap-add: tails [C][128][B]
    const neo_hip::cd* otw = nullptr;       // twiddles of the 256-point transform
};

namespace neo_hip {

// order a setup call after every step of this handle (upols_f64.hip)
int setup_join64(neo_hip_upols64* h, bool device_input);
// one pass of h->batch.T blocks of every channel on s (upols_f64_batch.hip)
int launch_pass64(neo_hip_upols64* h, const double* in, int64_t ld_in, double* out, int64_t ld_out, hipStream_t s);
void batch_free64(neo_hip_upols64* h);
// the pass's launches 1 and 3 (+ 4, overlap-add) for TB blocks with one slab per block, on buffers
// of the caller's: the window passes' transforms and finish (upols_f64_batch.hip)
int launch_bwindow64(neo_hip_upols64* h, const double* in, int64_t ld_in, cd* N, int TB, hipStream_t s);
int launch_bfinish64(neo_hip_upols64* h, const cd* slab, const cd* N, double* tails, int TB, const double* in,
                     int64_t ld_in, double* out, int64_t ld_out, hipStream_t s);
// the double twiddle tables of block B (B-point, then 2B-point) on the current device (upols_f64.hip)
int shared_tw64(const cd** out, int B);
// one window pass of 128 blocks of every channel on s (upols_f64_offline.hip)
int launch_window64(neo_hip_upols64* h, const double* in, int64_t ld_in, double* out, int64_t ld_out, hipStream_t s);
void offline_free64(neo_hip_upols64* h);

}  // namespace neo_hip
