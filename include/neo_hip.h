/*
 * neo_hip.h — C-ABI drop-in boundary of the MI355X (gfx950) FFT + UPOLS hot path.
 *
 * libneo_hip.so exports exactly these symbols. Plain pointers, sizes and int
 * status codes only (no HIP / torch / C++ types in the signatures), so the
 * reference's C++ headers (include/neo/fft.hpp, include/neo/convolution.hpp in
 * this repo), its pybind11 module or any FFI can bind them.
 *
 * Conventions shared with the reference (paths relative to neo-dsp's tree):
 *   - complex data is interleaved float {re, im} = std::complex<float>
 *     (src/neo/complex/scalar_complex.hpp:14-114);
 *   - direction: -1 = forward e^{-2 pi i nk/N}, +1 = backward
 *     (src/neo/fft/direction.hpp:8-12); transforms are UNNORMALIZED
 *     (src/neo/fft/reference/c2c_dit2_plan.hpp:81-95);
 *   - r2c writes N/2+1 bins; c2r reads N/2+1 bins, ignores the imaginary parts of
 *     the DC and Nyquist bins and does not scale
 *     (src/neo/fft/fallback/fallback_rfft_plan.hpp:27-55);
 *   - UPOLS filters are uniform_partition's [C][P][B+1] layout
 *     (src/neo/convolution/uniform_partition.hpp:12-26).
 * Every function returns NEO_HIP_OK (0) or a nonzero status; neo_hip_last_error()
 * then holds a message (thread-local). Construction errors map to the
 * reference's std::runtime_error (c2c_dit2_plan.hpp:97-104).
 *
 * Threads and streams:
 *   - DISTINCT OBJECTS (FFT plans, convolver handles of every kind, overlap stages, groups,
 *     multi-device convolvers) may be used at the same time from distinct threads with no
 *     locking by the caller; what they share inside the library (the device-memory pool, the
 *     four streams per device, the twiddle tables, the groups' page-lock table) is the
 *     library's to protect. Results are bit-identical to the same calls made one thread after
 *     the other.
 *   - ONE-SHOT ENTRY POINTS are re-entrant: neo_hip_fft_convolve*, neo_hip_direct_convolve*,
 *     neo_hip_stft*, neo_hip_uniform_partition, neo_hip_normalize_impulse, neo_hip_perceptual_*.
 *   - ONE FFT PLAN may be executed from several threads and on several streams. The library
 *     serialises what the plan's buffers require: neo_hip_fft_execute_host calls on one plan
 *     run one after the other (one pair of staging buffers), and an execute of a multi-pass
 *     plan (inner order above 12: the plan owns scratch) on another stream than the plan's
 *     last execute first waits, on the device, for that execute. A call's result is that of
 *     the call alone. Destroying a plan is for one thread, after its last call has returned.
 *   - ONE CONVOLVER HANDLE, OVERLAP STAGE OR GROUP is for one thread at a time, as the
 *     reference's stateful convolvers are: its calls carry state from block to block and take
 *     no lock on the step path. A caller that moves one between threads orders the calls.
 *     One handle's process calls on DIFFERENT streams are the caller's to order as well (an
 *     event from one stream to the next); setup and destroy calls wait for the handle's calls
 *     on every stream they ran on (those streams, never the device) before they free,
 *     reallocate or rewrite a buffer, so they may follow a queued call with no wait between.
 *   - neo_hip_last_error() is per thread: the message of the calling thread's last failed call.
 */
#ifndef NEO_HIP_H
#define NEO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define NEO_HIP_API __attribute__((visibility("default")))
#else
#define NEO_HIP_API
#endif

enum neo_hip_status {
    NEO_HIP_OK = 0,
    NEO_HIP_EINVAL = 1,   /* bad argument (order > max_order, null pointer, shape) */
    NEO_HIP_ERUNTIME = 2, /* HIP runtime / kernel failure */
    NEO_HIP_ENOMEM = 3,   /* device allocation failed */
    NEO_HIP_ENODEV = 4    /* no such GPU */
};

/* fft kinds; OR NEO_HIP_F64 for std::complex<double> / double plans (the reference's
 * fft_plan<complex<double>>, rfft_plan<double>; Python _neo.fft complex128 overloads,
 * extra/python/src/main.cpp:248-252). */
enum neo_hip_fft_kind { NEO_HIP_C2C = 0, NEO_HIP_R2C = 1, NEO_HIP_C2R = 2, NEO_HIP_F64 = 16 };

typedef struct neo_hip_fft_plan neo_hip_fft_plan;
typedef struct neo_hip_upols neo_hip_upols;

/* -- library ------------------------------------------------------------ */
/* ABI version of this header. neo_hip_upols_opts grows with it (0.1.0: 6 ints; 0.2.0: the 10
 * below), so a caller checks neo_hip_version() == NEO_HIP_VERSION before passing one.
 * 0.3.0: the sparse convolvers (neo_hip_upols_create_sparse and what goes with it).
 * 0.4.0: the perceptual sparsity predicate (neo_hip_perceptual_* and the two handle calls).
 * 0.5.0: batched passes on sparse handles (set_batch(1) accepted; neo_hip_upols_sparse_window_plan,
 *        neo_hip_upols_sparse_batch_info).
 * 0.6.0: the matrix convolver (neo_hip_matrix_*).
 * 0.7.0: batched passes on matrix handles (neo_hip_matrix_set_batch, neo_hip_matrix_batch_info,
 *        neo_hip_matrix_batch_plan).
 * 0.8.0: offline windows on matrix handles (neo_hip_matrix_set_offline, neo_hip_matrix_offline_info,
 *        neo_hip_matrix_offline_plan; neo_hip_matrix_desc gains offline_bytes at its end).
 * 0.9.0: crossfaded live filter updates on matrix handles (neo_hip_matrix_update_filter,
 *        neo_hip_matrix_update_impulse, neo_hip_matrix_fade_info, neo_hip_matrix_fade_gains).
 * 0.10.0: window levels on matrix handles, long filters one block per call (neo_hip_matrix_set_levels,
 *        neo_hip_matrix_levels_info, neo_hip_matrix_level_plan).
 * 0.11.0: staggered level windows (neo_hip_upols_opts gains windows at its end: 11 ints;
 *        neo_hip_upols_stagger_plan).
 * 0.12.0: the step groups' background stream is readable (neo_hip_upols_get_background_stream).
 * 0.13.0: crossfaded live filter updates on dense upols / upola handles (neo_hip_upols_update_filter,
 *        neo_hip_upols_update_impulse, neo_hip_upols_fade_info, neo_hip_upols_multi_update_filter,
 *        neo_hip_upols_multi_update_impulse).
 * 0.14.0: crossfaded live filter updates on sparse handles (neo_hip_upols_update_filter_sparse,
 *        neo_hip_upols_update_filter_perceptual, neo_hip_upols_update_impulse_perceptual,
 *        neo_hip_upols_sparse_fade_plan; neo_hip_upols_fade_info and neo_hip_upols_sparse_info follow
 *        a sparse handle's fade).
 * 0.15.0: double-precision upols / upola convolvers (neo_hip_upols64_*) and the setup path in double
 *        (neo_hip_uniform_partition_f64, neo_hip_normalize_impulse_f64).
 * 0.16.0: batched passes on double-precision handles (neo_hip_upols64_set_batch,
 *        neo_hip_upols64_batch_info, neo_hip_upols64_batch_plan).
 * 0.17.0: offline windows on double-precision handles (neo_hip_upols64_set_offline,
 *        neo_hip_upols64_offline_info, neo_hip_upols64_offline_plan). */
#define NEO_HIP_VERSION 1700 /* 0.17.0 */
NEO_HIP_API const char* neo_hip_last_error(void);
NEO_HIP_API int neo_hip_version(void);
NEO_HIP_API int neo_hip_device_count(int* count);
/* Page-lock a caller-owned host range [p, p + bytes) and map it for every device, so that
 * host-memory entry points (neo_hip_upols_process) read and write it in place over PCIe
 * instead of staging it. The caller keeps the range alive until neo_hip_host_unregister(p). */
NEO_HIP_API int neo_hip_host_register(void* p, int64_t bytes);
NEO_HIP_API int neo_hip_host_unregister(void* p);
/* Handle buffers come from per-device chunks the library keeps mapped (256 MiB, or a request's own
 * size above 64 MiB), so creating and destroying convolvers never synchronizes the device. Empty
 * chunks stay cached (up to a quarter of the device's memory) for later handles; trim returns
 * every chunk no handle uses; info reports the bytes held and the bytes in use on a device. */
NEO_HIP_API int neo_hip_memory_trim(int device);
NEO_HIP_API int neo_hip_memory_info(int device, int64_t* reserved, int64_t* in_use);

/* -- FFT plans ------------------------------------------------------------
 * Replaces fft_plan<complex<float>> = c2c_dit2_plan (src/neo/fft/fft.hpp:36-52,
 * c2c_dit2_plan.hpp:21-104) and rfft_plan<float> = fallback_rfft_plan
 * (src/neo/fft/rfft.hpp:15-23, fallback_rfft_plan.hpp:14-61), batched.
 * max order 27 (c2c_dit2_plan.hpp:58-61); order > 27 -> NEO_HIP_EINVAL. */
NEO_HIP_API int neo_hip_fft_max_order(void);
NEO_HIP_API int neo_hip_fft_plan_create(int order, int64_t batch, int kind, int device, neo_hip_fft_plan** plan);
NEO_HIP_API int neo_hip_fft_plan_destroy(neo_hip_fft_plan* plan);
/* Device pointers, asynchronous on `stream` (a hipStream_t; NULL = the HIP
 * null stream, which is also torch's default stream). c2c: in/out [batch][N] complex (in == out allowed).
 * r2c: in [batch][N] float, out [batch][N/2+1] complex.
 * c2r: in [batch][N/2+1] complex, out [batch][N] float. `direction` is used by
 * c2c only (r2c is forward, c2r backward, as in fallback_rfft_plan). */
NEO_HIP_API int neo_hip_fft_execute(neo_hip_fft_plan* plan, const void* in, void* out, int direction, void* stream);
/* Host pointers, synchronous (staging through the plan's device buffers). */
NEO_HIP_API int neo_hip_fft_execute_host(neo_hip_fft_plan* plan, const void* in, void* out, int direction);

/* -- UPOLS convolver --------------------------------------------------------
 * Replaces C instances of upols_convolver<complex<float>> (one per channel,
 * src/neo/convolution/dense_convolver.hpp:19-20;
 * uniform_partitioned_convolver.hpp:13-65; overlap_save.hpp:84-112;
 * fdl_index.hpp:23-36) as driven by dense_convolve / DenseConvolution
 * (extra/plugin/src/dsp/DenseConvolution.hpp:35,39-70). `block` = B must be a
 * power of two in [16, 4096]; output block t corresponds to input block t
 * (zero latency). Channels are independent. */
NEO_HIP_API int neo_hip_upols_create(int channels, int block, int partitions, int device, neo_hip_upols** h);
/* Same engine with the overlap-add stage: C instances of upola_convolver<complex<float>>
 * (dense_convolver.hpp:23-24; overlap_add.hpp:76-106). All other neo_hip_upols_*
 * entry points apply to it unchanged. */
NEO_HIP_API int neo_hip_upola_create(int channels, int block, int partitions, int device, neo_hip_upols** h);
/* C instances of upola_convolver_v2<complex<float>> = overlap_add_convolver
 * (dense_convolver.hpp:28; overlap_add_convolver.hpp:20-136): overlap-add that also
 * takes sub-block input through neo_hip_upols_process_samples, with the reference's
 * window state (the irfft result is written back into the real window, :114). Whole
 * blocks through the other process calls behave like neo_hip_upola_create. */
NEO_HIP_API int neo_hip_upola2_create(int channels, int block, int partitions, int device, neo_hip_upols** h);
/* Any of the three with explicit choices instead of the shape-based defaults
 * (method 0 = upols, 1 = upola, 2 = upola v2; opts NULL = all defaults). Results are the
 * same for every choice up to float summation order; they exist so that every code path
 * can be exercised and timed on any shape. */
typedef struct neo_hip_upols_opts {
    int fused;            /* plain step: -1 auto (one launch below 64 MiB of filter + FDL), 0 MAC + finish, 1 one launch */
    int split_workgroups; /* plain step: 0 auto (1024 workgroups, >= 8 or 16 partitions per split), else the
                             workgroup target for its partition splits, taken as given (up to 64 per channel) */
    int batch_blocks;     /* batched passes: 0 auto (32), else blocks per pass (power of two, 2..32) */
    int batch_bins;       /* batched passes: 0 auto (1), else bins per lane vector (1 or 2) */
    int levels;           /* single-block steps: -1 auto (streaming levels from 64 partitions), 0 plain step, 1 levels */
    int far_level;        /* streaming levels, partitions >= 256: -1 auto (= 1), 0 a 128-block Toeplitz level (more
                             VALU / LDS work), 1 the 128-block partition-axis transform level with stored segment
                             and row-pair spectra, 2 the same transform recomputed every window from the filter and
                             FDL rows (fewest bytes; 2 nseg + 1 transforms per unit and window: more VALU, a longer
                             chain) */
    int far_group;        /* far transform level: 0 auto, else 1..4 windows per phase-1 pass over the stored
                             segment spectra (auto: 2, or round(sqrt(2 (nseg - 1))) from 32768 16-column units) */
    int toep_split;       /* 32-block Toeplitz level: 0 auto (2 below 256 16-column units), 1 whole windows per
                             workgroup, 2 two window halves */
    int step_group;       /* streaming levels: 0 auto, 1 one launch per block (the block and 1/T of every level's
                             next window), 2, 4 or 8 step groups: the block of every call as a launch of its own on the
                             caller's stream, the level slices of G calls as ONE launch on the handle's background
                             stream, issued at the group's first call (ordered by events; the output of a call is
                             complete when the caller's stream reaches it, as with G = 1) */
    int far_phase2;       /* far transform level, G = 1: 0 auto, 1 one workgroup per unit (the fresh row pair's
                             transform kept in registers for the window's products), 2 two steps (the fresh
                             transform stored to its slot, read back with the products one step later: half the
                             chain per step); step groups always run 1 */
    int windows;          /* streaming levels with step groups: 0 auto, 1 aligned (every slice of a level's window
                             shares the window's start, bands from 2 T), 2 staggered (a level of window T >= 4 G and
                             the far level are cut into T / G classes of channels, each with a window phase of its
                             own: bands from T + 4 G, fewer rows per step; needs step groups and the far level's
                             stored form; no latency mode). Auto: staggered where the step group
                             is chosen automatically and channels x block / 16 >= 65536, aligned everywhere else
                             (a group's members too) */
} neo_hip_upols_opts;
NEO_HIP_API int neo_hip_upols_create_ex(int channels, int block, int partitions, int device, int method,
                                        const neo_hip_upols_opts* opts, neo_hip_upols** h);
/* -- Sparse convolvers ----------------------------------------------------------
 * C instances of sparse_upols_convolver / sparse_upola_convolver (method 0 / 1;
 * src/neo/convolution/sparse_convolver.hpp:12-17) over sparse_filter (sparse_filter.hpp:25-45),
 * as the plugin's sparse_convolve steps them (extra/plugin/src/dsp/DenseConvolution.cpp:124-186):
 * only the filter bins a mask keeps take part in the sums (the reference's CSR multiply_add,
 * src/neo/algorithm/multiply_add.hpp:303-324). The reference stores single bins; here the unit is
 * a TILE of 16 packed bins (128 B, one memory request) of a packed filter row: packed index 0 =
 * {DC, Nyquist}, so reference columns 0 and B both lie in tile 0 and column k in [1, B) in tile
 * k / 16. A tile is kept if the mask keeps any of its columns; the columns it drops inside a kept
 * tile are stored as zero (DC and Nyquist each on its own), so the results are those of the dense
 * convolver on the filter with the dropped columns zeroed. Per filter row the handle keeps a
 * bitmap of NW = max(1, B / 512) uint32 words (tile t = bit t % 32 of word t / 32) and an offset
 * in tiles into its channel's compacted values ([C][P + 1], the exclusive prefix sum of the rows'
 * popcounts); a block step reads the kept tiles of the filter and of the FDL rows only.
 * A sparse handle holds no dense filter buffer and no streaming-level or offline buffers.
 * Of opts only fused and split_workgroups apply (the partitions are cut at equal row counts, as
 * the dense plain step cuts them; with the same cuts and the same fused choice its outputs equal
 * the dense plain step's on the zeroed filter bit for bit, up to the sign of zero). method 2
 * (sub-block input) is EINVAL. On a sparse handle process, process_device, process_blocks,
 * process_samples (multiples of B), reset, info, destroy and the timing calls work. Batching is
 * OFF by default (one block per pass, as a real-time caller steps it); set_batch(1) turns it on:
 * process_blocks / process_samples then cut a call as on a dense handle, into the largest
 * power-of-two batches <= 32 of the whole blocks left, and the T blocks of a batch share ONE pass
 * over the kept filter tiles and over the FDL tiles of the window bitmaps (below); the rest run one
 * block per pass. Batched and single passes mix in any order at block boundaries; the results are
 * equal within float rounding (another summation order), and two runs of the same calls are equal
 * bit for bit. The batch buffers are allocated at the first batched pass.
 * set_filter and set_impulse (it takes set_filter_sparse, set_filter_perceptual or
 * set_impulse_perceptual), set_ahead(1), set_offline(1), set_persistent(1) and set_paced(1 / 2)
 * return EINVAL and name the reason, and their getters report off. Groups and the multi-device
 * convolver take no sparse members. */
NEO_HIP_API int neo_hip_upols_create_sparse(int channels, int block, int partitions, int device, int method,
                                            const neo_hip_upols_opts* opts, neo_hip_upols** h);
/* filter [C][P][B+1] complex and mask [C][P][B+1] bytes (nonzero = keep), both host or both device
 * memory; sparse handles only. Resets all state, like filter(). The bitmaps, offsets and compacted
 * tiles are made on the device; the call waits on the handle's stream, never on the device. */
NEO_HIP_API int neo_hip_upols_set_filter_sparse(neo_hip_upols* h, const void* filter, const uint8_t* mask, int is_device);
/* the current filter's kept columns and kept tiles over all channels, and the device bytes that
 * stand in for a dense handle's [C][R][B] filter buffer (tiles, bitmaps, offsets); from a live
 * update's call on (neo_hip_upols_update_filter_sparse) the filter being faded to */
NEO_HIP_API int neo_hip_upols_sparse_info(neo_hip_upols* h, int64_t* kept_bins, int64_t* kept_tiles, int64_t* filter_bytes);
/* The format on the host (no device needed; it is what set_filter_sparse computes on the device):
 * mask [C][P][B+1] -> tile_mask [C][P][NW], row_off [C][P+1], kept columns, kept tiles. */
NEO_HIP_API int neo_hip_upols_sparse_plan(const uint8_t* mask, int channels, int block, int partitions,
                                          uint32_t* tile_mask, uint32_t* row_off, int64_t* kept_bins, int64_t* kept_tiles);
/* The window bitmaps of a batched pass of `window` blocks (a power of two, 2..32), on the host (no
 * device needed): the FDL row that enters the pass at partition p meets the filter rows
 * p .. p + window - 1, so win_mask[c][p] = OR of tile_mask[c][q] over q in [p, min(P, p + window));
 * tile_mask (from neo_hip_upols_sparse_plan) and win_mask [C][P][NW], not the same buffer;
 * window_tiles (may be NULL) = the sum of win_mask's popcounts. */
NEO_HIP_API int neo_hip_upols_sparse_window_plan(const uint32_t* tile_mask, int channels, int block, int partitions,
                                                 int window, uint32_t* win_mask, int64_t* window_tiles);
/* Sparse handles: the blocks per batched pass T and its splits per channel (whether batching is on
 * or not; neo_hip_upols_batch_info reports what process_blocks does now), and the popcount sum of
 * the window bitmaps the device made for T at the last filter change. */
NEO_HIP_API int neo_hip_upols_sparse_batch_info(neo_hip_upols* h, int* blocks_per_pass, int* splits, int64_t* window_tiles);
/* -- Perceptual sparsity (the plugin's sparse_convolve threshold) -------------------
 * Which bins of a filter [C][P][B+1] (uniform_partition layout) a sparse handle keeps, as the
 * plugin decides it (extra/plugin/src/dsp/DenseConvolution.cpp:110-170; src/neo/unit/decibel.hpp,
 * src/neo/math/a_weighting.hpp), on the device:
 *   weights   w[k] = 100 for k < low_bins_to_keep; otherwise 0 (weighting 0) or the A-weighting in
 *             dB at f = k sample_rate / (2 B) (weighting 1; A(0) = -inf, so DC is dropped unless
 *             low_bins_to_keep >= 1). Computed in double on the host, rounded to float once.
 *   scale     per CHANNEL: 1 / max over p, k of re^2 + im^2 (float)
 *   level     x = (re^2 + im^2) scale; dB = max(-144, 20 log10 x) / 2 + w[k] for x > 0, else
 *             -72 + w[k] (zero bins, and every bin of an all-zero channel)
 *   keep      dB > threshold_db
 * Unweighted, a threshold below -72 therefore keeps every bin, zeros included.
 * The histograms count per channel the columns (hist_bins) and the 16-column tiles of the sparse
 * format (hist_tiles; a tile's level is the maximum over its columns, column B in tile 0) by level:
 * bucket j = min(143, floor(max(0, -dB))), [C][144] each. The tiles of channel c that an integer
 * threshold -k (1 <= k <= 143) keeps are the sum of hist_tiles[c][j] over j < k. threshold_db
 * plays no part in weights and histograms (it must be finite all the same). */
typedef struct neo_hip_perceptual {
    double sample_rate;   /* Hz, > 0 */
    float threshold_db;   /* finite; the plugin passes -dynamicRange, -10 .. -90 */
    int low_bins_to_keep; /* 0 .. B; columns below it are always kept */
    int weighting;        /* 0 = none, 1 = A-weighting */
} neo_hip_perceptual;
/* Every call below checks its arguments before a device is touched (EINVAL names the reason). */
NEO_HIP_API int neo_hip_perceptual_weights(int block, const neo_hip_perceptual* p, float* weights /* [B+1] */);
/* the definition, on the host (csrc/perceptual_plan.hpp; no device needed) */
NEO_HIP_API int neo_hip_perceptual_mask_host(const void* filter, int channels, int block, int partitions,
                                             const neo_hip_perceptual* p, uint8_t* mask);
NEO_HIP_API int neo_hip_perceptual_hist_host(const void* filter, int channels, int block, int partitions,
                                             const neo_hip_perceptual* p, int64_t* hist_bins, int64_t* hist_tiles);
/* the same on the device: filter and mask both host or both device memory; the histograms are
 * always host memory. Synchronous (one of the library's streams, never the device). */
NEO_HIP_API int neo_hip_perceptual_mask(const void* filter, int channels, int block, int partitions,
                                        const neo_hip_perceptual* p, uint8_t* mask, int is_device, int device);
NEO_HIP_API int neo_hip_perceptual_histogram(const void* filter, int channels, int block, int partitions,
                                             const neo_hip_perceptual* p, int64_t* hist_bins, int64_t* hist_tiles,
                                             int is_device, int device);
/* Sparse handles only: set_filter_sparse with the mask made on the device from `filter`
 * [C][P][B+1] (host or device memory), and the whole setup from an impulse response ir [C][length]
 * (normalize_impulse if `normalize`, uniform_partition, mask, tiles; all on the device, on the
 * handle's stream). Both reset all state, like filter(); a refused call leaves the handle as it was. */
NEO_HIP_API int neo_hip_upols_set_filter_perceptual(neo_hip_upols* h, const void* filter, const neo_hip_perceptual* p,
                                                    int is_device);
NEO_HIP_API int neo_hip_upols_set_impulse_perceptual(neo_hip_upols* h, const float* ir, int64_t length, int normalize,
                                                     const neo_hip_perceptual* p, int is_device);
NEO_HIP_API int neo_hip_upols_destroy(neo_hip_upols* h);
/* filter [C][P][B+1] complex (uniform_partition layout), host or device memory;
 * like uniform_partitioned_convolver::filter() it also resets all state. */
NEO_HIP_API int neo_hip_upols_set_filter(neo_hip_upols* h, const void* filter, int is_device);
/* normalize_impulse + uniform_partition of ir [C][L] float straight into the
 * convolver (setup path, DenseConvolution.cpp:78-108); host or device memory. */
NEO_HIP_API int neo_hip_upols_set_impulse(neo_hip_upols* h, const float* ir, int64_t length, int normalize, int is_device);
/* one block for all channels, in place: io [C][B] float. Host memory, synchronous (own
 * stream if `stream` is NULL): the step kernel reads and writes the block over PCIe
 * itself -- in place if io is page-locked (neo_hip_host_register / hipHostMalloc), else
 * through the handle's mapped pinned staging (one memcpy each way) -- and the call waits by
 * polling the stream. Device memory: same as process_device on `stream`. */
NEO_HIP_API int neo_hip_upols_process(neo_hip_upols* h, float* io, int io_is_device, void* stream);
/* one block, device pointers, channel c at in + c*ld_in / out + c*ld_out
 * (in == out allowed); asynchronous on `stream` (NULL = HIP null stream). Both pointers
 * 16-byte aligned, ld_in and ld_out multiples of 4 and >= B (they may differ); anything else is
 * EINVAL and leaves the state as it was. The call reads [c*ld_in, c*ld_in + B) of every channel
 * and writes [c*ld_out, c*ld_out + B), nothing else; `in` is left as it was unless it is `out`. */
NEO_HIP_API int neo_hip_upols_process_device(neo_hip_upols* h, const float* in, int64_t ld_in, float* out,
                                             int64_t ld_out, void* stream);
/* nblocks consecutive blocks: channel c samples at in + c*ld + t*B (16-byte aligned, ld
 * a multiple of 4; in == out allowed). With batching on (the default) whole groups of T
 * blocks (32 for B <= 512, fewer for larger blocks; neo_hip_upols_batch_info) share one
 * pass over the filter and the FDL, so HBM traffic per block drops ~T-fold; results equal the one-block-per-pass path within
 * float rounding (another summation order). The rest run one block per pass. */
NEO_HIP_API int neo_hip_upols_process_blocks(neo_hip_upols* h, const float* in, float* out, int64_t ld,
                                             int64_t nblocks, void* stream);
/* process_blocks batching on (default) or off (one block per pass, as a real-time
 * caller stepping process_device block by block). */
NEO_HIP_API int neo_hip_upols_set_batch(neo_hip_upols* h, int enable);
/* blocks one process_blocks pass consumes (1 with batching off) and its splits per channel */
NEO_HIP_API int neo_hip_upols_batch_info(neo_hip_upols* h, int* blocks_per_pass, int* splits);
/* Offline windows (whole-block handles of >= 128 partitions; on by default): with batching on,
 * every 256 (or 128) whole blocks of a process_blocks / process_samples call take ONE pass that
 * computes each 128-block window of every bin as the far level does its band -- DFT256 along the
 * block axis of each 128-partition segment's FDL rows, times the filter segment's spectrum (made
 * at the first pass after a filter change), one inverse transform per window -- instead of T-block
 * MAC passes over all P partitions: ~(nseg + 2) 128 FDL rows and nseg 256 spectrum rows per column
 * and pass, not 2 P per 32 blocks. Same outputs within float rounding (the blocks are known up
 * front, as in the reference's offline harness, extra/plugin/src/dsp/DenseConvolution.hpp:39-70,
 * extra/plugin/src/ui/BenchmarkTab.hpp:47-66). The rest of a call runs the T-block passes. */
NEO_HIP_API int neo_hip_upols_set_offline(neo_hip_upols* h, int enable);
/* offline windows on, and the 128-partition segments they transform */
NEO_HIP_API int neo_hip_upols_get_offline(neo_hip_upols* h, int* enabled, int* segments);
/* num_samples samples for every channel: channel c at in + c*ld_in / out + c*ld_out
 * (in == out allowed), host (synchronous) or device (asynchronous on `stream`) memory.
 * upola_convolver_v2 handles accept any count, split at block boundaries like
 * overlap_add_convolver::operator() (:80-134); upols / upola handles need a multiple
 * of the block (the reference's operator() takes exactly one block). Device memory of upols /
 * upola handles, and of any handle in latency mode: both pointers 16-byte aligned, ld_in and
 * ld_out multiples of 4, as for process_device; upola_convolver_v2 handles take any (4-byte)
 * alignment and any ld >= num_samples, and run batched passes and the UPOLA launch pair only
 * where the alignment allows. Host memory: any alignment (it is staged). ld_in and ld_out may
 * differ; a refused call (EINVAL) leaves the state as it was. */
NEO_HIP_API int neo_hip_upols_process_samples(neo_hip_upols* h, const float* in, int64_t ld_in, float* out,
                                              int64_t ld_out, int64_t num_samples, int is_device, void* stream);
NEO_HIP_API int neo_hip_upols_reset(neo_hip_upols* h);
/* Live filter update of a dense upols / upola handle: crossfade from the handle's filter A to `filter`
 * (B, [C][P][B+1] complex like set_filter) over the next fade_blocks blocks, keeping ALL state (the
 * delay line, the previous block, the overlap-add tail); set_filter / set_impulse remain the
 * resetting calls. With y_A, y_B the outputs of two convolvers with filters A and B fed the whole
 * input from the start, sample n = 0 .. fade_blocks * B - 1 of the next fade_blocks blocks is
 * y_A + g[n] (y_B - y_A), g as neo_hip_matrix_fade_gains gives it (curve 0 linear, 1 raised cosine);
 * every block after them is y_B. On a handle that runs plain steps (no streaming levels) those are
 * bit for bit what a handle that had B from the start gives (overlap-add: from the second block after
 * the fade on; the first takes a tail summed in the fade kernel's order); a streaming handle primes
 * its levels after the fade at another phase than such a handle, so there the sums differ in order.
 * The new filter is packed into a second bank of the handle's own layout, allocated at the first
 * update (neo_hip_upols_fade_info reports it; beside it the fade's slabs [C][splits][2][B] and,
 * overlap-add, a second set of tails [C][B]) and kept until the handle is destroyed: no later update
 * allocates. While a fade has blocks left every whole block of every process call runs as one fade
 * step (two launches: both banks against the same delay-line rows; two inverse transforms and the
 * mix per channel) whatever the handle's modes say (streaming levels, step groups, paced pieces,
 * batched passes, offline windows); a longer call is cut at the fade's last block and goes on in its
 * usual passes, and the streaming levels prime again from the stepped delay line. A fade block
 * costs about one and a half plain steps, not a streaming step. Equal calls
 * give equal bits.
 * STREAM CONTRACT: `stream` must be the stream the caller's process calls run on, or be ordered
 * with it (after every earlier process call, before every later one): the update reads the delay
 * line those calls write (overlap-add) and writes the bank the later ones read. Device pointer:
 * asynchronous on `stream` (NULL = the HIP null stream). Host pointer: staged on `stream` (NULL = the
 * handle's stream, as host process calls) after the handle's earlier steps on any stream; returns
 * when the bank is written.
 * EINVAL, the handle unchanged: a null argument; before a filter is set; fade_blocks < 1 or > 2^20;
 * curve not 0 or 1; while a fade has blocks left; a sparse handle (it has forms of its own:
 * neo_hip_upols_update_filter_sparse); an upola_convolver_v2 handle; a
 * handle owned by a convolver group; a handle in latency mode (neo_hip_upols_set_persistent, which
 * in turn refuses to switch on while a fade has blocks left). set_filter / set_impulse cancel a
 * running fade; reset completes it (B is the filter) and clears the state; set_batch, set_offline,
 * set_ahead and set_paced keep it. */
NEO_HIP_API int neo_hip_upols_update_filter(neo_hip_upols* h, const void* filter, int is_device, int fade_blocks,
                                            int curve, void* stream);
/* The same from ir [C][length] float (host or device): normalize_impulse over the new impulse's
 * channels if `normalize`, then uniform_partition on the device straight into the second bank, as
 * set_impulse does. Also EINVAL: a length that gives another partition count than the handle's. */
NEO_HIP_API int neo_hip_upols_update_impulse(neo_hip_upols* h, const float* ir, int64_t length, int normalize,
                                             int is_device, int fade_blocks, int curve, void* stream);
/* blocks left of the running fade (0: none), its length (0: none) and the bytes of the second filter
 * bank (0 until the first update; a sparse handle: the spare bank's tables plus the tiles it holds) */
NEO_HIP_API int neo_hip_upols_fade_info(neo_hip_upols* h, int* remaining_blocks, int* fade_blocks, int64_t* bank_bytes);
/* Live filter update of a SPARSE handle (neo_hip_upols_create_sparse): neo_hip_upols_update_filter's
 * definition, curves and guarantees with sparse filters. A is the handle's filter (its kept tiles), B
 * is `filter` [C][P][B+1] under `mask` [C][P][B+1] (nonzero = keep; both host or both device memory,
 * as set_filter_sparse takes them): y_A and y_B are the outputs of two sparse convolvers that had A
 * and B from the start. ALL state is kept: the delay line is dense, so both banks run against the
 * same rows; set_filter_sparse and the set_*_perceptual calls remain the resetting calls. A fade
 * block is one two-bank sparse step (k_upols_sparse_fade_step: a delay-line tile is loaded once if
 * either bank keeps it; neo_hip_upols_sparse_fade_plan gives its bytes) and the finish of the dense
 * fade; its blocks equal the dense handle's fade on the zeroed filters bit for bit (same splits, up to
 * the sign of zero), the blocks after it a sparse handle's that had B from the start (overlap-add:
 * from the second block after the fade on). While a fade has blocks left every whole block of
 * every process call is one fade step, whatever set_batch says; batched passes after it use B's
 * window bitmaps. The spare bank's tables, the slabs [C][splits][2][B] and (overlap-add) a second
 * set of tails come from the pool at the first update and are kept; B's tiles are sized by its kept
 * tiles and so are allocated per update (none for a mask that keeps nothing: the fade to silence).
 * The retired bank's tiles go back to the pool at the next update, resetting filter call, reset or
 * destroy.
 * STREAM CONTRACT: as neo_hip_upols_update_filter, with ONE difference: the call is NOT asynchronous,
 * even with device memory. It waits on `stream` (never on the device) for the three counts that
 * size B's tiles, as set_filter_sparse does; the perceptual forms wait once more for their scratch.
 * EINVAL, the handle unchanged: a null argument; a handle that is not sparse; before a filter is
 * set; fade_blocks < 1 or > 2^20; curve not 0 or 1; while a fade has blocks left.
 * set_filter_sparse / set_*_perceptual cancel a running fade; reset completes it; set_batch keeps it. */
NEO_HIP_API int neo_hip_upols_update_filter_sparse(neo_hip_upols* h, const void* filter, const uint8_t* mask, int is_device,
                                                   int fade_blocks, int curve, void* stream);
/* The same with the mask made on the device from `filter` by the perceptual predicate (the threshold
 * knob: the same filter under another neo_hip_perceptual), and from an impulse response ir
 * [C][length] (normalize_impulse if `normalize`, uniform_partition, mask, tiles: another impulse
 * response while audio runs). Also EINVAL: parameters neo_hip_perceptual_weights refuses; a length
 * that gives another partition count than the handle's. */
NEO_HIP_API int neo_hip_upols_update_filter_perceptual(neo_hip_upols* h, const void* filter, const neo_hip_perceptual* p,
                                                       int is_device, int fade_blocks, int curve, void* stream);
NEO_HIP_API int neo_hip_upols_update_impulse_perceptual(neo_hip_upols* h, const float* ir, int64_t length, int normalize,
                                                        const neo_hip_perceptual* p, int is_device, int fade_blocks,
                                                        int curve, void* stream);
/* What a sparse fade will cost, before a handle exists (host only): masks A and B [C][P][B+1] -> the
 * kept tiles of A, of B and of A | B, the splits of a sparse handle of that shape with default
 * options, and the model bytes of one fade step: 128 (tiles_a + tiles_b + tiles_union) + both banks'
 * bitmap words and offsets 2 C P (NW + 1) 4 + the inserted row C B 8 + the slabs, written and read,
 * 2 C splits 2 B 8 + the block in and out 2 C B 4. Outputs may be null. */
NEO_HIP_API int neo_hip_upols_sparse_fade_plan(const uint8_t* mask_a, const uint8_t* mask_b, int channels, int block,
                                               int partitions, int64_t* tiles_a, int64_t* tiles_b, int64_t* tiles_union,
                                               int* splits, int64_t* step_bytes);
/* Streaming levels for single-block steps (upols / upola; upols_levels.hip): the
 * partitions are cut into bands -- p in [0, 8) MAC'd by the block itself; Toeplitz windows
 * of 4 / 8 / 16 / 32 blocks for [8, 16) / [16, 32) / [32, 64) / [64, 256); for [256, P) a
 * 128-block partition-axis transform (or, by neo_hip_upols_opts.far_level, a Toeplitz window
 * of 128 blocks) -- and every band's contribution to the
 * blocks of its next window is computed during the current window, a slice of the columns
 * per block step, so every call does the same work (ONE launch per block, k_lvl_step: the
 * block and the slices side by side). Output is the same block by
 * block (summation order differs), latency stays one block. Default on from 64 partitions
 * (B <= 1024); v2 handles refuse it. Switching is allowed at any block boundary (the next
 * step computes the current windows whole). */
NEO_HIP_API int neo_hip_upols_set_ahead(neo_hip_upols* h, int enable);
/* enabled, block position in the current far window, longest window, number of levels */
NEO_HIP_API int neo_hip_upols_get_ahead(neo_hip_upols* h, int* enabled, int* phase, int* window, int* levels);
/* The level plan for `partitions` (no device needed): the block step takes [0, a0);
 * Toeplitz level l < nlevels has a window of T[l] blocks and the band [a[l], b[l]);
 * nseg far segments of 128 partitions from 256 (arrays of >= 5 entries); the automatic
 * choice of far_level. */
NEO_HIP_API int neo_hip_upols_level_plan(int partitions, int* a0, int* nlevels, int* T, int* a, int* b, int* nseg);
/* The step groups' background plan for (channels, block, partitions, step_group; 0 = automatic)
 * with default options (no device needed; for tests): phi[l], the window offset of Toeplitz level
 * l (its windows start at t0 + W T - phi: a level of 4 G <= T <= 32 blocks starts half a window
 * later, so the groups where the levels skip fall apart); the cycle length in step groups; the unit
 * cuts of every background level in level order, cycle / (T / G) windows of T / G cuts each, into
 * cuts[cuts_cap] (*ncuts = how many there are); the predicted background bytes per step group of
 * the cycle into loads[loads_cap]. uniform != 0: equal parts and no offsets (for comparison). */
NEO_HIP_API int neo_hip_upols_part_plan(int channels, int block, int partitions, int step_group, int uniform, int* phi,
                                        int* cycle, int* cuts, int cuts_cap, int* ncuts, double* loads, int loads_cap);
/* The staggered plan (neo_hip_upols_opts.windows = 2) of a (channels, block, partitions) convolver
 * with step groups of step_group blocks (0: the automatic group; 2, 4 or 8) and far window group
 * far_group (0: auto), no device needed; for tests. Per level l < *nlevels its window T[l], band
 * [a[l], b[l]) and staggered[l] (1: T >= 4 G, cut into T / G classes of channels, band from T + 4 G; 0: as in
 * the aligned plan); *far_a, the far level's first partition, and its *nseg segments of 128;
 * *even_share, the even classes' share of a pair of classes in 1/1024ths (the far level's; every
 * level has its own, chosen so that odd and even groups carry the same bytes). Then for every staggered
 * level in level order, and last for the far level (if any), T / G + 1 channel cuts into
 * cuts[cuts_cap] (*ncuts = how many there are in all): class k = channels [cut[k], cut[k + 1]) is
 * computed in the background launches of the groups g = k mod T / G, for its window that starts at
 * block (g + 2) G -- offs[] holds that start modulo T beside the class's first cut (0 beside a
 * list's last cut). The far level's phase 1 of a class runs two groups before. loads[loads_cap]: the
 * predicted background bytes per group of the far window (*nloads = 128 / G). */
NEO_HIP_API int neo_hip_upols_stagger_plan(int channels, int block, int partitions, int step_group, int far_group,
                                           int* nlevels, int* T, int* a, int* b, int* staggered, int* far_a, int* nseg,
                                           int* even_share, int* cuts, int* offs, int cuts_cap, int* ncuts, double* loads,
                                           int loads_cap, int* nloads);
/* Paced background work (step groups only; a no-op with one launch per block): enable = 1 issues
 * the step group's background launch in G pieces, one per call, and every block waits for the
 * piece of the call before it; enable = 2 issues it in two pieces, at the group's calls 0 and
 * G / 2, and those calls' blocks wait for the piece before. Either way no call waits for more
 * than one piece of background work, so the host round trip per block is even (p99 near p50)
 * instead of one call in 2 G paying for two groups' launches. Same outputs; costs one
 * cross-stream wait per piece. 0 = off. The levels re-prime when it changes. */
NEO_HIP_API int neo_hip_upols_set_paced(neo_hip_upols* h, int enable);
/* Latency mode for latency-bound shapes (up to 16 channels; C3, and the reference benchmark's
 * one channel at B = 4096): ONE persistent kernel per handle steps every block. With the
 * streaming levels (64 partitions and up, blocks up to 512, the far level included) it runs their
 * block and slice roles, the Toeplitz levels' slices beside the caller's next block instead of
 * before it; without them (fewer than 64 partitions, any block up to 4096) the plain fused step.
 * A call writes the block's record to a mailbox in mapped host memory and spins until the kernel
 * reports the block done: no launch and no stream wait per block. Every process call is then
 * SYNCHRONOUS (complete on return; the stream argument is not used) and device inputs must be
 * ready when it is made. The kernel leaves after idle_ms without a block (the next call
 * relaunches it) and whenever a setup call (set_filter, set_impulse, reset, set_ahead,
 * set_persistent(0), destroy) runs. Outputs equal the normal step's bit for bit (the same sums in
 * the same order; the levels re-prime on entry and exit). Not available: EINVAL names the
 * reason. */
NEO_HIP_API int neo_hip_upols_set_persistent(neo_hip_upols* h, int enable, double idle_ms);
/* requested, kernel resident now, persistent launches so far */
NEO_HIP_API int neo_hip_upols_get_persistent(neo_hip_upols* h, int* enabled, int* running, int64_t* launches);
/* GPU time of the last min(63, cap) latency-mode steps, oldest first, in us: from the kernel
 * reading the block's record to its completion signal (both on the GPU clock) */
NEO_HIP_API int neo_hip_upols_persist_step_times(neo_hip_upols* h, double* us, int64_t cap, int64_t* count);
/* windows per far phase-1 pass the handle runs (neo_hip_upols_opts.far_group or the automatic
 * choice); 0 without a far transform level */
NEO_HIP_API int neo_hip_upols_get_far_group(neo_hip_upols* h, int* windows);
/* the form of the handle's p >= 256 band: 0 none, 1 partition-axis transform with stored segment
 * and row-pair spectra (far phase 1 + 2), 2 the same transform recomputed every window from the
 * filter and FDL rows (neo_hip_upols_opts.far_level 2), 3 the
 * 128-block Toeplitz level (far_level 0) */
NEO_HIP_API int neo_hip_upols_get_far_form(neo_hip_upols* h, int* form);
/* steps per background launch of the streaming levels' slices (neo_hip_upols_opts.step_group or
 * the automatic choice): 1 = one launch per step */
NEO_HIP_API int neo_hip_upols_get_step_group(neo_hip_upols* h, int* steps);
/* the level windows the handle runs: 1 aligned, 2 staggered (neo_hip_upols_opts.windows or the
 * automatic choice) */
NEO_HIP_API int neo_hip_upols_get_windows(neo_hip_upols* h, int* windows);
/* make `stream` wait (device-side, no host wait) for every background slice launch of the
 * handle's step groups issued so far; a no-op with one launch per step. Outputs never need
 * it (a block's launch already waits for the slices it reads); a caller bracketing steps with
 * events on `stream`, or reusing the device's bandwidth right after, does. No reference
 * counterpart: the reference's operator() is synchronous (uniform_partitioned_convolver.hpp:47-65). */
NEO_HIP_API int neo_hip_upols_join_background(neo_hip_upols* h, void* stream);
/* the background stream of the handle's step groups (a hipStream_t), null while there is none:
 * before the first grouped step, with one launch per step and in latency mode. For tests and
 * tools that enqueue work of their own on it to shift the two streams against each other. Any
 * setup call (filter, options, set_ahead, set_persistent, destroy) may destroy the stream, so a
 * caller fetches it again after one. */
NEO_HIP_API int neo_hip_upols_get_background_stream(neo_hip_upols* h, void** stream);
/* -- Multichannel convolver over several devices ------------------------------
 * C channels cut into n contiguous shards, shard i = channels [C i / n, C (i + 1) / n) on
 * devices[i] (a device may repeat), each a neo_hip_upols handle of its own (own stream).
 * The reference steps all channels of a plugin instance in one loop
 * (extra/plugin/src/dsp/DenseConvolution.hpp:35,50-67); channels never interact, so there is
 * no collective: every call below fans out to the shards concurrently (one host thread per
 * shard) and returns when all are done. Shard results equal those of one handle over all
 * channels within float summation order: the shape-based code-path choices (far window
 * group, Toeplitz window parts, fused step, splits) follow each shard's own channel count;
 * they are bit for bit equal where those choices coincide (the same opts force them).
 * method / opts as neo_hip_upols_create_ex. */
typedef struct neo_hip_upols_multi neo_hip_upols_multi;
NEO_HIP_API int neo_hip_upols_multi_create(int channels, int block, int partitions, const int* devices, int ndevices,
                                           int method, const neo_hip_upols_opts* opts, neo_hip_upols_multi** m);
NEO_HIP_API int neo_hip_upols_multi_destroy(neo_hip_upols_multi* m);
NEO_HIP_API int neo_hip_upols_multi_shards(neo_hip_upols_multi* m, int* nshards);
/* shard i: its handle (for device-resident I/O with neo_hip_upols_process_device /
 * process_blocks on that device), device, first channel and channel count */
NEO_HIP_API int neo_hip_upols_multi_shard(neo_hip_upols_multi* m, int i, neo_hip_upols** h, int* device,
                                          int* first_channel, int* channels);
/* filter [C][P][B+1] complex, host memory; resets all state */
NEO_HIP_API int neo_hip_upols_multi_set_filter(neo_hip_upols_multi* m, const void* filter);
/* ir [C][length] float, host memory; normalize: one factor over all C channels
 * (normalize_impulse.hpp:21-30), as a single handle would */
NEO_HIP_API int neo_hip_upols_multi_set_impulse(neo_hip_upols_multi* m, const float* ir, int64_t length, int normalize);
/* num_samples per channel (channel c at in + c*ld_in / out + c*ld_out, in == out allowed),
 * host memory, synchronous; block rules as neo_hip_upols_process_samples */
NEO_HIP_API int neo_hip_upols_multi_process_samples(neo_hip_upols_multi* m, const float* in, int64_t ld_in, float* out,
                                                    int64_t ld_out, int64_t num_samples);
NEO_HIP_API int neo_hip_upols_multi_reset(neo_hip_upols_multi* m);
/* Live filter updates (neo_hip_upols_update_filter / _update_impulse) on every shard, host memory,
 * each shard on its own stream; complete on return. For an impulse the normalisation factor is
 * taken once over all C channels, as neo_hip_upols_multi_set_impulse takes it. A refusal by one
 * shard is a refusal by all: every shard checks the same conditions. */
NEO_HIP_API int neo_hip_upols_multi_update_filter(neo_hip_upols_multi* m, const void* filter, int fade_blocks, int curve);
NEO_HIP_API int neo_hip_upols_multi_update_impulse(neo_hip_upols_multi* m, const float* ir, int64_t length, int normalize,
                                                   int fade_blocks, int curve);
/* -- Groups of single-channel convolvers (upols_group.hip) ---------------------------------
 * Members are C independent one-channel upols / upola convolvers of one shape, each with its
 * own filter and state, as the plugin's std::vector<upols_convolver> (DenseConvolution.hpp:35)
 * holds them; process(member, io) is that member's operator()(block): one block of B samples,
 * host memory, in place, complete on return. A group belongs to ONE owner (one plugin
 * instance's convolvers; C++: neo::convolution::convolver_group). While the callers follow the
 * plugin's frame pattern (every member called once per frame on a buffer of its own that it
 * reuses) AND every member's buffer lies in a range the owner registered AND the members' shape
 * runs the streaming levels (64 partitions and up, blocks up to 1024), the group steps every
 * member in ONE launch at a frame's first call, from the blocks in the other members'
 * registered buffers, and later calls only verify their block (a different block re-runs that
 * member's block step alone); any other pattern runs each member on a handle of its own. Either
 * way each member's outputs are those of its own sequential convolver (up to float summation
 * order after a mode switch, which re-primes the streaming levels). The group never reads a
 * buffer outside the registered ranges. method 0 upols, 1 upola. */
typedef struct neo_hip_upols_group neo_hip_upols_group;
NEO_HIP_API int neo_hip_upols_group_create(int block, int partitions, int method, int device, neo_hip_upols_group** g);
NEO_HIP_API int neo_hip_upols_group_destroy(neo_hip_upols_group* g);
NEO_HIP_API int neo_hip_upols_group_join(neo_hip_upols_group* g, int* member);
NEO_HIP_API int neo_hip_upols_group_leave(neo_hip_upols_group* g, int member);
/* filter [P][B+1] complex (uniform_partition layout of one channel); resets the member's state */
NEO_HIP_API int neo_hip_upols_group_set_filter(neo_hip_upols_group* g, int member, const void* filter, int is_device);
NEO_HIP_API int neo_hip_upols_group_process(neo_hip_upols_group* g, int member, float* io);
NEO_HIP_API int neo_hip_upols_group_reset(neo_hip_upols_group* g, int member);
/* register [ptr, ptr + bytes) of host memory the owner keeps allocated until it unregisters it
 * (e.g. the plugin's frame buffer, ConstantOverlapAdd.hpp:34, between two prepare() calls):
 * only members whose buffers lie in a registered range are stepped ahead of their call.
 * Registering a range again is a no-op (cheap enough per frame). unregister(ptr) removes the
 * range starting at ptr, unregister(NULL) every range; the group then stops reading them
 * before the call returns (a coalesced group splits at its next frame). */
NEO_HIP_API int neo_hip_upols_group_register(neo_hip_upols_group* g, const void* ptr, int64_t bytes);
/* register_ex with flags: NEO_HIP_GROUP_FRAME_STABLE = the owner also promises that during a frame
 * (from its first member call until every member has made its call) nothing but those calls writes
 * the range, as in the plugin's loop over the channels of a filled frame (DenseConvolution.cpp:62-74).
 * A frame read in place from such a range then skips the leader's snapshot of every member's block
 * and the members' comparisons with it: a member's call on the buffer the step read is the copy of
 * its output (a call on another buffer re-runs that member's block step, exact). Without the flag
 * (register) each member's block is compared exactly and re-stepped on a difference. Registering the
 * same range again updates its flags. */
#define NEO_HIP_GROUP_FRAME_STABLE 1
/* NEO_HIP_GROUP_FRAME_INPLACE (implies STABLE): the owner also reads or writes a member's block only
 * through that member's call, every member on the same block of the range every frame -- exactly
 * processFrame's loop. The frame's first call then writes EVERY member's output into its block in
 * place, and a later member's call has nothing left to do. A member called on another buffer is
 * still stepped exactly (its own block step again), but its speculative output was written to its
 * old block: that is the promise the flag makes.
 * Under the in-place promise a frame's blocks are consumed at its first call, and a state change in
 * mid-frame takes effect after them: when set_filter, reset, join, leave or a second call of a member
 * ends the one-launch mode while members have not made their call of the frame yet, their blocks hold
 * their outputs already (the inputs are gone, so no member is stepped back), each one's remaining call
 * of the frame on its block returns at once, and a new filter or a reset of such a member starts with
 * its next frame (a member that leaves takes its consumed block with it). Called on another buffer
 * instead, such a member is stepped on it as a NEW block: the owner broke the in-place promise.
 * Without the flag (plain or STABLE) the inputs are still there: those members are stepped back one
 * block and a state change applies where it is made. */
#define NEO_HIP_GROUP_FRAME_INPLACE 2
NEO_HIP_API int neo_hip_upols_group_register_ex(neo_hip_upols_group* g, const void* ptr, int64_t bytes, int flags);
NEO_HIP_API int neo_hip_upols_group_unregister(neo_hip_upols_group* g, const void* ptr);
/* coalesced now; one-launch frame steps, member calls, block re-runs, mode switches so far */
NEO_HIP_API int neo_hip_upols_group_stats(neo_hip_upols_group* g, int* coalesced, int64_t* frame_steps, int64_t* calls,
                                          int64_t* redos, int64_t* switches);
/* -- Matrix (multi-input, multi-output) convolver (upols_matrix.hip) ---------------------------
 * I inputs, O outputs and a list of ROUTES: a route is a pair (out, in) with a filter [P][B+1]
 * complex in uniform_partition layout. Output o is the sum over its routes of what the reference's
 * upols_convolver (method 0) / upola_convolver (method 1) gives for (x_in, that route's filter);
 * the reference itself has no such class (its plugin runs one convolver per channel,
 * extra/plugin/src/dsp/DenseConvolution.hpp:35). The route list is unique pairs in any order (the
 * results do not depend on the order); a dense matrix is the list of all O * I pairs. An output
 * with no route produces zeros, and an input reaches only the outputs it has a route to (an Inf or
 * NaN in it does not touch the others); an input with no route is accepted. Overlap-save keeps its window
 * state per input, overlap-add its overlap tail per output. One delay line per input serves every
 * output, the sum over the inputs is taken on spectra, and there is one inverse transform per
 * output. A block step is two launches: the inputs' windows and transforms, then the plain step's
 * MAC over (tiles of outputs) x (splits of the tile's rows), where a TILE is up to out_tile
 * consecutive outputs that share each FDL row load. Equal calls with equal options give equal bits.
 * Batched passes are the handle's second gear (neo_hip_matrix_set_batch below): with the blocks of a
 * call known up front, up to 32 of them share one pass over every route's filter. Offline windows
 * are the third (neo_hip_matrix_set_offline below): windows of 128 blocks by 256-point transforms
 * along the block axis, for long filters with every block of a call known up front. A filter
 * changes in one of two ways: neo_hip_matrix_set_filter / _set_impulse take a new route list and
 * RESET all state; neo_hip_matrix_update_filter / _update_impulse (below) keep the route list and
 * ALL state and crossfade to the new filter while audio runs. Window levels
 * (neo_hip_matrix_set_levels below) are the gear for long filters with ONE block per call: only the
 * first partitions are read on every block, the rest once per window of 8 or 32 blocks, one window
 * ahead of time. The dense handle's streaming levels (a background stream),
 * latency mode, sub-block input (method 2), groups and the multi-device convolver
 * do not apply to this handle type (DESIGN 5.8 has the measurements of both forms). */
typedef struct neo_hip_matrix neo_hip_matrix;
typedef struct neo_hip_matrix_opts {
    int fused;            /* -1 auto (one MAC launch with the last-arriver tail up to 64 workgroups, tiles x splits),
                             0 MAC + finish, 1 the last split of a tile to arrive runs its tails */
    int split_workgroups; /* 0 auto (about 1024 workgroups, >= 8 rows per split; 16 for the fused form up to
                             B = 512), else the workgroup target for the splits, taken as given (up to 64 per tile) */
    int out_tile;         /* outputs per workgroup: 0 auto (4 at B = 512 for 8 tiles or more whose outputs all take
                             every input of their tile, from 2048 rows per tile: the measured range, DESIGN
                             5.8; otherwise 1), else 1, 2 or 4; clamped to 4 for B <= 512, 2 for
                             B = 1024 and 1 above (the accumulators of a tile stay in registers); info and plan
                             report the value in use */
} neo_hip_matrix_opts;
/* method 0 = overlap-save, 1 = overlap-add (2 is EINVAL); opts NULL = all defaults. The shape, the
 * method and the options are checked before a device is touched. */
NEO_HIP_API int neo_hip_matrix_create(int inputs, int outputs, int block, int partitions, int device, int method,
                                      const neo_hip_matrix_opts* opts, neo_hip_matrix** m);
NEO_HIP_API int neo_hip_matrix_destroy(neo_hip_matrix* m);
/* filter [nroutes][P][B+1] complex, host or device memory; route r = (route_out[r], route_in[r]),
 * both arrays ALWAYS in host memory. A duplicate route, an index out of range or nroutes < 1 is
 * EINVAL and leaves the handle as it was. Resets all state, like filter(). The call waits on the
 * handle's stream only. */
NEO_HIP_API int neo_hip_matrix_set_filter(neo_hip_matrix* m, const void* filter, const int* route_out,
                                          const int* route_in, int nroutes, int is_device);
/* ir [nroutes][length] float, host or device memory: normalize_impulse over all routes' rows (one
 * factor, as neo_hip_upols_set_impulse takes it over channels) if `normalize`, then
 * uniform_partition on the device; otherwise as set_filter. */
NEO_HIP_API int neo_hip_matrix_set_impulse(neo_hip_matrix* m, const float* ir, int64_t length, const int* route_out,
                                           const int* route_in, int nroutes, int normalize, int is_device);
/* nblocks consecutive single-block steps (batched passes with neo_hip_matrix_set_batch): input i at in + i*ld_in, output o at out + o*ld_out, block
 * t of either at + t*B. Device memory: asynchronous on `stream` (NULL = the HIP null stream), both
 * pointers 16-byte aligned, ld_in and ld_out multiples of 4; host memory: staged, synchronous (the
 * handle's stream if `stream` is NULL), any alignment. ld_in and ld_out >= nblocks * B. A refused
 * call (EINVAL) leaves the state as it was. Every read of a block of `in` happens before the first
 * write of that block of `out`, so in == out (same strides, I == O) is allowed, and for one block
 * the two may overlap in any way. EINVAL before the first set_filter / set_impulse. */
NEO_HIP_API int neo_hip_matrix_process(neo_hip_matrix* m, const float* in, int64_t ld_in, float* out, int64_t ld_out,
                                       int64_t nblocks, int is_device, void* stream);
/* Clears all state. A running fade (below) completes: the new filter is the filter. */
NEO_HIP_API int neo_hip_matrix_reset(neo_hip_matrix* m);
/* Live filter update: crossfade from the handle's filter A to `filter` (B) over the next fade_blocks
 * blocks, keeping ALL state (delay lines, overlap-save windows, overlap-add tails); set_filter
 * remains the resetting call. filter [nroutes][P][B+1] complex in the route order of the last
 * set_filter / set_impulse; the route list does not change (a route that is to vanish gets zeros).
 * With y_A, y_B the outputs of two convolvers with filters A and B fed the whole input from the
 * start, sample n = 0 .. fade_blocks * B - 1 of the next fade_blocks blocks is
 * y_A + g[n] (y_B - y_A) (the kernel's form of (1 - g) y_A + g y_B), g as neo_hip_matrix_fade_gains
 * gives it; every block after them is y_B, bit for bit what a handle that had B from the start
 * gives (overlap-add: from the second block after the fade on; the first takes a tail summed in the
 * fade kernel's order). The new filter is packed into a second bank, allocated at the first update
 * after a set_filter / set_impulse (neo_hip_matrix_fade_info reports it; beside it the fade's slabs
 * [O][splits][2][B] and, overlap-add, a second set of tails [O][B]); no update re-plans or
 * re-allocates after that. While a fade has blocks left, neo_hip_matrix_process runs them as single
 * fade steps (three launches: the inputs' windows, both banks against the same delay-line rows, two
 * inverse transforms and the mix per output) whatever set_batch / set_offline say, then swaps the
 * banks and goes on in passes. Equal calls give equal bits.
 * STREAM CONTRACT: `stream` must be the stream the caller's neo_hip_matrix_process calls run on, or
 * be ordered with it (after every earlier process call, before every later one): the update reads
 * the delay lines those calls write (overlap-add) and writes the bank the later ones read. Device
 * pointer: asynchronous on `stream` (NULL = the HIP null stream). Host pointer: staged on `stream`
 * (NULL = the handle's stream, as host process calls) after the handle's earlier steps on any
 * stream; returns when the bank is written.
 * EINVAL, the handle unchanged: before a filter is set, fade_blocks < 1, curve not 0 (linear) or 1
 * (raised cosine), or while a fade has blocks left. set_filter / set_impulse cancel a running fade
 * (and free the second bank: the route list may change); set_batch / set_offline keep it. */
NEO_HIP_API int neo_hip_matrix_update_filter(neo_hip_matrix* m, const void* filter, int is_device, int fade_blocks,
                                             int curve, void* stream);
/* The same from ir [nroutes][length] float (host or device): normalize_impulse over all routes' rows
 * if `normalize`, then uniform_partition on the device into the second bank, as set_impulse does. */
NEO_HIP_API int neo_hip_matrix_update_impulse(neo_hip_matrix* m, const float* ir, int64_t length, int normalize,
                                              int is_device, int fade_blocks, int curve, void* stream);
/* blocks left of the running fade (0: none), its length (0: none) and the bytes of the second filter
 * bank (0 until the first update after a filter; then neo_hip_matrix_desc.filter_bytes) */
NEO_HIP_API int neo_hip_matrix_fade_info(neo_hip_matrix* m, int* remaining_blocks, int* fade_blocks, int64_t* bank_bytes);
/* Host only: the fade_blocks * block gains g[n] of a fade, t = n / (fade_blocks * block): curve 0
 * g = t, curve 1 g = 0.5 - 0.5 cos(pi t), evaluated in float64 and rounded to float32; the kernel
 * evaluates the same expression. EINVAL for a block that is no power of two in [16, 4096],
 * fade_blocks < 1 (or > 2^20) and an unknown curve. */
NEO_HIP_API int neo_hip_matrix_fade_gains(int block, int fade_blocks, int curve, float* g);
/* what the handle runs; routes, tiles, out_tile, splits, fused and filter_bytes are 0 until a filter is set */
typedef struct neo_hip_matrix_desc {
    int inputs, outputs, block, partitions, method;
    int routes, tiles, out_tile, splits, fused;
    int64_t filter_bytes; /* [routes][P][B] packed */
    int64_t fdl_bytes;    /* [inputs][ring rows][B]: P rows, P + 31 once batching was turned on, at least
                             128 (ceil(P / 128) + 2) + 1 once offline windows were */
    int64_t offline_bytes; /* the buffers of the offline windows (segment, pair and output spectra, overlap-add
                              tails), 0 until the first offline pass after a filter allocates them */
} neo_hip_matrix_desc;
NEO_HIP_API int neo_hip_matrix_info(neo_hip_matrix* m, neo_hip_matrix_desc* desc);
/* Batched passes. enable = 1: neo_hip_matrix_process cuts a call into the largest power-of-two
 * passes <= 32 of the blocks left (95 blocks: 32, 32, 16, 8, 4, 2 and one single step); a pass of T
 * blocks is the inputs' T window transforms, ONE walk over every route's filter with T accumulators
 * per bin (k_matrix_batch_mac: one output per workgroup, the sum over the inputs taken on spectra,
 * fixed order, no atomics: equal calls give equal bits and the order of the route list plays no
 * part), and T inverse transforms per output. Results equal those of single steps up to summation
 * order; every read of the T blocks of `in` still happens before the first write of those blocks of
 * `out`. Turning batching on grows every input's ring from P to P + 31 rows: the call joins the
 * handle's streams and re-lays the live rows, so a stream continues across it; turning it off keeps
 * the larger ring (single steps then give the bits they gave before). Batched passes and single
 * steps mix freely at block boundaries. split_workgroups: 0 automatic (about 512 workgroups,
 * outputs x splits x bin chunks, with at least 32 rows in every split of the longest output), else
 * the workgroup target, taken as given (up to 64 splits per output). enable other than 0 / 1 or a
 * negative target is EINVAL and leaves the state untouched. The slabs of the passes are allocated
 * at the first batched pass and freed with the filter. Default: off. */
NEO_HIP_API int neo_hip_matrix_set_batch(neo_hip_matrix* m, int enable, int split_workgroups);
/* blocks_per_pass 32 (batching on) or 1; splits per output of a pass (0 until a filter is set or
 * with batching off); the rows of every input's ring. Each pointer may be NULL. */
NEO_HIP_API int neo_hip_matrix_batch_info(neo_hip_matrix* m, int* blocks_per_pass, int* splits, int* ring_rows);
/* The plan of a batched pass of `blocks` (2, 4, 8, 16 or 32) blocks for a route list, on the host (no
 * device needed; the handle is built from the same function). Output o's row list is its inputs
 * (ascending) x partitions 0..P-1, flattened, out_rows[o] rows; split s of its `splits` walks rows
 * [s rows / splits, (s + 1) rows / splits) as a list of RUNS: run k covers partitions [run_first[k],
 * run_last[k]) of input run_in[k], and the runs of split s of output o are k in [run_off[65 o + s],
 * run_off[65 o + s + 1]). A run of n rows loads n filter rows and n + blocks - 1 FDL rows (its window).
 * Per pass: filter_row_loads (routes x P), fdl_row_loads, slab_rows (outputs x splits x blocks,
 * written once and read once), and bytes = 8 B (filter + FDL rows + 2 slab rows) + 4 B blocks
 * (inputs + outputs). Arrays (each may be NULL): out_rows [outputs], run_off [outputs][65], run_in,
 * run_first, run_last [nroutes + 63 * outputs]. */
typedef struct neo_hip_matrix_batch_plan_info {
    int blocks, splits, chunks, runs; /* chunks: workgroups per row (B / 256 above 256 bins) */
    int64_t filter_row_loads, fdl_row_loads, slab_rows, bytes;
} neo_hip_matrix_batch_plan_info;
NEO_HIP_API int neo_hip_matrix_batch_plan(int inputs, int outputs, int block, int partitions, const int* route_out,
                                          const int* route_in, int nroutes, int blocks, int split_workgroups,
                                          neo_hip_matrix_batch_plan_info* plan, int* out_rows, int* run_off, int* run_in,
                                          int* run_first, int* run_last);
/* Offline windows, for long filters when every block of a call is known up front (a file render, a
 * matrix over a dataset). enable = 1: while neo_hip_matrix_process has 256 blocks or more left it
 * runs a pass of two windows of 128 blocks (windows_per_pass 0 = automatic = 2, or 2), else while 128
 * or more are left a pass of one window (windows_per_pass 1: one-window passes only); the rest of
 * the call goes as without it (batched passes if batching is on, else single steps). Per bin, the
 * blocks t_W + j (j < 128) of a window are samples 128 + j of IDFT256 of the sum, over the output's
 * routes (o, i) in ascending input order and the segments q < ceil(P / 128) of 128 partitions, of
 * DFT256(ring rows t_W - 128 (q + 1) ... + 255 of input i) . DFT256(segment q of the route's
 * filter, zero past P): forward transforms per input, inverse transforms per output, per route only
 * the spectrum products; fixed order, no atomics, equal calls give equal bits and the order of the
 * route list plays no part. Results equal those of single steps up to rounding. Every read of the
 * pass's blocks of `in` happens before the first write of those blocks of `out`. Turning it on joins
 * the handle's streams and re-lays every input's ring in at least 128 (ceil(P / 128) + 2) + 1 rows
 * (the larger of this and P + 31 with batching), so a stream continues across it; a ring that would
 * span 2 GiB or more per input is EINVAL. Turning it off keeps the larger ring (the other passes then
 * give the bits they gave before). All kinds of pass mix freely at block boundaries, across calls
 * and across toggling. enable other than 0 / 1 or windows_per_pass other than 0, 1, 2 is EINVAL and
 * leaves the state untouched. The spectra ([routes][segments][256][B] of the filters: as large as
 * the filters rounded up to 256 rows per 128 partitions, recomputed at the first offline pass after
 * every set_filter / set_impulse) and the pass buffers are allocated at the first offline pass and
 * freed with the filter; if that allocation fails the call returns ENOMEM and the handle goes on
 * with batched passes and single steps. Default: off.
 * Inf / NaN: the 256-point transforms mix the rows of a pair, and the zero-padded last segment
 * meets rows older than the filter reaches. So a non-finite input block makes EVERY block of every
 * window whose pairs hold it non-finite, on the outputs routed from that input: count on every
 * block of every pass from the one containing the block up to the last pass with
 * t_W - 128 ceil(P / 128) <= that block (as on a neo_hip_upols handle's offline windows), and with
 * overlap-add on the first block after them, which takes the last one's overlap tail. Outputs with
 * no route from that input are untouched, bit for bit. */
NEO_HIP_API int neo_hip_matrix_set_offline(neo_hip_matrix* m, int enable, int windows_per_pass);
/* blocks_per_pass 256 or 128 (offline windows on; 0 off); segments = ceil(P / 128); the rows of every
 * input's ring; the payload bytes of the segment spectra (0 until allocated). Each pointer may be NULL. */
NEO_HIP_API int neo_hip_matrix_offline_info(neo_hip_matrix* m, int* blocks_per_pass, int* segments, int* ring_rows,
                                            int64_t* spectra_bytes);
/* The plan of an offline pass, on the host (no device needed; the pass takes its rows from the same
 * function): `windows` (0 = 2, 1, 2) windows at ring row write_pos of a ring of ring_rows rows (0 =
 * min_ring_rows, the least a handle takes). A PAIR is 256 consecutive ring rows (mod ring_rows):
 * pair_row[k], k < pairs = segments + windows - 1, is the first row of pair k (k = 0 the newest) and
 * pair_of[window * segments + q] the pair that segment q of that window multiplies. hf_bytes and
 * xf_bytes: the payloads of the segment spectra [routes][segments][256][B] and of the pass's pair
 * spectra [inputs][pairs][256][B]. The model of a pass, in rows of 8 B bytes: spectrum_rows (routes x
 * segments x 256, read once), pair_cache_rows (routes x pairs x 256: the pair spectra re-read by
 * every route, expected from L2 / Infinity Cache), fdl_rows and pair_rows_written (inputs x pairs x
 * 256 each), output_rows (outputs x 128 windows, written and read: x 2); bytes = 8 B times their sum
 * + 4 B blocks_per_pass (inputs + outputs), of which cache_bytes = 8 B pair_cache_rows. Arrays (each
 * may be NULL): pair_row [segments + 1], pair_of [2][segments] (only `windows` rows are written). */
typedef struct neo_hip_matrix_offline_plan_info {
    int segments, windows, blocks_per_pass, pairs, min_ring_rows, ring_rows;
    int64_t hf_bytes, xf_bytes;
    int64_t spectrum_rows, pair_cache_rows, fdl_rows, pair_rows_written, output_rows;
    int64_t bytes, cache_bytes;
} neo_hip_matrix_offline_plan_info;
NEO_HIP_API int neo_hip_matrix_offline_plan(int inputs, int outputs, int block, int partitions, const int* route_out,
                                            const int* route_in, int nroutes, int windows, int write_pos, int ring_rows,
                                            neo_hip_matrix_offline_plan_info* plan, int* pair_row, int* pair_of);
/* Window levels: long filters in real time (one block per call). enable = 1: a single step reads
 * only the HEAD, partitions [0, 2 T0), per block (the ordinary step on a compact second bank
 * [routes][2 T0][B], copied from the filter at the first level step after a filter or a fade). A LEVEL
 * with window length T (`windows`: ascending powers of two from 2, 4, 8, 16, 32, each at least twice
 * the one before; NULL: the default 8, 32) takes the band of partitions [2 T, 2 T_next), the last level up
 * to P; a level whose band is empty is dropped, and with P <= 2 T0 there is no level and the handle
 * runs the ordinary step. n counts the blocks since the last reset (on every path); window W of a
 * level is the blocks [W T, W T + T). The level's contribution to the T blocks of a window is one
 * batched MAC over its band (k_matrix_lvl_mac), whose workgroups are cut into T parts of equal count:
 * block n launches part n mod T of window n / T + 1 on the caller's stream, so every call does the
 * same work, and a finish launch sums the head's slabs and row n mod T of every level's current
 * window in a fixed order (head splits, then levels by T, splits ascending) and runs the inverse
 * transform. Equal calls give equal bits; no atomics. Any block that runs without the parts (a
 * batched or offline pass, a fade step, a step with the mode off) and a filter that changed (the end
 * of a fade) leave the slabs stale; the next level step PRIMES them first (every level's current
 * window whole, then the due parts of the next) and gives the bits the parts run in their turn
 * would have given. Precedence in neo_hip_matrix_process: fade steps, offline windows, batched
 * passes, then level steps. The ring stays at P rows (the schedule, priming included, never reads a
 * row older than the ordinary step does). split_workgroups: the workgroup target of one PART (0
 * automatic: 512, and no split of the longest output shorter than T rows; else taken as given), at
 * most 64 splits per output. Allowed at any time between calls; joins the handle's streams; bad
 * windows are refused and leave the handle as it was. */
#define NEO_HIP_MATRIX_MAX_LEVELS 5
NEO_HIP_API int neo_hip_matrix_set_levels(neo_hip_matrix* m, int enable, const int* windows, int nwindows,
                                          int split_workgroups);
typedef struct neo_hip_matrix_levels_desc {
    int enabled, levels, head; /* levels in use (0: the ordinary step; 0 without a filter), head partitions */
    int window[NEO_HIP_MATRIX_MAX_LEVELS], first[NEO_HIP_MATRIX_MAX_LEVELS], last[NEO_HIP_MATRIX_MAX_LEVELS];
    int splits[NEO_HIP_MATRIX_MAX_LEVELS]; /* level l: window length, band [first, last), splits per output */
    int ring_rows, primed;     /* rows of every input's ring; 1: the slabs are current */
    int64_t partial_bytes;     /* the levels' double-buffered slabs, sum of 2 O S T rows (as planned) */
    int64_t head_bank_bytes;   /* [routes][head][B] (as planned; allocated at the first level step) */
} neo_hip_matrix_levels_desc;
NEO_HIP_API int neo_hip_matrix_levels_info(neo_hip_matrix* m, neo_hip_matrix_levels_desc* desc);
/* The level plan for a route list, on the host (no device needed; the handle is built from the same
 * function). Per level l < levels: window[l], the band [first[l], last[l]), splits[l] per output,
 * workgroups[l] = outputs x splits x chunks of a window, runs[l], and per WINDOW filter_rows[l]
 * (routes x band) and fdl_rows[l] (per run its length + window - 1). bytes is the model of ONE block:
 * 8 B (the head's filter and FDL row loads + 2 O head_splits slab rows) + per level 8 B (filter_rows +
 * fdl_rows) / window + 8 B 2 O splits (the partial rows written per block and read by the finish) +
 * 4 B (inputs + outputs). Arrays (each may be NULL): part_cut [5][33] (part k of level l is the
 * workgroups [part_cut[33 l + k], part_cut[33 l + k + 1]), workgroup = (output x splits + split) x
 * chunks + chunk); run_off [5][64 outputs + 1] (level l, split s of output o: runs k in [run_off[o S +
 * s], run_off[o S + s + 1]) of that level's row); run_in, run_first, run_last [5][nroutes + 63 outputs]
 * (run k covers partitions [run_first, run_last) of input run_in). */
typedef struct neo_hip_matrix_level_plan_info {
    int levels, head, ring_rows, chunks, head_splits, head_out_tile;
    int window[NEO_HIP_MATRIX_MAX_LEVELS], first[NEO_HIP_MATRIX_MAX_LEVELS], last[NEO_HIP_MATRIX_MAX_LEVELS];
    int splits[NEO_HIP_MATRIX_MAX_LEVELS], workgroups[NEO_HIP_MATRIX_MAX_LEVELS], runs[NEO_HIP_MATRIX_MAX_LEVELS];
    int64_t filter_rows[NEO_HIP_MATRIX_MAX_LEVELS], fdl_rows[NEO_HIP_MATRIX_MAX_LEVELS];
    int64_t head_filter_rows, head_fdl_rows; /* per block */
    int64_t partial_bytes, head_bank_bytes, bytes;
} neo_hip_matrix_level_plan_info;
NEO_HIP_API int neo_hip_matrix_level_plan(int inputs, int outputs, int block, int partitions, const int* route_out,
                                          const int* route_in, int nroutes, const int* windows, int nwindows,
                                          int split_workgroups, neo_hip_matrix_level_plan_info* plan, int* part_cut,
                                          int* run_off, int* run_in, int* run_first, int* run_last);
/* The plan for a route list and options, on the host (no device needed; the handle is built from
 * the same function). Consecutive outputs form tiles of out_tile; a tile's row list is the union
 * of its outputs' inputs (ascending) x partitions 0..P-1, flattened, and split s of the S splits
 * walks rows [cuts[s], cuts[s + 1]) of it. Per step the MAC launch loads fdl_row_loads FDL rows
 * (the sum of the tiles' row counts) and filter_row_loads filter rows (routes x P) of 8 B bytes
 * each; the algorithmic bytes of a step are 8 B (fdl_row_loads + filter_row_loads) plus the block
 * I/O. Arrays (each may be NULL): tile_first, tile_count, tile_rows [outputs]; union_off
 * [outputs + 1] and union_in [outputs * inputs] (tile t's inputs are union_in[union_off[t] ..
 * union_off[t + 1])); cuts [outputs][65] (row 65 t + s). Only the first `tiles` rows are written. */
typedef struct neo_hip_matrix_plan_info {
    int out_tile, fused, splits, tiles;
    int64_t fdl_row_loads, filter_row_loads;
} neo_hip_matrix_plan_info;
NEO_HIP_API int neo_hip_matrix_plan(int inputs, int outputs, int block, int partitions, const int* route_out,
                                    const int* route_in, int nroutes, const neo_hip_matrix_opts* opts,
                                    neo_hip_matrix_plan_info* plan, int* tile_first, int* tile_count, int* tile_rows,
                                    int* union_off, int* union_in, int* cuts);
/* Kernel timing with HIP events recorded on the launch stream (for the roofline in
 * bench.py): enable = n > 0 brackets every n-th launch group with events (0 = off).
 * timing() returns the summed ms of the bracketed part and the count of timed groups:
 * the MAC kernel of a plain or batched step, the whole step of a streaming-level step.
 * timing_detail() returns per part (ms[4], launches[4]): streaming-level steps 0 = the
 * step kernel (step groups: the block launch and the wait for the previous group's slices,
 * 1 = the slice launches on the background stream, one per G steps); plain / batched steps
 * 0 = MAC kernel. Both drain the events. */
NEO_HIP_API int neo_hip_upols_set_timing(neo_hip_upols* h, int enable);
NEO_HIP_API int neo_hip_upols_timing(neo_hip_upols* h, double* mac_ms, int64_t* launches);
NEO_HIP_API int neo_hip_upols_timing_detail(neo_hip_upols* h, double* ms, int64_t* launches);
/* the duration of every timed launch group in order (first to last event; a streaming
 * step: the whole step), up to cap into ms; count = groups recorded. Drains the events. */
NEO_HIP_API int neo_hip_upols_step_times(neo_hip_upols* h, double* ms, int64_t cap, int64_t* count);
NEO_HIP_API int neo_hip_upols_info(neo_hip_upols* h, int* channels, int* block, int* partitions, int* splits);

/* -- standalone overlap stages (overlap_save.hpp:19-112, overlap_add.hpp:23-107) -----------
 * C independent stages of block B (a power of two) for filters of F taps, transform size
 * n = 2^next_order(B + F - 1) (<= 2^27). The reference's operator()(block, callback) split
 * at the callback: forward = window update + rfft -> spectrum [C][n/2 + 1] complex (what the
 * callback sees), inverse = irfft of the (processed) spectrum, 1/n, output block. kind 0 =
 * overlap_save (window slid left by B, block at its end; output = the last B samples), 1 =
 * overlap_add (block at the window's start, [B, 2B) zeroed; output = first B + overlap, the
 * irfft written back into the window as the reference does). Blocks: channel c at in + c*ld.
 * Host memory: synchronous (own stream if NULL); device memory: asynchronous on `stream`. */
typedef struct neo_hip_overlap neo_hip_overlap;
NEO_HIP_API int neo_hip_overlap_create(int kind, int channels, int64_t block, int64_t filter, int device,
                                       neo_hip_overlap** h);
NEO_HIP_API int neo_hip_overlap_destroy(neo_hip_overlap* h);
NEO_HIP_API int neo_hip_overlap_info(neo_hip_overlap* h, int64_t* block, int64_t* filter, int64_t* transform_size);
NEO_HIP_API int neo_hip_overlap_reset(neo_hip_overlap* h);
NEO_HIP_API int neo_hip_overlap_forward(neo_hip_overlap* h, const float* in, int64_t ld_in, void* spectrum,
                                        int is_device, void* stream);
NEO_HIP_API int neo_hip_overlap_inverse(neo_hip_overlap* h, const void* spectrum, float* out, int64_t ld_out,
                                        int is_device, void* stream);

/* -- setup path (uniform_partition.hpp:12-26, normalize_impulse.hpp:11-33) -- */
NEO_HIP_API int neo_hip_num_partitions(int64_t length, int block, int64_t* partitions);
/* ir [C][L] float -> out [C][P][B+1] complex; host or device pointers. */
NEO_HIP_API int neo_hip_uniform_partition(const float* ir, int channels, int64_t length, int block, void* out,
                                          int is_device, int device);
/* in place on ir [C][L]: scale all channels by min_c 1/sqrt(sum ir[c]^2). */
NEO_HIP_API int neo_hip_normalize_impulse(float* ir, int channels, int64_t length, int is_device, int device);

/* the same in double: ir [C][L] double -> out [C][P][B+1] complex double; in place on ir [C][L]
 * double. The energy sum runs in a fixed order that depends on L alone (not the reference's
 * sequential one; the two agree to ~1e-13 relative). */
NEO_HIP_API int neo_hip_uniform_partition_f64(const double* ir, int channels, int64_t length, int block, void* out,
                                              int is_device, int device);
NEO_HIP_API int neo_hip_normalize_impulse_f64(double* ir, int channels, int64_t length, int is_device, int device);

/* -- double-precision UPOLS / UPOLA convolver ----------------------------------
 * C instances of upols_convolver<complex<double>> (method 0) or upola_convolver<complex<double>>
 * (method 1): the float handles' semantics per block and bin with Float = double
 * (uniform_partitioned_convolver.hpp:13-65, overlap_save.hpp:84-112, overlap_add.hpp:76-106), a
 * handle type of its own. `block` = B a power of two in [16, 4096]. A block is two launches (MAC
 * over C x splits workgroups, then one workgroup per channel sums the splits' slabs in order and
 * runs the c2r); equal calls give equal bits. split_workgroups: the workgroups the MAC aims for
 * (0: automatic, the float plain step's rule). Whole blocks only; no streaming levels, fades,
 * latency mode or groups. Bad arguments return NEO_HIP_EINVAL before any device call.
 * Batched passes (neo_hip_upols64_set_batch, off by default) are for calls of many blocks, as in
 * offline work: T consecutive blocks of every channel share one read of the filter and the delay
 * line. A pass is three launches, four for overlap-add: the T window transforms into scratch rows;
 * the MAC with T accumulators and a sliding window of T delay-line rows per bin; the slab sums and
 * c2r of the T blocks, where the last min(T, P) spectra also enter the ring. A call of q T + r
 * blocks runs q passes, then r plain steps. Passes and steps share the ring and the previous block /
 * tail, so calls with and without batching interleave freely. Fixed order, no atomics. */
typedef struct neo_hip_upols64 neo_hip_upols64;
NEO_HIP_API int neo_hip_upols64_create(int channels, int block, int partitions, int device, int method /* 0 upols, 1 upola */,
                                       int split_workgroups /* 0 auto */, neo_hip_upols64** h);
NEO_HIP_API int neo_hip_upols64_destroy(neo_hip_upols64* h);
/* filter [C][P][B+1] complex double (uniform_partition layout), host or device. Resets all state,
 * as filter() does in the reference. Synchronous. */
NEO_HIP_API int neo_hip_upols64_set_filter(neo_hip_upols64* h, const void* filter, int is_device);
/* ir [C][length] double -> (normalize_impulse) -> uniform_partition -> filter, all on the device;
 * equal bit for bit to the three calls in turn. length must give the handle's partitions. */
NEO_HIP_API int neo_hip_upols64_set_impulse(neo_hip_upols64* h, const double* ir, int64_t length, int normalize,
                                            int is_device);
NEO_HIP_API int neo_hip_upols64_reset(neo_hip_upols64* h);
/* n = k B samples per channel, channel c at in + c*ld_in / out + c*ld_out (in == out allowed):
 * k step pairs (with offline windows on: whole windows of 128 blocks first; with batching on: whole
 * passes next; then step pairs). Strides in doubles, >= n and even
 * (16-byte rows); device bases 16-byte aligned;
 * anything else is refused without advancing state. Device memory: asynchronous on `stream`, no
 * host wait between blocks. Host memory: through pinned staging, synchronous. */
NEO_HIP_API int neo_hip_upols64_process_samples(neo_hip_upols64* h, const double* in, int64_t ld_in, double* out,
                                                int64_t ld_out, int64_t num_samples, int is_device, void* stream);
/* splits per channel, partitions per split (the last split may be shorter), device bytes held */
NEO_HIP_API int neo_hip_upols64_info(neo_hip_upols64* h, int* splits, int* rows, int64_t* state_bytes);
/* the same for a shape, host only (no device call) */
NEO_HIP_API int neo_hip_upols64_plan(int channels, int block, int partitions, int split_workgroups, int* splits,
                                     int* rows, int64_t* state_bytes);
/* Batched passes on or off. blocks: 0 off, 1 on with the plan's blocks per pass, 8 or 16 on with that
 * many. A setup call: it waits for the handle's queued work; turning on takes the scratch, the
 * pass's slabs and (overlap-add) the tails from the device pool, turning off or destroy gives them
 * back. Filter, ring and previous block / tail are untouched: it may come between any two process
 * calls. Off by default; a handle that never calls it behaves and reports as before. */
NEO_HIP_API int neo_hip_upols64_set_batch(neo_hip_upols64* h, int blocks);
/* blocks per pass (1 while batching is off), splits per channel of the pass's MAC, device bytes that
 * batching holds on top of state_bytes */
NEO_HIP_API int neo_hip_upols64_batch_info(neo_hip_upols64* h, int* blocks_per_pass, int* splits, int64_t* extra_bytes);
/* the same for a shape, host only, `blocks` as in set_batch (0 counts as 1): also the partitions per
 * split (the last split may be shorter) and the algorithmic bytes of one pass */
NEO_HIP_API int neo_hip_upols64_batch_plan(int channels, int block, int partitions, int method, int split_workgroups,
                                           int blocks, int* blocks_per_pass, int* splits, int* rows, int64_t* extra_bytes,
                                           int64_t* pass_bytes);
/* Offline windows, the third gear, for calls of 128 blocks and more (a whole file to render): off
 * by default, enable 0 or 1 (anything else: NEO_HIP_EINVAL), any P >= 1. While on, process_samples
 * runs a window pass for every 128 blocks left, then batched passes if batching is on, then plain
 * steps; all three share the ring and the previous block / tail, so they mix freely at block
 * boundaries, across calls and across toggling.
 * The rule, per channel and bin (packed rows of B complex doubles, bin 0 = {DC, Nyquist}): a window
 * is 128 consecutive blocks at write position w; block j's spectrum is the fresh scratch row N[j].
 * Window row e, the spectrum of the block e blocks after the window's first, is N[e] for e >= 0, the
 * ring row (w + e) mod P as it stood before the pass for -P < e < 0, and zero for e <= -P (such rows
 * meet only the zero padding of the last filter segment; the ring stays at exactly P rows). With
 * nseg = ceil(P / 128),
 *   Y[j], j = 0..127 = samples 128 + j of IDFT256( sum over q < nseg of
 *                      DFT256(rows -128 (q + 1) .. -128 q + 127) . HF[q] ),
 * HF[q] = DFT256 along the partition axis of filter rows 128 q .. 128 q + 127 (zero past P, zero
 * padded to 256), accumulated in the fixed order q = 0, 1, ..; no atomics, equal calls give equal
 * bits. A pass is three launches, four for overlap-add: the 128 window transforms; per 8 bins of a
 * channel the pairs from the newest back (every ring row read once), the products and one inverse
 * transform; per block the c2r, the output and, for the last min(128, P) blocks, the ring commit;
 * the overlap chain. The segment spectra are rebuilt on the stream of the first window pass after
 * set_filter / set_impulse / set_offline(1). in == out holds as for the other gears.
 * Memory, from the device pool, given back by set_offline(0) and destroy: the spectra
 * [C][nseg][256][B] (16 C nseg 256 B bytes, about twice the filter), and extra_bytes: the scratch
 * and Y [C][128][B] complex double each and (overlap-add) the tails [C][128][B] double. If the pool
 * cannot give them: NEO_HIP_ENOMEM, the handle as it was. A setup call: it waits for the handle's
 * queued work.
 * Inf / NaN: a non-finite input block makes every output block of every window whose pairs hold it
 * non-finite, on that channel: the window that contains it and the windows after it up to the last
 * one that starts at a block t_W with t_W - 128 nseg <= that block; overlap-add adds the block after
 * those. Other channels, and earlier windows of that channel, are untouched bit for bit. */
NEO_HIP_API int neo_hip_upols64_set_offline(neo_hip_upols64* h, int enable);
/* blocks per window pass (128; 0 while off), segments nseg, bytes of the segment spectra, bytes of
 * scratch + Y + tails (all 0 while off) */
NEO_HIP_API int neo_hip_upols64_offline_info(neo_hip_upols64* h, int* blocks_per_pass, int* segments,
                                             int64_t* spectra_bytes, int64_t* extra_bytes);
/* the same for a shape, host only (bad shapes refused before any device call): also the algorithmic
 * bytes of one window pass */
NEO_HIP_API int neo_hip_upols64_offline_plan(int channels, int block, int partitions, int method, int* blocks_per_pass,
                                             int* segments, int64_t* spectra_bytes, int64_t* extra_bytes,
                                             int64_t* pass_bytes);

/* -- one-shot full convolution (extra/python/src/neo/__init__.py:43-48) ----
 * out has n + m - 1 samples; n == 0 or m == 0 is a no-op (empty result).
 * fft_convolve: fft_convolver.hpp:19-93 (one r2c/c2r pair of size
 * 2^next_order(n+m-1) <= 2^27). direct_convolve: direct_convolve.hpp:14-56,
 * bit-identical to the reference's float loop. Host or device pointers. */
NEO_HIP_API int neo_hip_fft_convolve(const float* signal, int64_t n, const float* patch, int64_t m, float* out,
                                     int is_device, int device);
NEO_HIP_API int neo_hip_direct_convolve(const float* signal, int64_t n, const float* patch, int64_t m, float* out,
                                        int is_device, int device);
/* double overloads (main.cpp:257-258 bind both float and double) */
NEO_HIP_API int neo_hip_fft_convolve_f64(const double* signal, int64_t n, const double* patch, int64_t m, double* out,
                                         int is_device, int device);
NEO_HIP_API int neo_hip_direct_convolve_f64(const double* signal, int64_t n, const double* patch, int64_t m,
                                            double* out, int is_device, int device);

/* -- STFT (stft_plan, src/neo/fft/stft.hpp:40-109) ------------------------------
 * x [C][L] -> out [C][F][N/2+1] complex (float or double), N = 2^next_order(transform_size),
 * hop = frame_size - overlap, F = neo_hip_stft_num_frames(L, frame_size, overlap)
 * (detail::num_sftf_frames, :21-25). Frame f = x[f*hop, +min(L - f*hop, frame_size))
 * zero-padded to N, times window[0, N) (NULL = hann_window over N, windowing.hpp:29-41),
 * then rfft. Host or device pointers (window in the same memory as x). */
NEO_HIP_API int neo_hip_stft_num_frames(int64_t length, int frame_size, int overlap, int64_t* frames);
NEO_HIP_API int neo_hip_stft(const float* x, int channels, int64_t length, int frame_size, int transform_size,
                             int overlap, const float* window, void* out, int is_device, int device);
NEO_HIP_API int neo_hip_stft_f64(const double* x, int channels, int64_t length, int frame_size, int transform_size,
                                 int overlap, const double* window, void* out, int is_device, int device);

#ifdef __cplusplus
}
#endif

#endif /* NEO_HIP_H */
