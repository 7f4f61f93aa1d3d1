// upols_f64_plan.hpp — the shape plan of a double-precision UPOLS / UPOLA convolver handle
// (neo_hip_upols64, upols_f64.hip): the create call's argument checks, the split of the partitions
// over workgroups and the byte counts, once. Host only, no HIP header, so it compiles into the plan
// test (tests/cpp/upols_f64_plan_main.cpp) without a GPU.
//   upols64_shape        the plan
//   make_upols64_shape   checks + rules; the refusal text or nullptr
//   upols64_io_refusal   the I/O contract of process_samples; the refusal text or nullptr
// and of its batched passes (upols_f64_batch.hip; tests/cpp/upols_f64_batch_plan_main.cpp):
//   upols64_window_src, upols64_commit_row   the two index rules of a pass, host and device
//   upols64_batch_shape, make_upols64_batch_shape   blocks per pass, splits, byte counts
// and of its offline windows (upols_f64_offline.hip; tests/cpp/upols_f64_offline_plan_main.cpp):
//   upols64_offline_src                                  where a window row comes from: scratch, ring or zero
//   upols64_offline_shape, make_upols64_offline_shape    segments and byte counts
#pragma once

#include "upols_plan.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>

namespace neo_hip {

// The plan of one handle, fixed at create. Layout (complex double units): filter H [C][P][B] and the
// FDL [C][P][B], a ring of exactly P rows, packed rows with bin 0 = {DC, Nyquist}; prev [C][B] double
// (overlap-save: the previous block, overlap-add: the overlap tail); slabs [C][S][B].
struct upols64_shape {
    int C = 0, B = 0, P = 0;
    bool ola = false;
    int S = 1, rows = 1;  // splits per channel, partitions per split (the last split may be shorter)
    int64_t filter_bytes = 0, fdl_bytes = 0, prev_bytes = 0, slab_bytes = 0;
    int64_t state_bytes = 0;  // their sum: what a handle holds on the device
    int64_t step_bytes = 0;   // algorithmic bytes of one block step
};

// The plan of a convolver of `channels` channels, blocks of `block`, `partitions` partitions;
// method 0 overlap-save, 1 overlap-add; split_workgroups 0: automatic. Returns nullptr, or why the
// handle cannot be had (a text that lives until the thread's next call). The checks and their
// texts are make_upols_shape's (upols_plan.hpp).
inline const char* make_upols64_shape(int channels, int block, int partitions, int method, int split_workgroups,
                                      upols64_shape& out)
{
    thread_local char why[160];
    if (split_workgroups < 0) return "invalid convolver options";
    if (method < 0 || method > 1) return "method must be 0 (upols) or 1 (upola)";
    if (channels < 1) return "channels must be >= 1";
    if (!valid_block(block)) {
        std::snprintf(why, sizeof why, "block must be a power of two in [16, 4096], got %d", block);
        return why;
    }
    if (partitions < 1) return "partitions must be >= 1";
    out = upols64_shape{};
    out.C = channels;
    out.B = block;
    out.P = partitions;
    out.ola = method == 1;
    // The float plain step's two-launch rule (upols_plan.hpp: ~1024 workgroups, >= 8 rows per split,
    // <= 64 slabs; an explicit workgroup target is taken as given). Its constants were measured for
    // 16 bytes per bin and partition, not 32: inherited here, see DESIGN.md 5.10.
    const int target = split_workgroups ? split_workgroups : 1024;
    const int min_rows = split_workgroups ? 1 : 8;
    const int S = std::max(1, std::min({(target + channels - 1) / channels, (partitions + min_rows - 1) / min_rows, 64}));
    out.rows = (partitions + S - 1) / S;
    out.S = (partitions + out.rows - 1) / out.rows;
    const int64_t row = int64_t(block) * 16;  // one packed row of complex doubles
    out.filter_bytes = int64_t(channels) * partitions * row;
    out.fdl_bytes = out.filter_bytes;
    out.prev_bytes = int64_t(channels) * block * 8;
    out.slab_bytes = int64_t(channels) * out.S * row;
    out.state_bytes = out.filter_bytes + out.fdl_bytes + out.prev_bytes + out.slab_bytes;
    // a step reads the filter and every FDL row but the fresh one, writes that one, reads the block
    // and (overlap-save) the previous one, writes the next prev / tail, writes and reads the slabs
    // and writes the output block
    out.step_bytes = 2 * out.filter_bytes + 2 * out.slab_bytes + int64_t(channels) * block * 8 * 4;
    return nullptr;
}

#if defined(__HIPCC__)
#define NEO_F64_HD __host__ __device__
#else
#define NEO_F64_HD
#endif

// ---- batched passes (upols_f64_batch.hip) ----
// A pass is T consecutive blocks of every channel at write position w. Block j's spectrum is the
// fresh row N[j] of a scratch [C][T][B]; block j at partition p takes window row e = j - p: the
// fresh row N[e] when e >= 0, else the ring row (w + e) mod P as it stood before the pass (one wrap:
// e > -P). The ring takes the fresh rows after the MAC, in the finish launch.

// where window row e comes from: the scratch row `row`, or the ring row `row`
struct upols64_row_src {
    bool scratch;
    int row;
};
NEO_F64_HD inline upols64_row_src upols64_window_src(int e, int w, int P)
{
    if (e >= 0) return {true, e};
    const int r = w + e;
    return {false, r < 0 ? r + P : r};
}

// the ring row that block j of a pass of T commits its fresh row to, or -1: only the last
// min(T, P) blocks commit, so a ring row is written at most once per pass
NEO_F64_HD inline int upols64_commit_row(int j, int T, int P, int w) { return j < T - P ? -1 : (w + j) % P; }

struct upols64_batch_shape {
    int T = 1;            // blocks per pass; 1: batching off
    int S = 1, rows = 1;  // splits per channel of the pass's MAC, partitions per split (the last may be shorter)
    int64_t scratch_bytes = 0, slab_bytes = 0, tail_bytes = 0;
    int64_t extra_bytes = 0;  // their sum: what batching adds to the handle on the device
    int64_t pass_bytes = 0;   // algorithmic bytes of one pass
};

// Blocks per pass: 16 for every B, by measurement. The MAC lane holds T accumulators and T window
// rows of 4 VGPRs each and 4 rows of prefetch: T = 16 compiles to 236 VGPRs without spills (2 waves
// per SIMD), T = 8 to 140 (3 waves), T = 32 cannot fit. The pass is HBM-bound and 16 halves the filter
// and ring traffic per block against 8: measured per block (profiles/upols_f64_batch_sweep.json,
// DESIGN.md 6) 45.7 us against 94.7 at 256 x 512 x 938, 82.6 against 176.1 at 256 x 256 x 3750 and
// 1.4 against 2.2 at 1 x 512 x 188. T = 8 was faster nowhere.
inline int upols64_default_blocks_per_pass(int /*block*/) { return 16; }

// The plan of the passes of a handle of shape sh. blocks: 0 or 1 the rule above, 8 or 16 that many.
// split_workgroups as at create: 0 automatic, else the plain step's splits are taken as they are.
// Returns nullptr or the refusal text.
inline const char* make_upols64_batch_shape(const upols64_shape& sh, int blocks, int split_workgroups, upols64_batch_shape& out)
{
    if (blocks != 0 && blocks != 1 && blocks != 8 && blocks != 16) return "blocks per pass must be 0 (automatic), 8 or 16";
    out = upols64_batch_shape{};
    out.T = blocks > 1 ? blocks : upols64_default_blocks_per_pass(sh.B);
    if (split_workgroups) {
        out.S = sh.S;
        out.rows = sh.rows;
    } else {
        // The plain step's rule over the pass's grid, C x S x ceil(B / 256) workgroups: ~1024 of them,
        // at least T rows per split (the sliding window fills once per split), <= 64 slabs. The
        // constants are the float step's, inherited: the sweep only shows that asking for two and
        // four times the workgroups is slower at all three shapes (more window rows and slabs).
        const int chunks = (sh.B + 255) / 256;
        const int64_t per_split = int64_t(sh.C) * chunks;
        const int want = int(std::min<int64_t>((1024 + per_split - 1) / per_split, 64));
        const int S = std::max(1, std::min(want, sh.P / out.T));
        out.rows = (sh.P + S - 1) / S;
        out.S = (sh.P + out.rows - 1) / out.rows;
    }
    const int64_t row = int64_t(sh.B) * 16;
    out.scratch_bytes = int64_t(sh.C) * out.T * row;
    out.slab_bytes = int64_t(sh.C) * out.S * out.T * row;
    out.tail_bytes = sh.ola ? int64_t(sh.C) * out.T * sh.B * 8 : 0;
    out.extra_bytes = out.scratch_bytes + out.slab_bytes + out.tail_bytes;
    // a pass reads the filter and the ring once, writes the scratch, reads T window rows per split,
    // writes and reads the slabs, copies min(T, P) rows into the ring, and moves per block 3 rows of
    // samples (overlap-save: block, previous block, output) or 6 (overlap-add: block; output and
    // tail written; output and the tail before it read, output written again); the next prev /
    // overlap adds one row per channel
    out.pass_bytes = sh.filter_bytes + sh.fdl_bytes + out.scratch_bytes + int64_t(sh.C) * out.S * out.T * row +
                     2 * out.slab_bytes + 2 * int64_t(sh.C) * std::min(out.T, sh.P) * row +
                     int64_t(sh.C) * sh.B * 8 * (int64_t(out.T) * (sh.ola ? 6 : 3) + 1);
    return nullptr;
}

// ---- offline windows (upols_f64_offline.hip) ----
// A window is kOff64W = 128 consecutive blocks of every channel at write position w, computed per
// bin with 256-point transforms along the block axis. Window row e is the spectrum of the block e
// blocks after the window's first: the fresh scratch row N[e] for e >= 0, the ring row (w + e) mod P
// as it stood before the pass for -P < e < 0, and ZERO for e <= -P: such rows meet only the zero
// padding of the last filter segment and the ring, exactly P rows, never held them. With
// nseg = ceil(P / 128), per channel and bin
//   Y[j], j = 0..127 = samples 128 + j of IDFT256( sum over q < nseg, ascending, of
//                      DFT256(rows -128 (q + 1) .. -128 q + 127) . HF[q] )
// HF[q] = DFT256 along the partition axis of filter rows 128 q .. 128 q + 127 (zero past P, zero
// padded to 256), [C][nseg][256][B]. The last min(128, P) fresh rows then go to the ring
// (upols64_commit_row(j, 128, P, w)) and w moves on by 128 mod P.
constexpr int kOff64W = 128;  // blocks per window
constexpr int kOff64F = 256;  // transform length along the block axis

// where window row e of a window pass comes from
enum upols64_offline_kind { kOff64Scratch = 0, kOff64Ring = 1, kOff64Zero = 2 };
struct upols64_offline_row {
    int kind;  // upols64_offline_kind
    int row;   // scratch or ring row; 0 for a zero row
};
NEO_F64_HD inline upols64_offline_row upols64_offline_src(int e, int w, int P)
{
    if (e >= 0) return {kOff64Scratch, e};
    if (e <= -P) return {kOff64Zero, 0};
    const int r = w + e;
    return {kOff64Ring, r < 0 ? r + P : r};
}

struct upols64_offline_shape {
    int nseg = 0;               // 128-partition segments, ceil(P / 128)
    int64_t spectra_bytes = 0;  // HF [C][nseg][256][B]
    int64_t scratch_bytes = 0, y_bytes = 0, tail_bytes = 0;  // N [C][128][B], Y [C][128][B], tails [C][128][B] double
    int64_t extra_bytes = 0;    // scratch + Y + tails (the spectra are counted apart)
    int64_t pass_bytes = 0;     // algorithmic bytes of one window pass
};

// The plan of the window passes of a handle of shape sh: any P >= 1.
inline upols64_offline_shape make_upols64_offline_shape(const upols64_shape& sh)
{
    upols64_offline_shape o;
    o.nseg = (sh.P + kOff64W - 1) / kOff64W;
    const int64_t crow = int64_t(sh.C) * sh.B * 16;  // one packed row of every channel
    o.spectra_bytes = crow * o.nseg * kOff64F;
    o.scratch_bytes = crow * kOff64W;
    o.y_bytes = crow * kOff64W;
    o.tail_bytes = sh.ola ? int64_t(sh.C) * kOff64W * sh.B * 8 : 0;
    o.extra_bytes = o.scratch_bytes + o.y_bytes + o.tail_bytes;
    // a pass writes the scratch; loads the pair rows that are not zero (the 128 fresh rows and the
    // ring rows -min(128 nseg, P - 1) .. -1, each once); reads 256 nseg spectrum rows; writes and
    // reads Y; copies min(128, P) rows into the ring; and moves the samples as a batched pass does
    // (3 rows per block overlap-save, 6 overlap-add, one more per channel for the next prev / overlap)
    const int64_t ring_rows = std::min(kOff64W * o.nseg, sh.P - 1);
    o.pass_bytes = crow * (kOff64W + (kOff64W + ring_rows) + int64_t(kOff64F) * o.nseg + 2 * kOff64W +
                           2 * std::min(kOff64W, sh.P)) +
                   int64_t(sh.C) * sh.B * 8 * (int64_t(kOff64W) * (sh.ola ? 6 : 3) + 1);
    return o;
}

// The I/O contract of process_samples on a handle of block B: n samples per channel, channel c at
// in + c ld_in / out + c ld_out (strides in doubles). Nothing is advanced when a text comes back.
inline const char* upols64_io_refusal(int B, int64_t n, int64_t ld_in, int64_t ld_out)
{
    thread_local char why[160];
    if (n < 0 || ld_in < n || ld_out < n) return "num_samples must be in [0, ld]";
    if (n % B) {
        std::snprintf(why, sizeof why, "upols/upola convolvers take whole blocks (%lld samples, block %d)", (long long)n, B);
        return why;
    }
    if ((ld_in | ld_out) & 1) return "I/O must be 16-byte aligned (ld multiple of 2 doubles)";
    return nullptr;
}

}  // namespace neo_hip
