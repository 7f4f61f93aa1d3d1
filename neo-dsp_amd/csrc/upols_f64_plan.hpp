// upols_f64_plan.hpp — the shape plan of a double-precision UPOLS / UPOLA convolver handle
// (neo_hip_upols64, upols_f64.hip): the create call's argument checks, the split of the partitions
// over workgroups and the byte counts, once. Host only, no HIP header, so it compiles into the plan
// test (tests/cpp/upols_f64_plan_main.cpp) without a GPU.
//   upols64_shape        the plan
//   make_upols64_shape   checks + rules; the refusal text or nullptr
//   upols64_io_refusal   the I/O contract of process_samples; the refusal text or nullptr
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
