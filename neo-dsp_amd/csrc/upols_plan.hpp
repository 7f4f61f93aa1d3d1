// upols_plan.hpp — the shape plan of a UPOLS convolver handle (neo_hip_upols; dense, v2 and sparse
// kinds): every argument and option check of the create calls and every rule that turns (channels,
// block, partitions, options) into launch shapes, once. Host only, no HIP header, so it compiles
// into the plan test (tests/cpp/upols_plan_main.cpp) without a GPU.
//   constants                         what the rules read, with their measurements
//   upols_shape                       the plan; its level schedule is a level_sched (levels_plan.hpp)
//   make_upols_shape                  checks + rules; the refusal text or nullptr
//   sparse_cache_rows                 a sparse handle's cacheable rows, from the kept bytes of a filter
#pragma once

#include "levels_plan.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>

namespace neo_hip {

constexpr int kMaxBatch = 32;                          // most blocks one batched MAC pass consumes
constexpr double kFusedMaxBytes = 64.0 * 1024 * 1024;  // filter + FDL bytes below which a step is one launch
constexpr double kCacheBudgetBytes = 216.0 * 1024 * 1024;  // filter bytes read cacheable (256 MiB Infinity Cache)
// the batched passes leave more of the Infinity Cache to the slabs (same-box A/B at C5, 4 runs
// each: 168 MiB 17.8 us/step, 216 MiB 18.3, 126 MiB 18.1)
constexpr double kBatchCacheBudgetBytes = 168.0 * 1024 * 1024;
// offline windows (k_off_mac): batched calls of >= 128 blocks take windows of kFarT blocks through
// partition-axis transforms of every 128-partition segment, from this many partitions
#ifndef NEO_OFF_MIN_P
#define NEO_OFF_MIN_P 128  // diagnostic builds (A/B)
#endif
constexpr int kOffMinP = NEO_OFF_MIN_P;
constexpr int kOffMaxWP = 2;  // windows per pass
// The offline windows' ring, 128 (nseg + 2) rows, is a multiple of 256 rows: a channel stride of
// 5 x 2^20 bytes at B = 512 made the streaming step 4 % slower at c5full (same-box A/B: 9.29-9.49
// vs 9.68-9.74 Gsamples/s at 20 steps, as with the ring of P + 31 rows); one more row keeps it odd
// and restores it (9.58-9.83). profiles/r6_ab_ring.json
#ifndef NEO_OFF_RING_PAD
#define NEO_OFF_RING_PAD 1  // diagnostic builds (A/B): 0 = the even ring
#endif

inline bool valid_block(int b) { return b >= 16 && b <= 4096 && (b & (b - 1)) == 0; }

// blocks per batched pass for block B and NB bins per lane-vector: the requested T,
// capped so one lane's accumulators (T * NB * VPT * 4 floats) stay <= 128 registers
constexpr int batch_t(int B, int NB, int want)
{
    (void)B;
    const int VPT = 1;
    int t = want;
    while (t > 2 && t * NB * VPT > 32) t /= 2;
    return t;
}

enum class upols_kind { dense, v2, sparse };

// The plan of one handle. Everything but batch, off, ahead (the set calls switch them) and, on a
// sparse handle, pc and pcb (sparse_cache_rows, with every filter) is fixed at create.
struct upols_shape {
    // the shape (C, B, P), the FDL ring's rows and the streaming levels' schedule; a sparse handle
    // has no levels: the shape and the ring only
    level_sched sched;
    // one launch per block (last-arriver tail) instead of MAC + finish: on for small filter
    // + FDL working sets, where the step is launch-bound (C3: 10.6 vs 12.4 us per block),
    // off for HBM-bound ones (C5: 0.342 vs 0.303 ms); neo_hip_upols_opts.fused overrides
    bool fused = false;
    int S = 1, rows = 1;     // plain step: splits per channel, partitions per split
    bool batch = true;       // process_blocks runs T blocks per MAC pass (neo_hip_upols_set_batch)
    int Sb = 1, rows_b = 1;  // batched pass: splits per channel, partitions per split (whole chunks of kMaxBatch)
    int bT = 32, bNB = 1;    // batched pass: blocks per pass (capped by batch_t), bins per lane-vector
    int pc = 0;              // filter rows per channel the step reads cacheable (kCacheBudgetBytes)
    int pcb = 0;             // the same for the batched MAC (kBatchCacheBudgetBytes)
    bool bufload = true;     // batched MAC with buffer loads (one channel's rows span < 2 GiB)
    // offline windows (k_off_mac, launch_offline): batched calls take 128 or 256 blocks per pass
    bool off = false;        // eligible (P >= kOffMinP, whole-block dense handles) and on (neo_hip_upols_set_offline)
    int off_nseg = 0;        // 128-partition segments from p = 0
    bool ahead = false;      // streaming levels (upols_levels.hip) on (neo_hip_upols_set_ahead)
    // H / FDL layout: row p of channel c at c * cstride + p * pstride (complex units), [C][ring][B]
    int64_t cstride = 0, pstride = 0;
};

inline int batch_blocks(const upols_shape& sh) { return batch_t(sh.sched.B, sh.bNB, sh.bT); }

// The plan of a convolver of `channels` channels, blocks of `block`, `partitions` partitions with
// the options opts (null: every choice automatic). A sparse handle reads fused and
// split_workgroups only. borrowed: a convolver group's member (its group's stream). Returns
// nullptr, or why the handle cannot be had (a text that lives until the thread's next call).
inline const char* make_upols_shape(int channels, int block, int partitions, const neo_hip_upols_opts* opts,
                                    upols_kind kind, bool borrowed, upols_shape& out)
{
    thread_local char why[160];
    const bool sparse = kind == upols_kind::sparse, v2 = kind == upols_kind::v2;
    neo_hip_upols_opts o{-1, 0, 0, 0, -1, -1, 0, 0, 0, 0, 0};
    if (opts && sparse) {
        o.fused = opts->fused;
        o.split_workgroups = opts->split_workgroups;
    } else if (opts) {
        o = *opts;
    }
    if (o.fused < -1 || o.fused > 1 || o.levels < -1 || o.levels > 1 || o.far_level < -1 || o.far_level > 2 ||
        o.split_workgroups < 0 ||
        (o.batch_blocks && (o.batch_blocks < 2 || o.batch_blocks > kMaxBatch || (o.batch_blocks & (o.batch_blocks - 1)))) ||
        o.batch_bins < 0 || o.batch_bins > 2 || o.far_group < 0 || o.far_group > 4 || o.toep_split < 0 || o.toep_split > 2 ||
        (o.step_group != 0 && o.step_group != 1 && o.step_group != 2 && o.step_group != 4 && o.step_group != 8) ||
        o.far_phase2 < 0 || o.far_phase2 > 2 || o.windows < 0 || o.windows > 2)
        return "invalid convolver options";
    if (channels < 1) return "channels must be >= 1";
    if (!valid_block(block)) {
        std::snprintf(why, sizeof why, "block must be a power of two in [16, 4096], got %d", block);
        return why;
    }
    if (partitions < 1) return "partitions must be >= 1";
    out = upols_shape{};
    level_sched& sc = out.sched;
    if (sparse) {
        // the step reads a channel's FDL ring (and its tiles, never more bytes than P rows) through one
        // buffer descriptor each
        if ((int64_t(partitions) + kMaxBatch - 1) * block * int64_t(sizeof(cf)) >= (int64_t(1) << 31)) {
            std::snprintf(why, sizeof why, "sparse convolvers take channels whose FDL ring spans < 2 GiB (%d partitions of %d)",
                          partitions, block);
            return why;
        }
        sc.C = channels;
        sc.B = block;
        sc.P = partitions;
        sc.ring = partitions + kMaxBatch - 1;
        // process_blocks: one block per pass through the sparse step unless neo_hip_upols_set_batch
        // turns the batched passes on (upols_sparse_batch.hip)
        out.batch = false;
    } else {
        // the level plan and schedule options; the ring grows to what the far level reads back
        if (const char* w = make_level_sched(channels, block, partitions, partitions + kMaxBatch - 1, o, borrowed, v2, sc))
            return w;
        // offline windows (k_off_mac): a pass of 128 wp blocks reads rows back to t_W - 128 nseg while
        // writing rows t_W .. t_W + 128 wp - 1
        out.off = !v2 && partitions >= kOffMinP;
        out.off_nseg = (partitions + kFarT - 1) / kFarT;
        if (out.off) sc.ring = std::max(sc.ring, kFarT * (out.off_nseg + kOffMaxWP) + NEO_OFF_RING_PAD);
        if (o.batch_blocks) out.bT = o.batch_blocks;
        if (o.batch_bins) out.bNB = o.batch_bins;
        // filter rows kept resident in the Infinity Cache across steps: the first pc rows of
        // every channel are read with the default policy, ~216 MiB in all (A/B on MI355X: C5
        // 0.302 -> 0.286 ms per MAC at 220 rows, C4 0.295 -> 0.282 at 400; past ~250 MiB
        // the cached rows start evicting each other)
        out.pc = int(std::min<double>(partitions, kCacheBudgetBytes / (double(channels) * block * sizeof(cf))));
        out.pcb = int(std::min<double>(partitions, kBatchCacheBudgetBytes / (double(channels) * block * sizeof(cf))));
        // streaming levels (upols_levels.hip) instead of one pass over filter + FDL per block,
        // from 64 partitions, blocks up to 1024; short filters keep the plain step, whose one pass
        // is already small (its working set sits in the Infinity Cache)
        out.ahead = !v2 && block <= 1024 && (o.levels >= 0 ? o.levels != 0 : partitions >= 64);
    }
    // the dense shape decides the rest for every kind, so a sparse handle and a dense one of the
    // same shape and options cut the partitions alike (equal row counts; the order per bin is the
    // dense order)
    out.fused = 2.0 * 8.0 * double(channels) * double(partitions) * double(block) < double(kFusedMaxBytes);
    if (o.fused >= 0) out.fused = o.fused != 0;
    out.cstride = int64_t(sc.ring) * block;
    out.pstride = block;
    out.bufload = (int64_t(sc.ring - 1) * out.pstride + block) * int64_t(sizeof(cf)) < (int64_t(1) << 31);
    // splits per channel: aim for ~1024 workgroups (4 per CU, all resident at 8 waves/SIMD;
    // A/B on MI355X: 1024 beat 512/768/2048/4096 at C4 and C5), <= 64 partial slabs
    const int target = o.split_workgroups ? o.split_workgroups : 1024;
    // >= 8 rows per split keeps the slab sum short at small C; the one-launch (latency) form
    // takes >= 16 (C3: 12 splits, 9.6 vs 10.6 us per block with 24)
    // (an explicit workgroup target is taken as given); above B = 512 the one-launch form takes
    // >= 8 rows: a split's rows stream through one CU (~130 GB/s), the tail sums the slabs alone.
    // One channel, P = 32, us per step with 2 / 4 / 8 splits (normal; latency mode): B = 4096
    // 25.1 / 22.6 / 22.3 (22.5 / 21.2 / 23.4), B = 2048 16.3 / 15.2 / 15.2 (12.8 / 11.9 / 12.4),
    // B = 1024 12.5 / 12.2 / 12.7 (10.0 / 9.3 / 9.6) (tools/plain_split_sweep.py)
    const int min_rows = o.split_workgroups ? 1 : out.fused ? (block > 512 ? 8 : 16) : 8;
    const int S = std::max(1, std::min({(target + channels - 1) / channels, (partitions + min_rows - 1) / min_rows, 64}));
    out.rows = (partitions + S - 1) / S;
    out.S = (partitions + out.rows - 1) / out.rows;
    // batched passes: >= 2T partitions per split so the sliding FDL window's warm-up (T - 1 extra
    // rows per split) stays under half the split's rows. 256-lane workgroups at 2 waves/SIMD -> 2
    // resident per CU, so 512 fill the chip once with no second round (A/B, bmac_var 3: C5 0.409 ->
    // 0.367 ms per pass, C4 0.369 -> 0.379 ms, within run-to-run spread)
    const int btarget = 512;
    // workgroups per (channel, split): the batched MAC has one lane per bin, <= 256 lanes
    const int bgroups = std::max(1, block / out.bNB / 256);
    const int Sb = std::max(1, std::min({(btarget + channels * bgroups - 1) / (channels * bgroups),
                                         partitions / (2 * batch_blocks(out)), 64}));
    out.rows_b = ((partitions + Sb - 1) / Sb + kMaxBatch - 1) / kMaxBatch * kMaxBatch;  // whole chunks of any T
    out.Sb = (partitions + out.rows_b - 1) / out.rows_b;
    return nullptr;
}

// The fade step of a live filter update (upols_fade.hip: both banks against the same FDL rows, always
// MAC + finish, never the last-arriver form): it cuts the partitions where the plain step does, S
// splits of `rows` partitions (the last one shorter), so a fade block runs the plain step's grid
// C x S (~1024 workgroups of 4 waves, 4 per CU) over 24 bytes per bin and partition instead of 16.
// slab_bytes: its slabs [C][S][2][B]; bank_bytes: the second filter bank, the handle's own layout
// [C][ring][B] (cstride, pstride), so every kernel takes it by pointer.
struct upols_fade_plan {
    int S = 1, rows = 1;
    int64_t slab_bytes = 0, bank_bytes = 0;
};
inline upols_fade_plan upols_fade_split(const upols_shape& sh)
{
    upols_fade_plan f;
    f.S = sh.S;
    f.rows = sh.rows;
    f.slab_bytes = int64_t(sh.sched.C) * f.S * 2 * sh.sched.B * int64_t(sizeof(cf));
    f.bank_bytes = int64_t(sh.sched.C) * sh.cstride * int64_t(sizeof(cf));
    return f;
}

// A sparse handle's cacheable rows: all P while the kept bytes of its filter fit the budget (the
// Infinity Cache budget of the dense step, in kept bytes), else the budget's share of them
inline int sparse_cache_rows(int P, double kept_bytes, double budget)
{
    return kept_bytes <= budget ? P : int(double(P) * budget / kept_bytes);
}

}  // namespace neo_hip
