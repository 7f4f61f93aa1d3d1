// matrix_plan.hpp — the host-side plan of a matrix convolver (upols_matrix.hip): which outputs
// share a workgroup, which FDL rows each of those workgroups walks, and where its splits cut.
// Plain C++, no device: neo_hip_matrix_plan returns it and the handle is built from the same call.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace neo_hip {

// The most workgroups (tiles x splits) for which the MAC launch also runs the tails: each workgroup's
// agent-scope release ahead of the arrival counter costs more than the second launch once there are
// many (tools/matrix_sweep.py at B = 512: ahead at 2 .. 64 workgroups, level at 126 and
// 128, behind from 256 on, up to 2.6 x). The dense step's rule, 64 MiB of filter + FDL, is too wide here.
constexpr int kMatrixFusedMaxWgs = 64;
constexpr int kMatrixMaxSplits = 64;

// the most outputs one workgroup accumulates: OT VPT <= 4 float4 accumulator pairs per lane
constexpr int matrix_max_tile(int B) { return B <= 512 ? 4 : B == 1024 ? 2 : 1; }

// The automatic out_tile is 4 where the sweep has it ahead of 1 by more than the spread of the same
// A/B (tools/matrix_sweep.py, B = 512): tiles whose outputs all take every input of the
// tile's union (dense 8 x 32 and 32 x 32: 8 tiles) with at least 2048 rows in the longest tile,
// -3 .. -10 %; below that many rows a tile of 1 is level or up to 13 % ahead, and so it is for the
// banded matrix (8 of a tile's 11 inputs per output) up to 2816 rows and for 2 x 2 (one tile: too few
// workgroups) at any length. Other block sizes are not measured: 1.
constexpr int kMatrixAutoTileBlock = 512;
constexpr int kMatrixAutoTileRows = 2048;
constexpr int kMatrixAutoTileTiles = 8;

struct matrix_plan {
    int I = 0, O = 0, B = 0, P = 0, nroutes = 0;
    int OT = 1, S = 1, ntiles = 0;
    bool fused = true;
    std::vector<int> rt;          // [O][I]: the route (index into the caller's list) or -1
    std::vector<int> tile_first;  // [ntiles] first output
    std::vector<int> tile_count;  // [ntiles] outputs (<= OT)
    std::vector<int> uni_off;     // [ntiles + 1] into uni
    std::vector<int> uni;         // the tiles' inputs, ascending per tile
    int64_t fdl_loads = 0, filter_loads = 0;  // row loads per step
    int rows(int t) const { return (uni_off[size_t(t) + 1] - uni_off[size_t(t)]) * P; }
    // split s of tile t walks rows [cut(t, s), cut(t, s + 1)) of the tile's list
    int cut(int t, int s) const
    {
        const int n = rows(t), per = (n + S - 1) / S;
        return std::min<int64_t>(n, int64_t(s) * per);
    }
};

// Checks the shape and the route list (why != nullptr: the reason) and fills the plan.
// fused: -1 auto, 0, 1; split_wgs: 0 auto, else the workgroup target; out_tile: 0 auto, 1, 2, 4.
inline const char* make_matrix_plan(int I, int O, int B, int P, const int* route_out, const int* route_in, int nroutes,
                                    int fused, int split_wgs, int out_tile, matrix_plan& pl)
{
    if (I < 1 || O < 1) return "inputs and outputs must be >= 1";
    if (B < 16 || B > 4096 || (B & (B - 1))) return "block must be a power of two in [16, 4096]";
    if (P < 1) return "partitions must be >= 1";
    if (int64_t(P) * B * 8 >= (int64_t(1) << 31)) return "a route's filter must span < 2 GiB";
    if (nroutes < 1) return "nroutes must be >= 1";
    if (!route_out || !route_in) return "null route list";
    if (int64_t(I) * O > (int64_t(1) << 26)) return "inputs x outputs too large";
    if (fused < -1 || fused > 1 || split_wgs < 0 || (out_tile != 0 && out_tile != 1 && out_tile != 2 && out_tile != 4))
        return "invalid options (fused -1 / 0 / 1, split_workgroups >= 0, out_tile 0 / 1 / 2 / 4)";
    pl = matrix_plan{};
    pl.I = I, pl.O = O, pl.B = B, pl.P = P, pl.nroutes = nroutes;
    pl.rt.assign(size_t(I) * size_t(O), -1);
    for (int r = 0; r < nroutes; ++r) {
        const int o = route_out[r], i = route_in[r];
        if (o < 0 || o >= O || i < 0 || i >= I) return "route index out of range";
        if (pl.rt[size_t(o) * I + i] >= 0) return "duplicate route";
        pl.rt[size_t(o) * I + i] = r;
    }
    // consecutive outputs in tiles of ot; returns the (output, union input) pairs of all tiles, which
    // equal the route count iff every output of a tile has a route from every input of its union
    auto tiles = [&](int ot) {
        pl.OT = ot;
        pl.ntiles = (O + ot - 1) / ot;
        pl.tile_first.clear(), pl.tile_count.clear(), pl.uni.clear();
        pl.uni_off.assign(1, 0);
        pl.fdl_loads = 0;
        int64_t pairs = 0;
        for (int t = 0; t < pl.ntiles; ++t) {
            const int first = t * ot, count = std::min(ot, O - first);
            pl.tile_first.push_back(first);
            pl.tile_count.push_back(count);
            for (int i = 0; i < I; ++i) {
                bool any = false;
                for (int o = first; o < first + count; ++o) any = any || pl.rt[size_t(o) * I + i] >= 0;
                if (any) pl.uni.push_back(i);
            }
            pl.uni_off.push_back(int(pl.uni.size()));
            const int nu = pl.uni_off[size_t(t) + 1] - pl.uni_off[size_t(t)];
            pl.fdl_loads += int64_t(nu) * P;
            pairs += int64_t(nu) * count;
        }
        return pairs;
    };
    auto longest = [&] {
        int n = 1;
        for (int t = 0; t < pl.ntiles; ++t) n = std::max(n, pl.rows(t));
        return n;
    };
    if (out_tile) {
        tiles(std::min(out_tile, matrix_max_tile(B)));
    } else if (!(B == kMatrixAutoTileBlock && tiles(4) == nroutes && pl.ntiles >= kMatrixAutoTileTiles &&
                 longest() >= kMatrixAutoTileRows)) {
        tiles(1);
    }
    pl.filter_loads = int64_t(nroutes) * P;
    // splits: the plain step's rule (about 1024 workgroups, >= 8 rows per split, 16 for the one-launch
    // form up to B = 512; an explicit workgroup target is taken as given), on the longest tile
    const int maxrows = longest();
    auto splits = [&](bool fu) {
        const int target = split_wgs ? split_wgs : 1024;
        const int min_rows = split_wgs ? 1 : fu ? (B > 512 ? 8 : 16) : 8;
        const int S = std::max(1, std::min({(target + pl.ntiles - 1) / pl.ntiles, (maxrows + min_rows - 1) / min_rows,
                                            kMatrixMaxSplits}));
        const int per = (maxrows + S - 1) / S;
        return (maxrows + per - 1) / per;  // no empty split in the longest tile
    };
    pl.fused = fused >= 0 ? fused != 0 : int64_t(pl.ntiles) * splits(true) <= kMatrixFusedMaxWgs;
    pl.S = splits(pl.fused);
    return nullptr;
}

// -- the device tables of a checked plan (the handle uploads both with the filter) -----------------
//
// What k_matrix_step reads: tiles [ntiles][4] {first output, outputs, inputs, offset into the
// unions}, the tiles' unions, the route matrix rt [O][I].
inline std::vector<int> matrix_tile_table(const matrix_plan& p)
{
    std::vector<int> tab;
    tab.reserve(size_t(4) * p.ntiles + p.uni.size() + p.rt.size());
    for (int t = 0; t < p.ntiles; ++t) {
        tab.push_back(p.tile_first[size_t(t)]);
        tab.push_back(p.tile_count[size_t(t)]);
        tab.push_back(p.uni_off[size_t(t) + 1] - p.uni_off[size_t(t)]);
        tab.push_back(p.uni_off[size_t(t)]);
    }
    tab.insert(tab.end(), p.uni.begin(), p.uni.end());
    tab.insert(tab.end(), p.rt.begin(), p.rt.end());
    return tab;
}

// What the kernels with one output per workgroup read (k_matrix_off_mac, k_matrix_fade_step): off
// [O + 1], then {input, route} per route, inputs ascending per output.
inline std::vector<int> matrix_route_table(const matrix_plan& p)
{
    std::vector<int> tab(size_t(p.O) + 1, 0);
    for (int o = 0; o < p.O; ++o) {
        for (int i = 0; i < p.I; ++i)
            if (const int r = p.rt[size_t(o) * p.I + i]; r >= 0) tab.insert(tab.end(), {i, r});
        tab[size_t(o) + 1] = int(tab.size() - size_t(p.O) - 1) / 2;
    }
    return tab;
}

// -- live filter updates (upols_matrix_fade.hip): the fade step runs one output per workgroup -------
//
// The splits of the fade step for a checked plan: the plain step's rule for the MAC + finish form
// (about 1024 workgroups, >= 8 rows per split; an explicit workgroup target is taken as given) on the
// output with the most rows, `chunks` workgroups per row (matrix_fade_chunks); no empty split in it.
inline int matrix_fade_splits(const matrix_plan& pl, int split_wgs, int chunks)
{
    int maxrows = 1;
    for (int o = 0; o < pl.O; ++o) {
        int n = 0;
        for (int i = 0; i < pl.I; ++i) n += pl.rt[size_t(o) * pl.I + i] >= 0;
        maxrows = std::max(maxrows, n * pl.P);
    }
    const int64_t per_split = int64_t(pl.O) * chunks;
    const int64_t want = ((split_wgs ? split_wgs : 1024) + per_split - 1) / per_split;
    const int min_rows = split_wgs ? 1 : 8;
    const int S = int(std::max<int64_t>(1, std::min<int64_t>({want, (maxrows + min_rows - 1) / min_rows, kMatrixMaxSplits})));
    const int per = (maxrows + S - 1) / S;
    return (maxrows + per - 1) / per;
}

// -- batched passes (upols_matrix_batch.hip): T blocks share one pass over every route's filter ----
//
// One output per workgroup (the out_tile = 1 row list: the output's inputs ascending x partitions
// 0..P-1). Split s of the Sb splits walks rows [cut(o, s), cut(o, s + 1)) of output o's list, a list
// of RUNS (input, partitions [pa, pb)): at a run's start the kernel reloads its window of T - 1 FDL
// rows, so a run of n rows loads n + T - 1 of them.
constexpr int kMatrixBatch = 32;  // most blocks per pass; a batching handle's ring has P + 31 rows
// the automatic split target, in workgroups (outputs x splits x bin chunks): the pass keeps 2
// workgroups per CU resident (256 VGPRs), 256 CUs
constexpr int kMatrixBatchAutoWgs = 512;

// workgroups per row: rows wider than 256 bins take several
constexpr int matrix_batch_chunks(int B) { return B > 256 ? B / 256 : 1; }

struct matrix_batch_plan {
    int T = 0, Sb = 1, G = 1, O = 0;
    std::vector<int> rows;     // [O] the output's row count
    std::vector<int> run_off;  // [O * Sb + 1] into the runs, split o * Sb + s
    std::vector<int> runs;     // 4 ints per run: input, route, pa, pb
    int64_t filter_rows = 0, fdl_rows = 0, slab_rows = 0, bytes = 0;  // per pass of T blocks
    int nruns() const { return int(runs.size() / 4); }
    // equal row counts (to one row): no split of an output with >= Sb rows is empty
    int cut(int o, int s) const { return int(int64_t(s) * rows[size_t(o)] / Sb); }
};

// The batch plan of a checked plan's route table for passes of T blocks (2 .. 32, a power of two).
// split_wgs: 0 auto (kMatrixBatchAutoWgs workgroups, at least kMatrixBatch rows in every split of the
// longest output, so the rows a run reloads never exceed the rows it walks), else the workgroup
// target, taken as given; at most kMatrixMaxSplits and never an empty split in the longest output.
inline const char* make_matrix_batch_plan(const matrix_plan& pl, int T, int split_wgs, matrix_batch_plan& bp)
{
    if (T < 2 || T > kMatrixBatch || (T & (T - 1))) return "blocks per pass must be 2, 4, 8, 16 or 32";
    if (split_wgs < 0) return "split_workgroups must be >= 0";
    if (int64_t(pl.P + kMatrixBatch - 1) * pl.B * 8 >= (int64_t(1) << 31)) return "an input's ring of P + 31 rows must span < 2 GiB";
    bp = matrix_batch_plan{};
    const int I = pl.I, O = pl.O, P = pl.P;
    bp.T = T, bp.O = O, bp.G = matrix_batch_chunks(pl.B);
    bp.rows.assign(size_t(O), 0);
    int maxrows = 1;
    for (int o = 0; o < O; ++o) {
        int n = 0;
        for (int i = 0; i < I; ++i) n += pl.rt[size_t(o) * I + i] >= 0;
        bp.rows[size_t(o)] = n * P;
        maxrows = std::max(maxrows, n * P);
    }
    const int64_t per_split = int64_t(O) * bp.G;
    const int64_t want = ((split_wgs ? split_wgs : kMatrixBatchAutoWgs) + per_split - 1) / per_split;
    const int most = split_wgs ? maxrows : std::max(1, maxrows / kMatrixBatch);
    bp.Sb = int(std::max<int64_t>(1, std::min<int64_t>({want, most, kMatrixMaxSplits})));
    bp.run_off.assign(1, 0);
    for (int o = 0; o < O; ++o) {
        for (int s = 0; s < bp.Sb; ++s) {
            const int r0 = bp.cut(o, s), r1 = bp.cut(o, s + 1);
            int row = 0;  // where the next of the output's inputs starts in its row list
            for (int i = 0; i < I && row < r1; ++i) {
                const int r = pl.rt[size_t(o) * I + i];
                if (r < 0) continue;
                const int a = std::max(r0, row), b = std::min(r1, row + P);
                if (a < b) {
                    bp.runs.insert(bp.runs.end(), {i, r, a - row, b - row});
                    bp.fdl_rows += b - a + T - 1;
                }
                row += P;
            }
            bp.run_off.push_back(bp.nruns());
        }
    }
    bp.filter_rows = int64_t(pl.nroutes) * P;
    bp.slab_rows = int64_t(O) * bp.Sb * T;
    // filter and FDL row loads, the slabs written and read once, the block I/O
    bp.bytes = 8 * int64_t(pl.B) * (bp.filter_rows + bp.fdl_rows + 2 * bp.slab_rows) + 4 * int64_t(pl.B) * T * (I + O);
    return nullptr;
}

// -- offline windows (upols_matrix_offline.hip): WP windows of 128 blocks per pass -----------------
//
// Per bin the blocks t_W + j (j < 128) of a window are samples 128 + j of the 256-point circular
// convolutions of PAIRS (256 consecutive ring rows: t_W - 128 (q + 1) ... + 255) with the segments
// h_q (partitions 128 q ... + 127, zero past P), summed over q < nseg = ceil(P / 128). A pass at
// write position w writes rows w .. w + 128 WP - 1 and reads back to w - 128 nseg; window 1's pair
// of segment q is window 0's pair of segment q - 1, so a pass has nseg + WP - 1 pairs.
constexpr int kMatrixOffWindow = 128;  // blocks per window (kFarT)
constexpr int kMatrixOffMaxWP = 2;     // windows per pass

constexpr int matrix_offline_segments(int P) { return (P + kMatrixOffWindow - 1) / kMatrixOffWindow; }
// the least ring: a two-window pass's span, and one row more to keep the per-input stride off a
// large power of two ("Ring and channel strides")
constexpr int matrix_offline_ring(int P) { return kMatrixOffWindow * (matrix_offline_segments(P) + kMatrixOffMaxWP) + 1; }
// the first ring row of pair k (k = 0 the newest: the last window's own rows and the 128 before)
constexpr int matrix_offline_pair_row(int w, int wp, int k, int ring)
{
    const int r = (w + kMatrixOffWindow * (wp - 2 - k)) % ring;
    return r < 0 ? r + ring : r;
}
// the pair that segment q of window `window` multiplies
constexpr int matrix_offline_pair_of(int wp, int window, int q) { return q + wp - 1 - window; }

struct matrix_offline_plan {
    int nseg = 0, WP = 0, T = 0, npairs = 0, min_ring = 0, ring = 0;
    std::vector<int> pair_row;  // [npairs]
    int64_t hf_bytes = 0, xf_bytes = 0;  // payloads of the segment and pair spectra
    // rows of B complex per pass: segment spectra read, pair spectra re-read per route (cache), FDL
    // rows read, pair spectra written, output spectra written and read
    int64_t spec_rows = 0, cache_rows = 0, fdl_rows = 0, xf_rows = 0, y_rows = 0;
    int64_t bytes = 0, cache_bytes = 0;  // the model of a pass (cache_bytes is part of bytes)
};

// windows: 0 automatic (2), 1 or 2; write_pos: the ring row of the pass's first block; ring_rows:
// 0 = the least ring
inline const char* make_matrix_offline_plan(int I, int O, int B, int P, int nroutes, int windows, int write_pos,
                                            int ring_rows, matrix_offline_plan& op)
{
    if (I < 1 || O < 1) return "inputs and outputs must be >= 1";
    if (B < 16 || B > 4096 || (B & (B - 1))) return "block must be a power of two in [16, 4096]";
    if (P < 1 || int64_t(P) * B * 8 >= (int64_t(1) << 31)) return "partitions must be >= 1 and a route's filter span < 2 GiB";
    if (nroutes < 1) return "nroutes must be >= 1";
    if (windows < 0 || windows > kMatrixOffMaxWP) return "windows per pass must be 0 (automatic), 1 or 2";
    op = matrix_offline_plan{};
    op.nseg = matrix_offline_segments(P);
    op.WP = windows ? windows : kMatrixOffMaxWP;
    op.T = kMatrixOffWindow * op.WP;
    op.npairs = op.nseg + op.WP - 1;
    op.min_ring = matrix_offline_ring(P);
    op.ring = ring_rows ? ring_rows : op.min_ring;
    if (op.ring < op.min_ring) return "ring_rows below 128 (segments + 2) + 1";
    if (int64_t(op.ring) * B * 8 >= (int64_t(1) << 31)) return "an input's ring must span < 2 GiB";
    if (write_pos < 0 || write_pos >= op.ring) return "write_pos outside the ring";
    for (int k = 0; k < op.npairs; ++k) op.pair_row.push_back(matrix_offline_pair_row(write_pos, op.WP, k, op.ring));
    const int64_t spec = 2 * kMatrixOffWindow;  // rows of a 256-point spectrum
    op.hf_bytes = int64_t(nroutes) * op.nseg * spec * B * 8;
    op.xf_bytes = int64_t(I) * op.npairs * spec * B * 8;
    op.spec_rows = int64_t(nroutes) * op.nseg * spec;
    op.cache_rows = int64_t(nroutes) * op.npairs * spec;
    op.fdl_rows = int64_t(I) * op.npairs * spec;
    op.xf_rows = int64_t(I) * op.npairs * spec;
    op.y_rows = int64_t(O) * op.T * 2;
    op.cache_bytes = 8 * int64_t(B) * op.cache_rows;
    op.bytes = 8 * int64_t(B) * (op.spec_rows + op.cache_rows + op.fdl_rows + op.xf_rows + op.y_rows) +
               4 * int64_t(B) * op.T * (I + O);
    return nullptr;
}

// -- window levels (upols_matrix_levels.hip): long filters block by block ---------------------------
//
// n counts the blocks since the last reset; window W of a level with window length T is the blocks
// [W T, W T + T). The head, the ordinary step on a compact bank, takes partitions [0, 2 T0); level k
// takes the band [2 T_k, 2 T_(k+1)), the last one [2 T_last, P). For a band [a, b) with a >= 2 T
//     slab[j] = sum over routes, p in [a, b) of H_r[p] X_i[W T + j - p],  j < T,
// needs no row newer than block W T + T - 1 - a <= (W - 1) T - 1: every row was written before window
// W - 1 began, so the slab may be computed at any step of window W - 1. Its workgroups (output x split
// x bin chunk, the batched pass's walk over a run table restricted to the band) are cut into T parts
// of equal count, to one; block n launches part n mod T of window n / T + 1.
//
// The ring. A step at block n has written the rows of blocks <= n and a ring of R rows holds blocks
// n - R + 1 .. n. In their turn the parts of window W + 1 run at n <= W T + T - 1 and read back to
// block (W + 1) T - P + 1: R >= P - 1. Priming at n = W T + m computes window W whole, of which the
// rows j >= m are still to be read; row j reads back to block W T + j - P + 1 >= n - P + 1: R >= P
// (the rows j < m may read overwritten ring rows: inside the ring, and nobody reads them). The head
// reads back to n - 2 T0 + 1. So the ring is the plain step's, P rows, and nothing grows; a ring of
// P - 1 rows loses the oldest row of a primed slab.
constexpr int kMatrixMaxLevels = 5;  // 2, 4, 8, 16, 32
// The most splits of a level. A level's partial slabs are 2 O S T rows (double-buffered) and the
// finish reads O S of them per block, so the cap stays the batched pass's: at 32 x 32, B = 512, T = 32
// 64 splits are 512 MiB of slabs and 128 workgroups per part.
constexpr int kMatrixLevelMaxSplits = kMatrixMaxSplits;

struct matrix_level {
    int T = 0, a = 0, b = 0;   // window length, band [a, b)
    int S = 1, nwg = 0;        // splits per output; workgroups of a window: O x S x G
    std::vector<int> run_off;  // [O * S + 1] into the runs, split o * S + s
    std::vector<int> runs;     // 4 ints per run: input, route, pa, pb (a <= pa < pb <= b)
    std::vector<int> part_cut; // [T + 1] part k is the workgroups [part_cut[k], part_cut[k + 1])
    int64_t filter_rows = 0, fdl_rows = 0;  // per window
    int64_t slab_off = 0;      // of this level's slabs [2][O][S][T][B] in the partial buffer, in rows
    int nruns() const { return int(runs.size() / 4); }
};

struct matrix_level_plan {
    int head = 0, G = 1, O = 0, ring = 0;
    matrix_plan hplan;                 // the head: the ordinary step over partitions [0, head), unfused
    std::vector<int> route_out, route_in;  // the route list the head plan was made from
    std::vector<matrix_level> levels;  // T ascending; empty: the handle runs the ordinary step
    int64_t partial_rows = 0, partial_bytes = 0, head_bank_bytes = 0;
    int64_t bytes = 0;                 // the model of one block
};

// windows == nullptr: the default (8, 32), ahead of (4, 8, 16, 32) at every shape of
// tools/matrix_levels_sweep.py (each level is a launch per block). split_wgs: 0 auto (each PART aims at
// kMatrixBatchAutoWgs workgroups, no split of the longest output shorter than T rows), else the
// workgroup target of a part, taken as given; at most kMatrixLevelMaxSplits.
inline const char* make_matrix_level_plan(const matrix_plan& pl, const int* windows, int nwindows, int split_wgs,
                                          matrix_level_plan& lp)
{
    static constexpr int kDefault[] = {8, 32};
    if (!windows) windows = kDefault, nwindows = 2;
    if (nwindows < 1 || nwindows > kMatrixMaxLevels) return "1 to 5 windows";
    for (int k = 0; k < nwindows; ++k) {
        const int T = windows[k];
        if (T < 2 || T > kMatrixBatch || (T & (T - 1))) return "a window must be 2, 4, 8, 16 or 32";
        if (k && T < 2 * windows[k - 1]) return "windows must ascend, each at least twice the one before";
    }
    if (split_wgs < 0) return "split_workgroups must be >= 0";
    lp = matrix_level_plan{};
    const int I = pl.I, O = pl.O, P = pl.P, B = pl.B;
    lp.O = O, lp.G = matrix_batch_chunks(B), lp.ring = P;
    lp.head = std::min(P, 2 * windows[0]);
    lp.route_out.assign(size_t(pl.nroutes), 0), lp.route_in.assign(size_t(pl.nroutes), 0);
    for (int o = 0; o < O; ++o)
        for (int i = 0; i < I; ++i)
            if (const int r = pl.rt[size_t(o) * I + i]; r >= 0) lp.route_out[size_t(r)] = o, lp.route_in[size_t(r)] = i;
    if (const char* why = make_matrix_plan(I, O, B, lp.head, lp.route_out.data(), lp.route_in.data(), pl.nroutes, 0, 0, 0, lp.hplan))
        return why;
    int maxin = 1;  // the inputs of the longest output
    for (int o = 0; o < O; ++o) {
        int n = 0;
        for (int i = 0; i < I; ++i) n += pl.rt[size_t(o) * I + i] >= 0;
        maxin = std::max(maxin, n);
    }
    // head: filter and FDL row loads, the slabs written and read; block I/O
    int64_t bytes = 8 * int64_t(B) * (lp.hplan.filter_loads + lp.hplan.fdl_loads + 2 * int64_t(O) * lp.hplan.S) +
                    4 * int64_t(B) * (I + O);
    for (int k = 0; k < nwindows; ++k) {
        matrix_level lv;
        lv.T = windows[k], lv.a = 2 * lv.T, lv.b = k + 1 < nwindows ? std::min(P, 2 * windows[k + 1]) : P;
        if (lv.a >= lv.b) continue;  // an empty band
        const int len = lv.b - lv.a, maxrows = maxin * len;
        const int64_t per_split = int64_t(O) * lp.G;
        const int64_t want = (int64_t(split_wgs ? split_wgs : kMatrixBatchAutoWgs) * lv.T + per_split - 1) / per_split;
        const int most = split_wgs ? maxrows : std::max(1, maxrows / lv.T);
        lv.S = int(std::max<int64_t>(1, std::min<int64_t>({want, most, kMatrixLevelMaxSplits})));
        lv.nwg = int(per_split) * lv.S;
        lv.run_off.assign(1, 0);
        for (int o = 0; o < O; ++o) {
            int rows = 0;
            for (int i = 0; i < I; ++i) rows += pl.rt[size_t(o) * I + i] >= 0 ? len : 0;
            for (int s = 0; s < lv.S; ++s) {
                const int r0 = int(int64_t(s) * rows / lv.S), r1 = int(int64_t(s + 1) * rows / lv.S);
                int row = 0;
                for (int i = 0; i < I && row < r1; ++i) {
                    const int r = pl.rt[size_t(o) * I + i];
                    if (r < 0) continue;
                    const int x = std::max(r0, row), y = std::min(r1, row + len);
                    if (x < y) {
                        lv.runs.insert(lv.runs.end(), {i, r, lv.a + x - row, lv.a + y - row});
                        lv.fdl_rows += y - x + lv.T - 1;
                    }
                    row += len;
                }
                lv.run_off.push_back(lv.nruns());
            }
        }
        for (int t = 0; t <= lv.T; ++t) lv.part_cut.push_back(int(int64_t(t) * lv.nwg / lv.T));
        lv.filter_rows = int64_t(pl.nroutes) * len;
        lv.slab_off = lp.partial_rows;
        lp.partial_rows += 2 * int64_t(O) * lv.S * lv.T;
        // per block: the window's filter and FDL rows / T, O S partial rows written and O S read
        bytes += 8 * int64_t(B) * (lv.filter_rows + lv.fdl_rows) / lv.T + 8 * int64_t(B) * 2 * O * lv.S;
        lp.levels.push_back(std::move(lv));
    }
    if (lp.levels.empty()) {  // the ordinary step: what neo_hip_matrix_plan's bytes are
        lp.head = P;
        lp.hplan = matrix_plan{};
        bytes = 8 * int64_t(B) * (pl.filter_loads + pl.fdl_loads) + 4 * int64_t(B) * (I + O);
    } else {
        lp.head_bank_bytes = int64_t(pl.nroutes) * lp.head * B * 8;
    }
    lp.partial_bytes = lp.partial_rows * B * 8;
    lp.bytes = bytes;
    return nullptr;
}

// what k_matrix_lvl_mac reads for one level: run_off [O S + 1], then the runs
inline std::vector<int> matrix_level_table(const matrix_level& lv)
{
    std::vector<int> tab(lv.run_off);
    tab.insert(tab.end(), lv.runs.begin(), lv.runs.end());
    return tab;
}

}  // namespace neo_hip
