// sparse_plan.hpp — the tile-compacted sparse filter format, on the host (no HIP header: the
// plan needs no device and a plain C++ compiler builds it).
//
// The reference's sparse_filter (src/neo/convolution/sparse_filter.hpp:25-45) keeps single bins
// in CSR. Here the unit is a TILE: 16 packed complex bins, 128 B, of one packed filter row
// (packed index 0 = {DC, Nyquist}, packed index k = bin k for 1 <= k < B). Reference column
// k in [1, B) lies in tile k / 16; columns 0 (DC) and B (Nyquist) both lie in tile 0. A row has
// NT = B / 16 tiles and a bitmap of NW = max(1, B / 512) uint32 words (tile t = bit t % 32 of
// word t / 32). A tile is kept if the mask keeps any of its columns; dropped columns inside a
// kept tile are stored as zero. Row (c, p) starts at tile row_off[c][p] of channel c's compacted
// values ([C][P + 1], the exclusive prefix sum of the rows' popcounts).
#pragma once

#include <cstdint>

namespace neo_hip {

constexpr int kSparseTile = 16;  // packed complex bins per tile (128 B)

constexpr int sparse_words(int block) { return block / 512 > 1 ? block / 512 : 1; }

constexpr bool sparse_block_ok(int b) { return b >= 16 && b <= 4096 && (b & (b - 1)) == 0; }

// mask [C][P][B + 1] (nonzero = keep) -> tile_mask [C][P][NW], row_off [C][P + 1], the kept
// columns and the kept tiles over all channels. false: bad arguments (nothing written).
inline bool sparse_plan(const uint8_t* mask, int channels, int block, int partitions, uint32_t* tile_mask,
                        uint32_t* row_off, int64_t* kept_bins, int64_t* kept_tiles)
{
    if (!mask || !tile_mask || !row_off || channels < 1 || partitions < 1 || !sparse_block_ok(block)) return false;
    const int NW = sparse_words(block);
    int64_t bins = 0, tiles = 0;
    for (int64_t c = 0; c < channels; ++c) {
        uint32_t off = 0;
        for (int64_t p = 0; p < partitions; ++p) {
            const int64_t r = c * partitions + p;
            const uint8_t* m = mask + r * (int64_t(block) + 1);
            uint32_t* w = tile_mask + r * NW;
            for (int i = 0; i < NW; ++i) w[i] = 0;
            for (int k = 0; k <= block; ++k) {
                if (!m[k]) continue;
                const int t = k == block ? 0 : k / kSparseTile;  // Nyquist shares packed bin 0 with DC
                w[t >> 5] |= uint32_t(1) << (t & 31);
                ++bins;
            }
            row_off[c * (int64_t(partitions) + 1) + p] = off;
            for (int i = 0; i < NW; ++i) off += uint32_t(__builtin_popcount(w[i]));
        }
        row_off[c * (int64_t(partitions) + 1) + partitions] = off;
        tiles += off;
    }
    if (kept_bins) *kept_bins = bins;
    if (kept_tiles) *kept_tiles = tiles;
    return true;
}

constexpr bool sparse_window_ok(int w) { return w >= 2 && w <= 32 && (w & (w - 1)) == 0; }

// The window bitmaps of a batched pass of `window` blocks (upols_sparse_batch.hip): the FDL row
// that enters a workgroup's sliding window at partition p is multiplied by the filter rows
// p .. p + window - 1, so a lane needs its tile only if one of those rows keeps the tile:
// win_mask[c][p] = OR of tile_mask[c][q] over q in [p, min(P, p + window)). window_tiles: the
// popcount sum. tile_mask and win_mask [C][P][NW]; false: bad arguments (nothing written).
inline bool sparse_window_plan(const uint32_t* tile_mask, int channels, int block, int partitions, int window,
                               uint32_t* win_mask, int64_t* window_tiles)
{
    if (!tile_mask || !win_mask || channels < 1 || partitions < 1 || !sparse_block_ok(block) || !sparse_window_ok(window))
        return false;
    const int NW = sparse_words(block);
    int64_t tiles = 0;
    for (int64_t c = 0; c < channels; ++c)
        for (int64_t p = 0; p < partitions; ++p) {
            const int64_t q1 = p + window < partitions ? p + window : partitions;
            for (int i = 0; i < NW; ++i) {
                uint32_t w = 0;
                for (int64_t q = p; q < q1; ++q) w |= tile_mask[(c * partitions + q) * NW + i];
                win_mask[(c * partitions + p) * NW + i] = w;
                tiles += __builtin_popcount(w);
            }
        }
    if (window_tiles) *window_tiles = tiles;
    return true;
}

// One fade step of a live filter update between two sparse filters (upols_sparse_fade.hip): both
// banks run against the same FDL rows, and a lane loads its FDL tile once if either bank keeps it.
// masks [C][P][B + 1] -> the kept tiles of A, of B and of A | B, and the model bytes of the step:
// 128 B per kept tile of each bank and per FDL tile of the union, both banks' bitmap words and
// offsets, the inserted row, the slabs [C][S][2][B] (written, then read by the finish) and the
// block in and out: DESIGN 5.7's "Bytes per step" with two banks. false: bad arguments.
struct sparse_fade_cost {
    int64_t tiles_a = 0, tiles_b = 0, tiles_union = 0, step_bytes = 0;
};
inline bool sparse_fade_plan(const uint8_t* mask_a, const uint8_t* mask_b, int channels, int block, int partitions,
                             int splits, sparse_fade_cost* out)
{
    if (!mask_a || !mask_b || !out || channels < 1 || partitions < 1 || splits < 1 || !sparse_block_ok(block)) return false;
    const int NW = sparse_words(block);
    const int64_t rows = int64_t(channels) * partitions, stride = int64_t(block) + 1;
    sparse_fade_cost f;
    for (int64_t r = 0; r < rows; ++r) {
        uint32_t wa[8] = {}, wb[8] = {};  // NW <= 8 (block <= 4096)
        for (int k = 0; k <= block; ++k) {
            const int t = k == block ? 0 : k / kSparseTile;
            if (mask_a[r * stride + k]) wa[t >> 5] |= uint32_t(1) << (t & 31);
            if (mask_b[r * stride + k]) wb[t >> 5] |= uint32_t(1) << (t & 31);
        }
        for (int i = 0; i < NW; ++i) {
            f.tiles_a += __builtin_popcount(wa[i]);
            f.tiles_b += __builtin_popcount(wb[i]);
            f.tiles_union += __builtin_popcount(wa[i] | wb[i]);
        }
    }
    const int64_t C = channels, B = block;
    f.step_bytes = 128 * (f.tiles_a + f.tiles_b + f.tiles_union) + 2 * rows * (NW + 1) * 4 + C * B * 8 +
                   2 * C * splits * 2 * B * 8 + 2 * C * B * 4;
    *out = f;
    return true;
}

}  // namespace neo_hip
