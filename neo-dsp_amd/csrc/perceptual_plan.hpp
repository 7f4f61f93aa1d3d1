// perceptual_plan.hpp — the perceptual sparsity predicate, defined once on the host (no HIP
// header: a plain C++ compiler builds it). It is the plugin's sparse_convolve threshold
// (extra/plugin/src/dsp/DenseConvolution.cpp:110-170 over src/neo/unit/decibel.hpp and
// src/neo/math/a_weighting.hpp) for a filter H[c][p][k], k in [0, B], in uniform_partition's
// layout; the kernels of perceptual.hip reproduce it with the level functions below.
//
//   w[k]     100 for k < low_bins_to_keep; else 0 (weighting 0) or A(k sample_rate / (2 B)),
//            A(0) = -inf; computed in double, rounded to float once
//   power    re^2 + im^2 (float); m_c = max over p, k of power; scale_c = 1 / m_c (per channel)
//   dB       x = power scale_c; x > 0: max(-144, 20 log10 x) 0.5 + w[k]; else (x <= 0, NaN: a
//            zero bin, an all-zero channel's 0 inf) -144 0.5 + w[k]
//   keep     dB > threshold_db
//   tile dB  the maximum of dB over the 16 columns of a tile of the sparse format (sparse_plan.hpp:
//            column B lies in tile 0); bucket j = min(143, floor(max(0, -dB))), -inf -> 143, so
//            that the tiles an integer threshold -k keeps are the sum of the buckets j < k
#pragma once

#include "../../include/neo_hip.h"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NEO_PERC_HD __host__ __device__
#else
#define NEO_PERC_HD
#endif

namespace neo_hip {

constexpr int kPercBuckets = 144;
constexpr int kPercTile = 16;  // kSparseTile: columns per tile

constexpr bool perc_block_ok(int b) { return b >= 16 && b <= 4096 && (b & (b - 1)) == 0; }

// nullptr, or what is wrong with the parameters for blocks of `block`
inline const char* perceptual_check(int block, const neo_hip_perceptual* p)
{
    if (!p) return "null perceptual parameters";
    if (!perc_block_ok(block)) return "block must be a power of two in [16, 4096]";
    if (!(p->sample_rate > 0.0) || !std::isfinite(p->sample_rate)) return "sample_rate must be finite and > 0";
    if (!std::isfinite(p->threshold_db)) return "threshold_db must be finite";
    if (p->low_bins_to_keep < 0 || p->low_bins_to_keep > block) return "low_bins_to_keep must lie in [0, block]";
    if (p->weighting != 0 && p->weighting != 1) return "weighting must be 0 (none) or 1 (A-weighting)";
    return nullptr;
}

// A-weighting in dB at f Hz (a_weighting.hpp), in double; f = 0 gives -inf
inline double perc_a_weighting(double f)
{
    const double c0 = 12194.217 * 12194.217, c1 = 20.598997 * 20.598997, c2 = 107.65265 * 107.65265,
                 c3 = 737.86223 * 737.86223;
    const double f2 = f * f;
    return 2.0 + 20.0 * (std::log10(c0) + 2.0 * std::log10(f2) - std::log10(f2 + c0) - std::log10(f2 + c1) -
                         0.5 * std::log10(f2 + c2) - 0.5 * std::log10(f2 + c3));
}

// weights [B + 1]. false: bad arguments (nothing written).
inline bool perceptual_weights(int block, const neo_hip_perceptual* p, float* weights)
{
    if (!weights || perceptual_check(block, p)) return false;
    for (int k = 0; k <= block; ++k) {
        if (k < p->low_bins_to_keep) weights[k] = 100.0f;
        else if (p->weighting == 0) weights[k] = 0.0f;
        else weights[k] = float(perc_a_weighting(double(k) * p->sample_rate / (2.0 * double(block))));
    }
    return true;
}

NEO_PERC_HD inline float perc_power(float re, float im) { return re * re + im * im; }

// the level of a bin in dB (the "otherwise" branch takes x <= 0 and NaN)
NEO_PERC_HD inline float perc_level(float power, float scale, float w)
{
    const float x = power * scale;
    const float l = x > 0.0f ? fmaxf(-144.0f, 20.0f * log10f(x)) : -144.0f;
    return l * 0.5f + w;
}

NEO_PERC_HD inline int perc_bucket(float db)
{
    const float v = -db;
    if (!(v > 0.0f)) return 0;
    return v >= float(kPercBuckets - 1) ? kPercBuckets - 1 : int(v);
}

// max over p, k of re^2 + im^2 per channel (NaN powers are passed over)
inline void perceptual_max(const float* filter, int C, int B, int P, float* maxp)
{
    const int64_t n = int64_t(P) * (int64_t(B) + 1);
    for (int64_t c = 0; c < C; ++c) {
        const float* f = filter + c * n * 2;
        float m = 0.0f;
        for (int64_t i = 0; i < n; ++i) {
            const float pw = perc_power(f[2 * i], f[2 * i + 1]);
            m = pw > m ? pw : m;
        }
        maxp[c] = m;
    }
}

// filter [C][P][B + 1] complex (interleaved float) -> mask [C][P][B + 1] bytes (1 = keep).
// false: bad arguments (nothing written).
inline bool perceptual_mask(const float* filter, int C, int B, int P, const neo_hip_perceptual* p, const float* weights,
                            uint8_t* mask)
{
    if (!filter || !mask || !weights || C < 1 || P < 1 || perceptual_check(B, p)) return false;
    const int64_t n = int64_t(P) * (int64_t(B) + 1);
    for (int64_t c = 0; c < C; ++c) {
        float m = 0.0f;
        perceptual_max(filter + c * n * 2, 1, B, P, &m);
        const float scale = 1.0f / m;
        const float* f = filter + c * n * 2;
        uint8_t* o = mask + c * n;
        for (int64_t r = 0; r < P; ++r)
            for (int k = 0; k <= B; ++k) {
                const int64_t i = r * (int64_t(B) + 1) + k;
                o[i] = perc_level(perc_power(f[2 * i], f[2 * i + 1]), scale, weights[k]) > p->threshold_db ? 1 : 0;
            }
    }
    return true;
}

// hist_bins, hist_tiles [C][144] (either may be null): counts of the columns and of the tiles per
// level bucket. false: bad arguments (nothing written).
inline bool perceptual_histogram(const float* filter, int C, int B, int P, const neo_hip_perceptual* p,
                                 const float* weights, int64_t* hist_bins, int64_t* hist_tiles)
{
    if (!filter || !weights || (!hist_bins && !hist_tiles) || C < 1 || P < 1 || perceptual_check(B, p)) return false;
    const int64_t n = int64_t(P) * (int64_t(B) + 1);
    const int NT = B / kPercTile;
    for (int64_t c = 0; c < C; ++c) {
        float m = 0.0f;
        perceptual_max(filter + c * n * 2, 1, B, P, &m);
        const float scale = 1.0f / m;
        int64_t* hb = hist_bins ? hist_bins + c * kPercBuckets : nullptr;
        int64_t* ht = hist_tiles ? hist_tiles + c * kPercBuckets : nullptr;
        for (int j = 0; j < kPercBuckets; ++j) {
            if (hb) hb[j] = 0;
            if (ht) ht[j] = 0;
        }
        for (int64_t r = 0; r < P; ++r) {
            const float* f = filter + (c * n + r * (int64_t(B) + 1)) * 2;
            const float last = perc_level(perc_power(f[2 * B], f[2 * B + 1]), scale, weights[B]);
            if (hb) ++hb[perc_bucket(last)];
            for (int t = 0; t < NT; ++t) {
                float top = t == 0 ? last : -INFINITY;  // the Nyquist column shares tile 0 with DC
                for (int k = t * kPercTile; k < (t + 1) * kPercTile; ++k) {
                    const float db = perc_level(perc_power(f[2 * k], f[2 * k + 1]), scale, weights[k]);
                    if (hb) ++hb[perc_bucket(db)];
                    top = fmaxf(top, db);
                }
                if (ht) ++ht[perc_bucket(top)];
            }
        }
    }
    return true;
}

}  // namespace neo_hip
