// matrix_fade.hpp — the gain curve of a live filter update of a matrix convolver
// (upols_matrix_fade.hip): ONE expression for the host (neo_hip_matrix_fade_gains) and the kernel.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NEO_FADE_HD __host__ __device__
#else
#define NEO_FADE_HD
#endif

namespace neo_hip {

constexpr int kMatrixFadeCurves = 2;           // 0 linear, 1 raised cosine
constexpr int kMatrixFadeMaxBlocks = 1 << 20;  // fade_blocks * block stays far below 2^53

// g[n] of a fade of `total` = fade_blocks * block samples, t = n / total: curve 0 g = t, curve 1
// g = 0.5 - 0.5 cos(pi t); evaluated in float64 and rounded to float32 once
NEO_FADE_HD inline float matrix_fade_gain(int64_t n, int64_t total, int curve)
{
    const double t = double(n) / double(total);
    return curve == 0 ? float(t) : float(0.5 - 0.5 * cos(3.14159265358979323846 * t));
}

}  // namespace neo_hip
