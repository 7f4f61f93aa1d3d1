// SPDX-License-Identifier: MIT
// neo/perceptual.hpp — the two scalar helpers behind the plugin's perceptual threshold, on the
// host, with the reference's names and signatures:
//   neo::a_weighting<Float>(frequency)             src/neo/math/a_weighting.hpp
//   neo::amplitude_to_db<Float>(gain[, infinity])  src/neo/unit/decibel.hpp (the accurate form)
// The device applies the threshold from an uploaded weight table (include/neo_hip.h,
// neo_hip_perceptual); these are for callers that want the same numbers on the host.
#pragma once

#include <cmath>
#include <concepts>

namespace neo {

/// A-weighting in dB at `frequency` Hz (0 dB near 1 kHz; -inf at 0 Hz)
template<std::floating_point Float>
[[nodiscard]] auto a_weighting(Float frequency) noexcept -> Float
{
    Float const c0 = Float(12194.217) * Float(12194.217), c1 = Float(20.598997) * Float(20.598997),
                c2 = Float(107.65265) * Float(107.65265), c3 = Float(737.86223) * Float(737.86223);
    Float const f2 = frequency * frequency;
    return Float(2) + Float(20) * (std::log10(c0) + Float(2) * std::log10(f2) - std::log10(f2 + c0) - std::log10(f2 + c1) -
                                   Float(0.5) * std::log10(f2 + c2) - Float(0.5) * std::log10(f2 + c3));
}

/// 20 log10(gain), never below `infinity`, which is also the value for gain <= 0
template<std::floating_point Float>
[[nodiscard]] auto amplitude_to_db(Float gain, Float infinity) noexcept -> Float
{
    if (gain <= Float(0)) return infinity;
    Float const db = Float(20) * std::log10(gain);
    return db > infinity ? db : infinity;
}

template<std::floating_point Float>
[[nodiscard]] auto amplitude_to_db(Float gain) noexcept -> Float
{
    return amplitude_to_db(gain, Float(-144));
}

}  // namespace neo
