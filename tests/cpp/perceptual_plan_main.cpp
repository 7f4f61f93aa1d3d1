// Stand-alone host program for neo-dsp_amd/csrc/perceptual_plan.hpp (no GPU, no HIP header):
// weights, mask and histograms of a set of filters against a restatement in double, with guard
// values around every output so that a write past an array shows (build with
// -fsanitize=address,undefined). Exit status 0 = every case agrees.
#include "../../neo-dsp_amd/csrc/perceptual_plan.hpp"

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

static std::uint64_t mix(std::uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static float unit(std::uint64_t seed)  // (-1, 1)
{
    return float(double(mix(seed) >> 11) * (2.0 / 9007199254740992.0) - 1.0);
}

// level in double from the float spectra; band: within 1e-3 dB of `at`
static double level(float re, float im, double maxp, double w)
{
    double const x = (double(re) * re + double(im) * im) / maxp;
    double const l = x > 0.0 ? std::fmax(-144.0, 20.0 * std::log10(x)) : -144.0;
    return l * 0.5 + w;
}

static int bucket(double db)
{
    double const v = -db;
    if (!(v > 0.0)) return 0;
    return v >= 143.0 ? 143 : int(v);
}

static int run(std::string const& name, int C, int B, int P, neo_hip_perceptual const& pp, int zero_channel)
{
    constexpr float fguard = 12345.5f;
    constexpr std::uint8_t bguard = 0xA5;
    constexpr std::int64_t hguard = -77;
    int const bins = B + 1, NT = B / 16;
    std::size_t const n = std::size_t(C) * P * bins;
    std::vector<float> filt(2 * n);
    for (int c = 0; c < C; ++c)
        for (int p = 0; p < P; ++p)
            for (int k = 0; k < bins; ++k) {
                std::size_t const i = (std::size_t(c) * P + p) * bins + k;
                float const decay = std::pow(10.0f, -4.0f * float(p * bins + k) / float(P * bins)) * (c == 1 ? 1e-3f : 1.0f);
                bool const zero = c == zero_channel || (p == P - 1 && P > 2 && k % 3 == 0);
                filt[2 * i] = zero ? 0.0f : decay * unit(i * 2 + 1);
                filt[2 * i + 1] = zero || k == 0 || k == B ? 0.0f : decay * unit(i * 2 + 2);
            }
    std::vector<float> w(std::size_t(bins) + 2, fguard);
    if (!neo_hip::perceptual_weights(B, &pp, w.data() + 1)) return std::printf("FAIL %s: weights refused\n", name.c_str()), 1;
    if (w.front() != fguard || w.back() != fguard) return std::printf("FAIL %s: weights guard\n", name.c_str()), 1;
    int bad = 0;
    for (int k = 0; k < bins; ++k) {
        double want = k < pp.low_bins_to_keep ? 100.0 : pp.weighting ? neo_hip::perc_a_weighting(k * pp.sample_rate / (2.0 * B)) : 0.0;
        float const got = w[std::size_t(k) + 1];
        if (std::isinf(want) ? !(std::isinf(got) && got < 0) : std::fabs(double(got) - want) > 1e-4) ++bad;
    }
    if (bad) return std::printf("FAIL %s: %d weights differ\n", name.c_str(), bad), 1;

    std::vector<std::uint8_t> mask(n + 2, bguard);
    if (!neo_hip::perceptual_mask(filt.data(), C, B, P, &pp, w.data() + 1, mask.data() + 1))
        return std::printf("FAIL %s: mask refused\n", name.c_str()), 1;
    if (mask.front() != bguard || mask.back() != bguard) return std::printf("FAIL %s: mask guard\n", name.c_str()), 1;
    std::vector<std::int64_t> hb(std::size_t(C) * 144 + 2, hguard), ht(std::size_t(C) * 144 + 2, hguard);
    if (!neo_hip::perceptual_histogram(filt.data(), C, B, P, &pp, w.data() + 1, hb.data() + 1, ht.data() + 1))
        return std::printf("FAIL %s: histogram refused\n", name.c_str()), 1;
    if (hb.front() != hguard || hb.back() != hguard || ht.front() != hguard || ht.back() != hguard)
        return std::printf("FAIL %s: histogram guard\n", name.c_str()), 1;

    double const delta = 1e-3;
    for (int c = 0; c < C; ++c) {
        double maxp = 0.0;
        for (std::size_t i = std::size_t(c) * P * bins; i < std::size_t(c + 1) * P * bins; ++i)
            maxp = std::fmax(maxp, double(filt[2 * i]) * filt[2 * i] + double(filt[2 * i + 1]) * filt[2 * i + 1]);
        std::int64_t sum_b = 0, sum_t = 0, lo_t[144] = {}, hi_t[144] = {};
        for (int j = 0; j < 144; ++j) {
            sum_b += hb[std::size_t(c) * 144 + j + 1];
            sum_t += ht[std::size_t(c) * 144 + j + 1];
        }
        if (sum_b != std::int64_t(P) * bins || sum_t != std::int64_t(P) * NT) ++bad;
        for (int p = 0; p < P; ++p) {
            std::size_t const r = (std::size_t(c) * P + p) * bins;
            std::vector<double> top(std::size_t(NT), -INFINITY);
            for (int k = 0; k < bins; ++k) {
                double const db = level(filt[2 * (r + k)], filt[2 * (r + k) + 1], maxp, double(w[std::size_t(k) + 1]));
                bool const keep = db > double(pp.threshold_db);
                if (std::fabs(db - double(pp.threshold_db)) > delta && (mask[r + k + 1] != 0) != keep) ++bad;
                if (mask[r + k + 1] > 1) ++bad;
                int const t = k == B ? 0 : k / 16;
                top[std::size_t(t)] = std::fmax(top[std::size_t(t)], db);
            }
            for (int t = 0; t < NT; ++t) {  // every tile lies in one of the buckets its level allows
                ++lo_t[bucket(top[std::size_t(t)] + delta)];
                ++hi_t[bucket(top[std::size_t(t)] - delta)];
            }
        }
        // cumulative counts: tiles surely in buckets <= j, the histogram's, tiles possibly there
        std::int64_t run = 0, run_lo = 0, run_hi = 0;
        for (int j = 0; j < 144; ++j) {
            run += ht[std::size_t(c) * 144 + j + 1];
            run_lo += lo_t[j];
            run_hi += hi_t[j];
            if (run > run_lo || run < run_hi) ++bad;
        }
    }
    if (bad) return std::printf("FAIL %s: %d disagreements\n", name.c_str(), bad), 1;
    return 0;
}

int main()
{
    int cases = 0, failed = 0;
    struct shape { int C, B, P, zero; };
    for (shape s : {shape{2, 16, 7, -1}, shape{3, 16, 1, 2}, shape{1, 4096, 3, -1}, shape{2, 4096, 1, 0}, shape{3, 128, 9, 2}})
        for (int weighting : {0, 1})
            for (int low : {0, 2, s.B})
                for (float theta : {-20.0f, -60.0f, -80.0f}) {
                    neo_hip_perceptual pp{48000.0, theta, low, weighting};
                    std::string const name = "C" + std::to_string(s.C) + " B" + std::to_string(s.B) + " P" + std::to_string(s.P) +
                                             " w" + std::to_string(weighting) + " low" + std::to_string(low) + " th" +
                                             std::to_string(int(theta));
                    ++cases;
                    failed += run(name, s.C, s.B, s.P, pp, s.zero);
                }
    // refused arguments write nothing
    {
        float w[17];
        std::uint8_t m[17];
        float f[34] = {};
        neo_hip_perceptual good{48000.0, -40.0f, 0, 1}, bad_rate{0.0, -40.0f, 0, 1}, bad_low{48000.0, -40.0f, 17, 1},
            bad_w{48000.0, -40.0f, 0, 3}, bad_th{48000.0, NAN, 0, 1};
        ++cases;
        bool ok = !neo_hip::perceptual_weights(16, &bad_rate, w) && !neo_hip::perceptual_weights(16, &bad_low, w) &&
                  !neo_hip::perceptual_weights(16, &bad_w, w) && !neo_hip::perceptual_weights(16, &bad_th, w) &&
                  !neo_hip::perceptual_weights(24, &good, w) && !neo_hip::perceptual_weights(16, nullptr, w) &&
                  !neo_hip::perceptual_weights(16, &good, nullptr) && neo_hip::perceptual_weights(16, &good, w) &&
                  !neo_hip::perceptual_mask(f, 0, 16, 1, &good, w, m) && !neo_hip::perceptual_mask(f, 1, 16, 0, &good, w, m) &&
                  !neo_hip::perceptual_mask(nullptr, 1, 16, 1, &good, w, m) &&
                  !neo_hip::perceptual_histogram(f, 1, 16, 1, &good, w, nullptr, nullptr);
        if (!ok) {
            std::printf("FAIL argument checks\n");
            ++failed;
        }
    }
    std::printf("%d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
