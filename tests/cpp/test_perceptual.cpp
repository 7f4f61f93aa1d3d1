// The perceptual sparsity rule through include/neo/convolution.hpp and include/neo/perceptual.hpp.
// Host part (no GPU): the headers compile; neo::a_weighting and neo::amplitude_to_db give the
// reference's values; perceptual_sparsity argument errors throw; the C-ABI host mask keeps what a
// direct evaluation of the rule keeps. GPU part: sparse_upola_convolver::filter(matrix,
// perceptual_sparsity) against the callable form with a lambda that evaluates the host definition.
#include <neo/convolution.hpp>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define REQUIRE(cond)                                                   \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

using cf = std::complex<float>;
using neo::convolution::perceptual_sparsity;

static std::uint64_t mix(std::uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::vector<float> rnoise(std::uint64_t seed, std::size_t n, double decay_db = 0.0)
{
    std::vector<float> v(n);
    for (std::size_t i = 0; i < n; ++i) {
        double const u = double(mix(seed * 0x100000001B3ull + i) >> 11) * (2.0 / 9007199254740992.0) - 1.0;
        v[i] = float(u * std::pow(10.0, -decay_db / 20.0 * double(i) / double(n)));
    }
    return v;
}

template<typename F>
static bool throws_invalid(F&& f)
{
    try {
        f();
    } catch (std::invalid_argument const&) {
        return true;
    } catch (...) {
        return false;
    }
    return false;
}

static void test_host()
{
    // the scalar helpers
    REQUIRE(std::abs(neo::a_weighting(1000.0)) <= 0.01);
    REQUIRE(std::abs(neo::a_weighting(1000.0F)) <= 0.01F);
    REQUIRE(std::abs(neo::a_weighting(100.0) + 19.1) < 0.1);
    REQUIRE(std::isinf(neo::a_weighting(0.0)) && neo::a_weighting(0.0) < 0);
    REQUIRE(neo::amplitude_to_db(1.0F) == 0.0F);
    REQUIRE(std::abs(neo::amplitude_to_db(10.0F) - 20.0F) <= 4e-6F);
    REQUIRE(neo::amplitude_to_db(0.0F) == -144.0F);
    REQUIRE(neo::amplitude_to_db(1e-9F) == -144.0F);
    REQUIRE(neo::amplitude_to_db(-1.0) == -144.0);
    REQUIRE(std::abs(neo::amplitude_to_db(1e-9, -200.0) + 180.0) <= 1e-9);
    static_assert(std::same_as<decltype(neo::amplitude_to_db(1.0F)), float>);
    static_assert(std::same_as<decltype(neo::a_weighting(1.0)), double>);

    // argument errors throw, and name the reason
    std::size_t const B = 32;
    perceptual_sparsity{48000.0, -40.0F, 0, 1}.validate(B);
    perceptual_sparsity{44100.0, -90.0F, int(B), 0}.validate(B);
    REQUIRE(throws_invalid([&] { perceptual_sparsity{0.0, -40.0F, 0, 1}.validate(B); }));
    REQUIRE(throws_invalid([&] { perceptual_sparsity{48000.0, NAN, 0, 1}.validate(B); }));
    REQUIRE(throws_invalid([&] { perceptual_sparsity{48000.0, -40.0F, -1, 1}.validate(B); }));
    REQUIRE(throws_invalid([&] { perceptual_sparsity{48000.0, -40.0F, int(B) + 1, 1}.validate(B); }));
    REQUIRE(throws_invalid([&] { perceptual_sparsity{48000.0, -40.0F, 0, 2}.validate(B); }));
    REQUIRE(throws_invalid([&] { perceptual_sparsity{48000.0, -40.0F, 0, 1}.validate(24); }));
    try {
        perceptual_sparsity{48000.0, -40.0F, 99, 1}.validate(B);
    } catch (std::invalid_argument const& e) {
        REQUIRE(std::strstr(e.what(), "low_bins_to_keep") != nullptr);
    }

    // the C-ABI host mask on a filter whose levels are known: bin (p, k) at -10 (p + 1) dB, unweighted
    std::size_t const P = 5;
    std::vector<cf> filt(P * (B + 1));
    for (std::size_t p = 0; p < P; ++p)
        for (std::size_t k = 0; k <= B; ++k) filt[p * (B + 1) + k] = cf{float(std::pow(10.0, -0.5 * double(p))), 0.0F};
    filt[3 * (B + 1) + 7] = cf{0.0F, 0.0F};  // a zero bin: the floor, -72 dB
    std::vector<std::uint8_t> mask(P * (B + 1));
    auto const p25 = perceptual_sparsity{48000.0, -25.0F, 0, 0}.c_struct();
    REQUIRE(neo_hip_perceptual_mask_host(filt.data(), 1, int(B), int(P), &p25, mask.data()) == NEO_HIP_OK);
    for (std::size_t p = 0; p < P; ++p)
        for (std::size_t k = 0; k <= B; ++k)
            REQUIRE(mask[p * (B + 1) + k] == (p < 3 ? 1 : 0));  // 0, -10, -20 dB pass; -30, -40 and the zero do not
    auto const p80 = perceptual_sparsity{48000.0, -80.0F, 0, 0}.c_struct();
    REQUIRE(neo_hip_perceptual_mask_host(filt.data(), 1, int(B), int(P), &p80, mask.data()) == NEO_HIP_OK);
    REQUIRE(std::all_of(mask.begin(), mask.end(), [](std::uint8_t m) { return m == 1; }));  // zeros included
    std::vector<std::int64_t> hb(144), ht(144);
    REQUIRE(neo_hip_perceptual_hist_host(filt.data(), 1, int(B), int(P), &p25, hb.data(), ht.data()) == NEO_HIP_OK);
    REQUIRE(ht[0] == std::int64_t(B / 16) && ht[10] + ht[9] == std::int64_t(B / 16) && hb[72] == 1);
    // refused before a device is touched
    REQUIRE(neo_hip_perceptual_mask(nullptr, 1, int(B), int(P), &p25, mask.data(), 0, 0) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_set_filter_perceptual(nullptr, filt.data(), &p25, 0) == NEO_HIP_EINVAL);
}

template<typename Conv>
static std::vector<float> run(Conv& conv, std::vector<float> const& signal, std::size_t B)
{
    auto out = signal;
    for (std::size_t i = 0; i < out.size(); i += B) conv(neo::hip::make_view(out.data() + i, B));
    return out;
}

static void device_route_equals_callable(std::size_t B, std::size_t P, perceptual_sparsity const& sp)
{
    std::size_t const bins = B + 1, nb = 30;
    auto ir = rnoise(B + P, B * P, 60.0);
    auto parts = neo::convolution::uniform_partition(neo::hip::make_matrix_view(ir.data(), 1, B * P), B);
    cf* filt = parts.data();
    auto const pp = sp.c_struct();
    std::vector<std::uint8_t> host(P * bins), dev(P * bins);
    REQUIRE(neo_hip_perceptual_mask_host(filt, 1, int(B), int(P), &pp, host.data()) == NEO_HIP_OK);
    REQUIRE(neo_hip_perceptual_mask(filt, 1, int(B), int(P), &pp, dev.data(), 0, 0) == NEO_HIP_OK);
    std::size_t differ = 0, kept = 0;
    for (std::size_t i = 0; i < host.size(); ++i) {
        differ += host[i] != dev[i];
        kept += host[i];
    }
    std::printf("B %zu P %zu: kept %zu of %zu, device and host masks differ on %zu\n", B, P, kept, host.size(), differ);
    REQUIRE(kept > 0 && kept < host.size());
    REQUIRE(differ * 1000 <= host.size());  // only bins within rounding of the threshold
    auto const signal = rnoise(99 + B, B * nb);
    neo::convolution::sparse_upola_convolver<cf> a, b;
    a.filter(neo::hip::make_matrix_view(filt, P, bins), sp);
    // the callable form on the host definition (on the device's own mask where the two differ on
    // a bin at the threshold): the same kernels on the same tiles, no tolerance
    auto const& want = differ ? dev : host;
    b.filter(neo::hip::make_matrix_view(filt, P, bins),
             [&](std::size_t r, std::size_t c, cf) { return want[r * bins + c] != 0; });
    auto const ya = run(a, signal, B), yb = run(b, signal, B);
    REQUIRE(std::memcmp(ya.data(), yb.data(), ya.size() * sizeof(float)) == 0);
    float peak = 0;
    for (float v : ya) peak = std::max(peak, std::abs(v));
    REQUIRE(peak > 0);
}

int main()
{
    test_host();
    int n = 0;
    if (neo_hip_device_count(&n) != NEO_HIP_OK || n < 1) {
        std::printf(failures ? "FAILED (%d)\n" : "perceptual host checks passed\nno GPU: only host-side checks ran\n", failures);
        return failures ? 1 : 0;
    }
    device_route_equals_callable(128, 9, perceptual_sparsity{48000.0, -40.0F, 0, 1});
    device_route_equals_callable(1024, 20, perceptual_sparsity{44100.0, -30.0F, 2, 1});
    device_route_equals_callable(128, 9, perceptual_sparsity{48000.0, -50.0F, 0, 0});
    std::printf(failures ? "FAILED (%d)\n" : "perceptual host checks passed\nperceptual C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
