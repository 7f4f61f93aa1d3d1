// The double-precision convolvers of include/neo/convolution.hpp. Host part (no GPU): the header
// compiles for std::complex<double>, the result types of the free functions, the argument checks.
// GPU part: the reference's identity test (uniform_partitioned_convolver_test.cpp) over
// upols_convolver, upola_convolver, split_upols_convolver and split_upola_convolver of
// std::complex<double>; upols_multichannel64 with 3 channels against the float64 numpy truth of
// tests/golden/upols_f64_case.bin (tools/make_upols_f64_golden.py); the free functions on double views.
// Usage: test_f64 <path of upols_f64_case.bin>
#include <neo/convolution.hpp>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <random>
#include <stdexcept>
#include <type_traits>
#include <vector>

static int failures = 0;
#define REQUIRE(cond)                                                   \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

using cd = std::complex<double>;
namespace conv = neo::convolution;

// the free functions follow the view's value_type, as the reference's Float = InMat::value_type
static_assert(std::is_same_v<decltype(conv::uniform_partition(neo::hip::view2d<double>{}, 16)), neo::hip::array<cd, 3>>);
static_assert(std::is_same_v<decltype(conv::uniform_partition(neo::hip::view2d<double const>{}, 16)), neo::hip::array<cd, 3>>);
static_assert(std::is_same_v<decltype(conv::uniform_partition(neo::hip::view2d<float>{}, 16)),
                             neo::hip::array<std::complex<float>, 3>>);
static_assert(std::is_same_v<conv::upols_convolver<cd>::real_type, double>);

static double peak(std::vector<double> const& y, double const* ref)
{
    double e = 0, s = 1e-300;
    for (std::size_t i = 0; i < y.size(); ++i) e = std::max(e, std::abs(y[i] - ref[i])), s = std::max(s, std::abs(ref[i]));
    return e / s;
}

static void test_host()
{
    neo_hip_upols64* h = nullptr;
    REQUIRE(neo_hip_upols64_create(1, 24, 3, 0, 0, 0, &h) == NEO_HIP_EINVAL && !h);
    REQUIRE(std::string(neo_hip_last_error()) == "block must be a power of two in [16, 4096], got 24");
    REQUIRE(neo_hip_upols64_create(1, 64, 3, 0, 2, 0, &h) == NEO_HIP_EINVAL && !h);
    int s = 0, r = 0;
    std::int64_t bytes = 0;
    REQUIRE(neo_hip_upols64_plan(3, 128, 70, 12, &s, &r, &bytes) == NEO_HIP_OK && s == 4 && r == 18);
    bool threw = false;
    try {
        conv::upols_multichannel64 bad(2, 48, 3);
    } catch (std::runtime_error const&) {
        threw = true;
    }
    REQUIRE(threw);
    threw = false;
    try {
        conv::upols_multichannel64 bad(2, 64, 3, 0, conv::method::ols);
    } catch (std::invalid_argument const&) {
        threw = true;
    }
    REQUIRE(threw);
    threw = false;
    try {
        conv::upols_convolver<cd> c;
        c.latency_mode(true);
    } catch (std::invalid_argument const&) {
        threw = true;
    }
    REQUIRE(threw);
}

// an identity filter of 3 partitions, 20 blocks, output equal to input within 1e-12 absolute
template<typename Convolver>
static void identity(char const* name)
{
    for (std::size_t B : {128, 256, 512, 1024}) {
        std::vector<cd> filt(3 * (B + 1), cd{0.0, 0.0});
        std::fill(filt.begin(), filt.begin() + std::ptrdiff_t(B + 1), cd{1.0, 0.0});
        Convolver c;
        c.filter(neo::hip::make_matrix_view(filt.data(), 3, B + 1));
        std::mt19937_64 rng{B};
        std::uniform_real_distribution<double> dist{-1.0, 1.0};
        double worst = 0;
        for (int t = 0; t < 20; ++t) {
            std::vector<double> x(B);
            for (auto& v : x) v = dist(rng);
            auto y = x;
            c(neo::hip::make_view(y.data(), B));
            for (std::size_t i = 0; i < B; ++i) worst = std::max(worst, std::abs(y[i] - x[i]));
        }
        std::printf("%s identity B %zu: max abs %.3g\n", name, B, worst);
        REQUIRE(worst <= 1e-12);
        // a strided block goes through the gather / scatter path
        std::vector<double> wide(2 * B, 0.25), keep(wide);
        c(neo::hip::make_strided_view(wide.data(), B, 2));
        for (std::size_t i = 0; i < B; ++i) REQUIRE(wide[2 * i + 1] == keep[2 * i + 1]);
    }
}

static void test_golden(char const* path)
{
    std::FILE* f = std::fopen(path, "rb");
    REQUIRE(f != nullptr);
    if (!f) return;
    std::int64_t hd[5] = {};
    REQUIRE(std::fread(hd, sizeof(std::int64_t), 5, f) == 5);
    auto const C = std::size_t(hd[0]), B = std::size_t(hd[1]), P = std::size_t(hd[2]), nb = std::size_t(hd[3]),
               L = std::size_t(hd[4]), n = nb * B;
    REQUIRE(C == 3 && B == 64 && P == 5 && conv::num_partitions(L, B) == P);
    std::vector<double> ir(C * L), x(C * n), want[2] = {std::vector<double>(C * n), std::vector<double>(C * n)};
    REQUIRE(std::fread(ir.data(), 8, ir.size(), f) == ir.size() && std::fread(x.data(), 8, x.size(), f) == x.size());
    for (auto& w : want) REQUIRE(std::fread(w.data(), 8, w.size(), f) == w.size());
    std::fclose(f);

    // the free function on a double view gives the filter in double
    auto H = conv::uniform_partition(neo::hip::make_matrix_view(ir.data(), C, L), B);
    REQUIRE(H.extent(0) == C && H.extent(1) == P && H.extent(2) == B + 1);
    for (int m = 0; m < 2; ++m) {
        conv::upols_multichannel64 mc(C, B, P, neo::hip::detail::default_device(), m ? conv::method::upola : conv::method::upols);
        REQUIRE(mc.channels() == C && mc.block_size() == B && mc.partitions() == P && mc.splits().first >= 1);
        mc.filter(H.data());
        auto y = x;
        mc.process(y.data(), n);  // one call of nb blocks
        double const e = peak(y, want[m].data());
        std::printf("upols_multichannel64 %s vs numpy: %.3g\n", m ? "upola" : "upols", e);
        REQUIRE(e <= 1e-12);
        // reset, then block by block through operator(): the same bits
        mc.reset();
        std::vector<double> z(C * n), blk(C * B);
        for (std::size_t t = 0; t < nb; ++t) {
            for (std::size_t c = 0; c < C; ++c) std::copy_n(x.data() + c * n + t * B, B, blk.data() + c * B);
            mc(blk.data());
            for (std::size_t c = 0; c < C; ++c) std::copy_n(blk.data() + c * B, B, z.data() + c * n + t * B);
        }
        REQUIRE(z == y);
        // impulse() without normalization is uniform_partition + filter
        mc.impulse(ir.data(), L, false);
        auto v = x;
        mc.process_checked(v.data(), n);
        REQUIRE(v == y);
        bool threw = false;
        try {
            mc.process_checked(v.data(), B + 1);
        } catch (std::runtime_error const&) {
            threw = true;
        }
        REQUIRE(threw);
    }

    // normalize_impulse on double views: min factor over channels; one channel: unit energy
    auto nir = ir;
    conv::normalize_impulse(neo::hip::make_matrix_view(nir.data(), C, L));
    double fmin = 1e300;
    for (std::size_t c = 0; c < C; ++c) {
        double e = 0;
        for (std::size_t i = 0; i < L; ++i) e += ir[c * L + i] * ir[c * L + i];
        fmin = std::min(fmin, 1.0 / std::sqrt(e));
    }
    std::vector<double> scaled(ir);
    for (auto& v : scaled) v *= fmin;
    REQUIRE(peak(nir, scaled.data()) <= 1e-12);
    std::vector<double> one(ir.begin(), ir.begin() + std::ptrdiff_t(L));
    conv::normalize_impulse(neo::hip::make_matrix_view(one.data(), 1, L));
    double e1 = 0;
    for (double v : one) e1 += v * v;
    REQUIRE(std::abs(e1 - 1.0) <= 1e-12);

    // dense_convolve in double: normalized impulse, ragged tail
    std::size_t const N = n - 29;
    std::vector<double> sig(C * N), out(C * N), ref(C * N);
    for (std::size_t c = 0; c < C; ++c) std::copy_n(x.data() + c * n, N, sig.data() + c * N);
    conv::dense_convolve(sig.data(), C, N, ir.data(), L, B, out.data());
    for (std::size_t c = 0; c < C; ++c) std::transform(want[0].begin() + std::ptrdiff_t(c * n), want[0].begin() + std::ptrdiff_t(c * n + N),
                                                       ref.begin() + std::ptrdiff_t(c * N), [&](double v) { return v * fmin; });
    double const ed = peak(out, ref.data());
    std::printf("dense_convolve (double) vs numpy: %.3g\n", ed);
    REQUIRE(ed <= 1e-12);
}

int main(int argc, char** argv)
{
    test_host();
    int devices = 0;
    if (neo_hip_device_count(&devices) != NEO_HIP_OK || devices < 1) {
        std::printf("no GPU: host checks only, %d failures\n", failures);
        return failures ? 1 : 0;
    }
    identity<conv::upols_convolver<cd>>("upols_convolver");
    identity<conv::upola_convolver<cd>>("upola_convolver");
    identity<conv::split_upols_convolver<cd>>("split_upols_convolver");
    identity<conv::split_upola_convolver<cd>>("split_upola_convolver");
    if (argc > 1) test_golden(argv[1]);
    else REQUIRE(!"the fixture's path is the first argument");
    if (!failures) std::printf("f64 C++ tests passed\n");
    return failures ? 1 : 0;
}
