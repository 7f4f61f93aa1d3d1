// Offline windows through the header API (include/neo/convolution.hpp: upols_multichannel64::offline,
// offline_info; dense_convolve on double arrays with the offline switch). Host part (no GPU): the new
// C calls' argument checks and the plan. GPU part: the 3-channel case of
// tests/golden/upols_f64_offline_case.bin (float64 numpy truth, tools/make_upols_f64_offline_golden.py),
// overlap-save and overlap-add, in calls that hold a window, a batched pass and a remainder, at 1e-12
// of the peak; and the same calls with the mode off within 2e-12 of them.
// Usage: test_f64_offline <path of upols_f64_offline_case.bin>
#include <neo/convolution.hpp>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

static int failures = 0;
#define REQUIRE(cond)                                                   \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

namespace conv = neo::convolution;

static double peak(std::vector<double> const& y, double const* ref)
{
    double e = 0, s = 1e-300;
    for (std::size_t i = 0; i < y.size(); ++i) e = std::max(e, std::abs(y[i] - ref[i])), s = std::max(s, std::abs(ref[i]));
    return e / s;
}

static void test_host()
{
    REQUIRE(neo_hip_version() == NEO_HIP_VERSION && NEO_HIP_VERSION >= 1700);
    REQUIRE(neo_hip_upols64_set_offline(nullptr, 1) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols64_offline_info(nullptr, nullptr, nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
    int t = 0, g = 0;
    std::int64_t spectra = 0, extra = 0, bytes = 0;
    REQUIRE(neo_hip_upols64_offline_plan(3, 24, 70, 0, &t, &g, &spectra, &extra, &bytes) == NEO_HIP_EINVAL);
    REQUIRE(std::string(neo_hip_last_error()) == "block must be a power of two in [16, 4096], got 24");
    REQUIRE(neo_hip_upols64_offline_plan(3, 128, 0, 0, &t, &g, &spectra, &extra, &bytes) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols64_offline_plan(3, 128, 200, 0, &t, &g, &spectra, &extra, &bytes) == NEO_HIP_OK);
    REQUIRE(t == 128 && g == 2);
    REQUIRE(spectra == std::int64_t(16) * 3 * 2 * 256 * 128);
    REQUIRE(extra == 2 * std::int64_t(16) * 3 * 128 * 128);  // scratch and Y; overlap-save has no tails
    REQUIRE(bytes > spectra);
    REQUIRE(neo_hip_upols64_offline_plan(3, 128, 200, 1, &t, &g, &spectra, &extra, &bytes) == NEO_HIP_OK);
    REQUIRE(extra == 2 * std::int64_t(16) * 3 * 128 * 128 + std::int64_t(8) * 3 * 128 * 128);
}

// a [C][n] signal through mc in calls of the given numbers of blocks, each call on a [C][k B] copy
static auto in_calls(conv::upols_multichannel64& mc, std::vector<double> const& x, std::size_t n,
                     std::vector<std::size_t> const& calls) -> std::vector<double>
{
    auto const C = mc.channels(), B = mc.block_size();
    std::vector<double> y(x.size());
    std::size_t done = 0;
    for (std::size_t k : calls) {
        std::vector<double> buf(C * k * B);
        for (std::size_t c = 0; c < C; ++c) std::copy_n(x.data() + c * n + done, k * B, buf.data() + c * k * B);
        mc.process_checked(buf.data(), k * B);
        for (std::size_t c = 0; c < C; ++c) std::copy_n(buf.data() + c * k * B, k * B, y.data() + c * n + done);
        done += k * B;
    }
    REQUIRE(done == n);
    return y;
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
    REQUIRE(C == 3 && B == 16 && P == 129 && nb == 147 && conv::num_partitions(L, B) == P);
    std::vector<double> ir(C * L), x(C * n), want[2] = {std::vector<double>(C * n), std::vector<double>(C * n)};
    REQUIRE(std::fread(ir.data(), 8, ir.size(), f) == ir.size() && std::fread(x.data(), 8, x.size(), f) == x.size());
    for (auto& w : want) REQUIRE(std::fread(w.data(), 8, w.size(), f) == w.size());
    std::fclose(f);

    for (int m = 0; m < 2; ++m) {
        conv::upols_multichannel64 mc(C, B, P, neo::hip::detail::default_device(), m ? conv::method::upola : conv::method::upols);
        mc.impulse(ir.data(), L, false);
        auto const off = mc.offline_info();
        REQUIRE(off.blocks_per_pass == 0 && off.segments == 0 && off.spectra_bytes == 0 && off.extra_bytes == 0);
        mc.offline(true);
        mc.batch(true);
        auto const on = mc.offline_info();
        REQUIRE(on.blocks_per_pass == 128 && on.segments == 2 && on.spectra_bytes == std::int64_t(16) * C * 2 * 256 * B);
        REQUIRE(on.extra_bytes == std::int64_t(C * 128 * B) * (m ? 40 : 32));
        // one call: a window, a batched pass of 16 blocks, three steps
        auto y = in_calls(mc, x, n, {nb});
        double const e = peak(y, want[m].data());
        std::printf("upols_multichannel64 offline %s, one call vs numpy: %.3g\n", m ? "upola" : "upols", e);
        REQUIRE(e <= 1e-12);
        // five steps first, so that the window starts at ring row 5 and the ring wraps inside a pair
        mc.reset();
        auto z = in_calls(mc, x, n, {5, 128, nb - 133});
        double const e2 = peak(z, want[m].data());
        std::printf("upols_multichannel64 offline %s, calls of 5, 128 and %zu blocks vs numpy: %.3g\n", m ? "upola" : "upols",
                    nb - 133, e2);
        REQUIRE(e2 <= 1e-12);
        // both modes off again on the same handle: plain steps, within 2e-12 of the windows
        mc.offline(false);
        mc.batch(false);
        REQUIRE(mc.offline_info().blocks_per_pass == 0);
        mc.reset();
        auto v = in_calls(mc, x, n, {nb});
        REQUIRE(peak(v, want[m].data()) <= 1e-12 && peak(v, y.data()) <= 2e-12);

        // dense_convolve with the switch: the normalized impulse scales the output by one factor
        std::vector<double> d0(C * n), d1(C * n);
        conv::dense_convolve(x.data(), C, n, ir.data(), L, B, d0.data(), m ? conv::method::upola : conv::method::upols);
        conv::dense_convolve(x.data(), C, n, ir.data(), L, B, d1.data(), m ? conv::method::upola : conv::method::upols, true);
        double const e3 = peak(d1, d0.data());
        std::printf("dense_convolve double %s, offline against steps: %.3g\n", m ? "upola" : "upols", e3);
        REQUIRE(e3 <= 2e-12);
        double energy = 0;
        for (std::size_t c = 0; c < C; ++c) {
            double ec = 0;
            for (std::size_t i = 0; i < L; ++i) ec += ir[c * L + i] * ir[c * L + i];
            energy = std::max(energy, ec);
        }
        std::vector<double> scaled(want[m]);
        for (auto& s : scaled) s /= std::sqrt(energy);
        REQUIRE(peak(d1, scaled.data()) <= 1e-12);
    }
}

int main(int argc, char** argv)
{
    test_host();
    int devices = 0;
    if (neo_hip_device_count(&devices) != NEO_HIP_OK || devices < 1) {
        std::printf("no GPU: host checks only, %d failures\n", failures);
        return failures ? 1 : 0;
    }
    if (argc > 1) test_golden(argv[1]);
    else REQUIRE(!"the fixture's path is the first argument");
    if (!failures) std::printf("f64 offline C++ tests passed\n");
    return failures ? 1 : 0;
}
