// Batched passes through the header API (include/neo/convolution.hpp: upols_multichannel64::batch,
// batch_info). Host part (no GPU): the new C calls' argument checks and the plan. GPU part: the
// 3-channel case of tests/golden/upols_f64_batch_case.bin (float64 numpy truth,
// tools/make_upols_f64_batch_golden.py), overlap-save and overlap-add, in calls that hold a pass and
// a remainder, at 1e-12 of the peak; and the same calls with batching off within 2e-12 of them.
// Usage: test_f64_batch <path of upols_f64_batch_case.bin>
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
    REQUIRE(neo_hip_upols64_set_batch(nullptr, 1) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols64_batch_info(nullptr, nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
    int t = 0, s = 0, r = 0;
    std::int64_t extra = 0, bytes = 0;
    REQUIRE(neo_hip_upols64_batch_plan(3, 24, 70, 0, 0, 0, &t, &s, &r, &extra, &bytes) == NEO_HIP_EINVAL);
    REQUIRE(std::string(neo_hip_last_error()) == "block must be a power of two in [16, 4096], got 24");
    REQUIRE(neo_hip_upols64_batch_plan(3, 128, 70, 0, 0, 3, &t, &s, &r, &extra, &bytes) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols64_batch_plan(3, 128, 70, 0, 12, 0, &t, &s, &r, &extra, &bytes) == NEO_HIP_OK);
    REQUIRE((t == 8 || t == 16) && s == 4 && r == 18);
    REQUIRE(extra == std::int64_t(16) * 3 * 128 * t * (1 + s));  // scratch and slabs; overlap-save has no tails
    REQUIRE(bytes > 2 * std::int64_t(16) * 3 * 70 * 128);
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
    REQUIRE(C == 3 && B == 64 && P == 21 && nb == 35 && conv::num_partitions(L, B) == P);
    std::vector<double> ir(C * L), x(C * n), want[2] = {std::vector<double>(C * n), std::vector<double>(C * n)};
    REQUIRE(std::fread(ir.data(), 8, ir.size(), f) == ir.size() && std::fread(x.data(), 8, x.size(), f) == x.size());
    for (auto& w : want) REQUIRE(std::fread(w.data(), 8, w.size(), f) == w.size());
    std::fclose(f);

    for (int m = 0; m < 2; ++m) {
        conv::upols_multichannel64 mc(C, B, P, neo::hip::detail::default_device(), m ? conv::method::upola : conv::method::upols);
        mc.impulse(ir.data(), L, false);
        auto const off = mc.batch_info();
        REQUIRE(off.blocks_per_pass == 1 && off.extra_bytes == 0);
        mc.batch(true);
        auto const on = mc.batch_info();
        auto const T = std::size_t(on.blocks_per_pass);
        REQUIRE((T == 8 || T == 16) && on.splits >= 1 && on.extra_bytes > 0 && nb > T + 3);
        // one call: whole passes and a remainder
        auto y = in_calls(mc, x, n, {nb});
        double const e = peak(y, want[m].data());
        std::printf("upols_multichannel64 batch %s, T %zu, one call vs numpy: %.3g\n", m ? "upola" : "upols", T, e);
        REQUIRE(e <= 1e-12);
        // a pass and a remainder, then the rest: other blocks run as passes, the same bar
        mc.reset();
        auto z = in_calls(mc, x, n, {T + 3, nb - T - 3});
        double const e2 = peak(z, want[m].data());
        std::printf("upols_multichannel64 batch %s, calls of %zu and %zu blocks vs numpy: %.3g\n", m ? "upola" : "upols", T + 3,
                    nb - T - 3, e2);
        REQUIRE(e2 <= 1e-12);
        // batching off again on the same handle: plain steps, within 2e-12 of the passes
        mc.batch(false);
        REQUIRE(mc.batch_info().blocks_per_pass == 1);
        mc.reset();
        auto v = in_calls(mc, x, n, {nb});
        REQUIRE(peak(v, want[m].data()) <= 1e-12 && peak(v, y.data()) <= 2e-12);
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
    if (!failures) std::printf("f64 batch C++ tests passed\n");
    return failures ? 1 : 0;
}
