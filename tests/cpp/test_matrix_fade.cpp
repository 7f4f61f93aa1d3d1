// Live filter updates of the matrix convolvers of include/neo/convolution.hpp (update_filter(),
// update_impulse(), fade_info(), fade_curve). Host part (no GPU): the header compiles,
// neo_hip_matrix_fade_gains against its closed form, the argument checks. GPU part: 2 x 2, B = 32,
// P = 5: filter A, 7 blocks, update_filter(B, 3 blocks, cosine), 13 blocks more; the outputs go to
// the files named on the command line (upols, upola: raw float32 [2][20 * 32]), where
// tests/test_matrix_fade_cpp.py compares them with the Python path's bits.
#include <neo/convolution.hpp>

#include "../../oracle/neo_oracle.h"

#include <cmath>
#include <complex>
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

using cf = std::complex<float>;
using neo::convolution::fade_curve;
using neo::convolution::matrix_route;

static void test_host()
{
    REQUIRE(neo_hip_version() == NEO_HIP_VERSION && NEO_HIP_VERSION >= 900);
    REQUIRE(int(fade_curve::linear) == 0 && int(fade_curve::cosine) == 1);
    int const B = 32, F = 3;
    std::vector<float> g(B * F), c(B * F);
    REQUIRE(neo_hip_matrix_fade_gains(B, F, 0, g.data()) == NEO_HIP_OK);
    REQUIRE(neo_hip_matrix_fade_gains(B, F, 1, c.data()) == NEO_HIP_OK);
    double const pi = 3.14159265358979323846;
    for (int n = 0; n < B * F; ++n) {
        double const t = double(n) / (B * F);
        REQUIRE(std::abs(double(g[n]) - t) <= 1.2e-7 * t);
        REQUIRE(std::abs(double(c[n]) - (0.5 - 0.5 * std::cos(pi * t))) <= 1.2e-7);
        REQUIRE(g[n] < 1.0f && c[n] < 1.0f);
    }
    REQUIRE(g[0] == 0.0f && c[0] == 0.0f);
    REQUIRE(neo_hip_matrix_fade_gains(B, 0, 0, g.data()) == NEO_HIP_EINVAL);
    REQUIRE(std::string(neo_hip_last_error()).find("fade_blocks") != std::string::npos);
    REQUIRE(neo_hip_matrix_fade_gains(B, F, 2, g.data()) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_fade_gains(48, F, 0, g.data()) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_update_filter(nullptr, g.data(), 0, 1, 0, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_update_impulse(nullptr, g.data(), 32, 1, 0, 1, 0, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_fade_info(nullptr, nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
}

// the seeds and shapes tests/test_matrix_fade_cpp.py repeats
constexpr std::size_t kI = 2, kO = 2, kB = 32, kP = 5, kBlocks = 20, kAt = 7;
constexpr int kFade = 3;

static std::vector<float> partitions(std::uint64_t seed, std::size_t R)
{
    std::size_t const L = kB * kP;
    std::vector<float> ir(R * L);
    for (std::size_t r = 0; r < R; ++r) oracle_noise(seed + r, ir.data() + r * L, L);
    oracle_normalize_impulse(ir.data(), R, L);
    std::vector<float> parts(R * kP * (kB + 1) * 2);
    oracle_uniform_partition(ir.data(), R, L, kB, parts.data());
    return parts;
}

template<typename Conv>
static void run(char const* path)
{
    std::vector<matrix_route> const routes{{0, 0}, {0, 1}, {1, 0}, {1, 1}};
    std::size_t const N = kB * kBlocks;
    auto const pa = partitions(4100, routes.size()), pb = partitions(4200, routes.size());
    std::vector<float> x(kI * N);
    for (std::size_t i = 0; i < kI; ++i) oracle_noise(4300 + i, x.data() + i * N, N);

    Conv conv(kI, kO, kB, kP);
    bool threw = false;
    try {
        conv.update_filter(reinterpret_cast<cf const*>(pb.data()));  // before a filter is set
    } catch (std::runtime_error const&) {
        threw = true;
    }
    REQUIRE(threw);
    conv.filter(reinterpret_cast<cf const*>(pa.data()), routes);
    REQUIRE(conv.fade_info().remaining_blocks == 0 && conv.fade_info().bank_bytes == 0);
    std::vector<float> y(kO * N);
    conv.process(x.data(), N, y.data(), N, kAt);
    conv.update_filter(reinterpret_cast<cf const*>(pb.data()), kFade, fade_curve::cosine);
    auto const fi = conv.fade_info();
    REQUIRE(fi.remaining_blocks == kFade && fi.fade_blocks == kFade && fi.bank_bytes == conv.info().filter_bytes);
    threw = false;
    try {
        conv.update_filter(reinterpret_cast<cf const*>(pa.data()));  // a fade is running
    } catch (std::runtime_error const&) {
        threw = true;
    }
    REQUIRE(threw);
    conv.process(x.data() + kAt * kB, N, y.data() + kAt * kB, N, kBlocks - kAt);
    REQUIRE(conv.fade_info().remaining_blocks == 0 && conv.fade_info().fade_blocks == 0);
    std::FILE* f = std::fopen(path, "wb");
    REQUIRE(f != nullptr);
    if (f) {
        REQUIRE(std::fwrite(y.data(), sizeof(float), y.size(), f) == y.size());
        std::fclose(f);
    }
}

int main(int argc, char** argv)
{
    test_host();
    int n = 0;
    if (neo_hip_device_count(&n) != NEO_HIP_OK || n < 1) {
        std::printf("no GPU: only host-side checks ran\n");
        return failures ? 1 : 0;
    }
    if (argc != 3) {  // test_matrix_fade <upols output file> <upola output file> runs the device part
        std::printf("no output files named: only host-side checks ran\n");
        return failures ? 1 : 0;
    }
    run<neo::convolution::upols_matrix_convolver>(argv[1]);
    run<neo::convolution::upola_matrix_convolver>(argv[2]);
    std::printf(failures ? "FAILED (%d)\n" : "matrix fade C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
