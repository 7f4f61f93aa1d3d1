// Offline windows of the matrix convolvers of include/neo/convolution.hpp (offline(), offline_info()).
// Host part (no GPU): the header compiles, neo_hip_matrix_offline_plan on hand-checked cases, a
// refused ring, the argument checks. GPU part: a 2 x 2, B = 256, P = 130 case of 384 blocks with
// offline(true) against the oracle's dense_convolve applied route by route and summed in double in
// ascending input order.
#include <neo/convolution.hpp>

#include "../../oracle/neo_oracle.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <string>
#include <vector>

// liboracle.so: dense_convolve with the overlap-add stage (ola = 1), not in the oracle's header
extern "C" int oracle_dense_convolve_method(const float* signal, float* out, const float* parts, size_t C, size_t N,
                                            size_t P, size_t B, int threads, int ola);

static int failures = 0;
#define REQUIRE(cond)                                                   \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

using cf = std::complex<float>;
using neo::convolution::matrix_route;

static void test_host()
{
    REQUIRE(neo_hip_version() == NEO_HIP_VERSION && NEO_HIP_VERSION >= 800);
    int const ro[4] = {0, 0, 1, 1}, ri[4] = {0, 1, 0, 1};
    neo_hip_matrix_offline_plan_info info{};
    int rows[3], of[2 * 2];
    // 2 x 2, P = 130: two segments, three pairs; write position 100 of the least ring of 513 rows
    REQUIRE(neo_hip_matrix_offline_plan(2, 2, 256, 130, ro, ri, 4, 0, 100, 0, &info, rows, of) == NEO_HIP_OK);
    REQUIRE(info.segments == 2 && info.windows == 2 && info.blocks_per_pass == 256 && info.pairs == 3);
    REQUIRE(info.min_ring_rows == 513 && info.ring_rows == 513);
    REQUIRE(rows[0] == 100 && rows[1] == 485 && rows[2] == 357);  // 100 - 128 k mod 513
    REQUIRE(of[0] == 1 && of[1] == 2 && of[2] == 0 && of[3] == 1);
    REQUIRE(info.hf_bytes == 4LL * 2 * 256 * 256 * 8 && info.xf_bytes == 2LL * 3 * 256 * 256 * 8);
    REQUIRE(info.bytes == 8LL * 256 * (4 * 2 * 256 + 4 * 3 * 256 + 2 * 2 * 3 * 256 + 2 * 256 * 2) + 4LL * 256 * 256 * 4);
    REQUIRE(info.cache_bytes == 8LL * 256 * 4 * 3 * 256);
    REQUIRE(neo_hip_matrix_offline_plan(2, 2, 256, 130, ro, ri, 4, 1, 100, 0, &info, rows, of) == NEO_HIP_OK);
    REQUIRE(info.pairs == 2 && info.blocks_per_pass == 128 && rows[0] == 485 && rows[1] == 357 && of[0] == 0 && of[1] == 1);
    // a refused ring: 128 (segments + 2) + 1 rows of 4096 bins span 2 GiB from 65281 partitions on
    REQUIRE(neo_hip_matrix_offline_plan(1, 1, 4096, 65000, ro, ri, 1, 0, 0, 0, &info, nullptr, nullptr) == NEO_HIP_OK);
    REQUIRE(neo_hip_matrix_offline_plan(1, 1, 4096, 65300, ro, ri, 1, 0, 0, 0, &info, nullptr, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(std::string(neo_hip_last_error()).find("2 GiB") != std::string::npos);
    // argument checks need no device
    REQUIRE(neo_hip_matrix_offline_plan(2, 2, 256, 130, ro, ri, 4, 3, 0, 0, &info, nullptr, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(std::string(neo_hip_last_error()).find("windows per pass") != std::string::npos);
    REQUIRE(neo_hip_matrix_offline_plan(2, 2, 256, 130, ro, ri, 4, 0, 513, 0, &info, nullptr, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_offline_plan(2, 2, 256, 130, ro, ri, 4, 0, 0, 512, &info, nullptr, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_set_offline(nullptr, 1, 0) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_offline_info(nullptr, nullptr, nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
}

template<typename Conv>
static void against_oracle(std::size_t I, std::size_t O, std::size_t B, std::size_t P, std::size_t nb,
                           std::vector<matrix_route> const& routes, int ola, std::uint64_t seed)
{
    std::size_t const R = routes.size(), L = B * P, N = B * nb;
    std::vector<float> ir(R * L);
    for (std::size_t r = 0; r < R; ++r) oracle_noise(seed + r, ir.data() + r * L, L);
    oracle_normalize_impulse(ir.data(), R, L);  // one factor over all routes
    std::vector<float> parts(R * P * (B + 1) * 2);
    oracle_uniform_partition(ir.data(), R, L, B, parts.data());
    std::vector<float> x(I * N);
    for (std::size_t i = 0; i < I; ++i) oracle_noise(seed + 100 + i, x.data() + i * N, N);
    std::vector<float> xin(R * N), yr(R * N);
    for (std::size_t r = 0; r < R; ++r) std::copy_n(x.data() + std::size_t(routes[r].in) * N, N, xin.data() + r * N);
    REQUIRE(oracle_dense_convolve_method(xin.data(), yr.data(), parts.data(), R, N, P, B, 1, ola) == 0);
    std::vector<double> ref(O * N, 0.0);
    for (std::size_t o = 0; o < O; ++o)
        for (std::size_t i = 0; i < I; ++i)
            for (std::size_t r = 0; r < R; ++r)
                if (std::size_t(routes[r].out) == o && std::size_t(routes[r].in) == i)
                    for (std::size_t k = 0; k < N; ++k) ref[o * N + k] += yr[r * N + k];
    double peak = 0;
    for (double v : ref) peak = std::max(peak, std::abs(v));
    REQUIRE(peak > 0);

    int const nseg = int((P + 127) / 128), ring = 128 * (nseg + 2) + 1;
    Conv conv(I, O, B, P);
    conv.filter(reinterpret_cast<cf const*>(parts.data()), routes);
    auto oi = conv.offline_info();
    REQUIRE(oi.blocks_per_pass == 0 && oi.segments == nseg && oi.ring_rows == int(P) && oi.spectra_bytes == 0);
    conv.offline(true);
    oi = conv.offline_info();
    REQUIRE(oi.blocks_per_pass == 256 && oi.segments == nseg && oi.ring_rows == ring && oi.spectra_bytes == 0);
    std::vector<float> y(O * N);
    conv.process(x.data(), N, y.data(), N, nb);
    REQUIRE(conv.offline_info().spectra_bytes == std::int64_t(R * nseg * 256 * B * 8));
    REQUIRE(conv.info().offline_bytes > conv.offline_info().spectra_bytes);
    double err = 0;
    for (std::size_t k = 0; k < y.size(); ++k) err = std::max(err, std::abs(double(y[k]) - ref[k]));
    std::printf("%zu x %zu B %zu P %zu %s offline windows: peak err %.3g\n", I, O, B, P, ola ? "upola" : "upols", err / peak);
    REQUIRE(err <= 1e-5 * peak);
    // again after reset(): the same bits; then in two calls, one-window passes in the second
    conv.reset();
    std::vector<float> y2(O * N);
    conv.process(x.data(), N, y2.data(), N, nb);
    REQUIRE(y2 == y);
    conv.reset();
    std::size_t const n0 = 130;
    conv.process(x.data(), N, y2.data(), N, n0);
    conv.offline(true, 1);
    REQUIRE(conv.offline_info().blocks_per_pass == 128 && conv.offline_info().ring_rows == ring);
    conv.process(x.data() + n0 * B, N, y2.data() + n0 * B, N, nb - n0);
    err = 0;
    for (std::size_t k = 0; k < y2.size(); ++k) err = std::max(err, std::abs(double(y2[k]) - ref[k]));
    REQUIRE(err <= 1e-5 * peak);
    REQUIRE(conv.info().fdl_bytes == std::int64_t(I * ring * B * 8));
    bool threw = false;
    try {
        conv.offline(true, 3);
    } catch (std::exception const&) {
        threw = true;
    }
    REQUIRE(threw && conv.offline_info().blocks_per_pass == 128);
}

int main()
{
    test_host();
    int n = 0;
    if (neo_hip_device_count(&n) != NEO_HIP_OK || n < 1) {
        std::printf("no GPU: only host-side checks ran\n");
        return failures ? 1 : 0;
    }
    std::vector<matrix_route> const stereo{{0, 0}, {0, 1}, {1, 0}, {1, 1}};
    against_oracle<neo::convolution::upols_matrix_convolver>(2, 2, 256, 130, 384, stereo, 0, 2900);
    against_oracle<neo::convolution::upola_matrix_convolver>(2, 2, 256, 130, 384, stereo, 1, 2910);
    std::printf(failures ? "FAILED (%d)\n" : "matrix offline C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
