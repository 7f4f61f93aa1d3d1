// Batched passes of the matrix convolvers of include/neo/convolution.hpp (batch(), batch_info()).
// Host part (no GPU): the header compiles, neo_hip_matrix_batch_plan on a hand-checked route list,
// the argument checks. GPU part: a 2 x 2 and a 3 x 5 case with batch(true) against the oracle's
// dense_convolve applied route by route and summed in double in ascending input order.
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
    REQUIRE(neo_hip_version() == NEO_HIP_VERSION && NEO_HIP_VERSION >= 700);
    // lower-triangular 4 x 4, P = 5, two splits per output (8 workgroups over 4 outputs)
    std::vector<int> ro, ri;
    for (int o = 0; o < 4; ++o)
        for (int i = 0; i <= o; ++i) ro.push_back(o), ri.push_back(i);
    neo_hip_matrix_batch_plan_info info{};
    int rows[4], off[4 * 65], rin[10 + 63 * 4], first[10 + 63 * 4], last[10 + 63 * 4];
    REQUIRE(neo_hip_matrix_batch_plan(4, 4, 64, 5, ro.data(), ri.data(), int(ro.size()), 32, 8, &info, rows, off, rin, first,
                                      last) == NEO_HIP_OK);
    REQUIRE(info.blocks == 32 && info.splits == 2 && info.chunks == 1);
    REQUIRE(rows[0] == 5 && rows[1] == 10 && rows[2] == 15 && rows[3] == 20);
    // output 2: 15 rows cut at 7: (0, 0..5) (1, 0..2) | (1, 2..5) (2, 0..5)
    int const* o2 = off + 2 * 65;
    REQUIRE(o2[1] - o2[0] == 2 && o2[2] - o2[1] == 2);
    REQUIRE(rin[o2[0]] == 0 && first[o2[0]] == 0 && last[o2[0]] == 5);
    REQUIRE(rin[o2[0] + 1] == 1 && first[o2[0] + 1] == 0 && last[o2[0] + 1] == 2);
    REQUIRE(rin[o2[1]] == 1 && first[o2[1]] == 2 && last[o2[1]] == 5);
    REQUIRE(rin[o2[1] + 1] == 2 && first[o2[1] + 1] == 0 && last[o2[1] + 1] == 5);
    REQUIRE(info.filter_row_loads == 50);
    REQUIRE(info.fdl_row_loads == 50 + 31 * info.runs);
    REQUIRE(info.slab_rows == 4 * 2 * 32);
    // argument checks need no device
    REQUIRE(neo_hip_matrix_batch_plan(4, 4, 64, 5, ro.data(), ri.data(), int(ro.size()), 3, 0, &info, nullptr, nullptr,
                                      nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(std::string(neo_hip_last_error()).find("blocks per pass") != std::string::npos);
    REQUIRE(neo_hip_matrix_batch_plan(4, 4, 64, 5, ro.data(), ri.data(), int(ro.size()), 32, -1, &info, nullptr, nullptr,
                                      nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_set_batch(nullptr, 1, 0) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_batch_info(nullptr, nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
}

template<typename Conv>
static void against_oracle(std::size_t I, std::size_t O, std::size_t B, std::size_t P, std::size_t nb,
                           std::vector<matrix_route> const& routes, int ola, int split, std::uint64_t seed)
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

    Conv conv(I, O, B, P);
    conv.filter(reinterpret_cast<cf const*>(parts.data()), routes);
    REQUIRE(conv.batch_info().blocks_per_pass == 1 && conv.batch_info().ring_rows == int(P));
    conv.batch(true, split);
    auto const bi = conv.batch_info();
    REQUIRE(bi.blocks_per_pass == 32 && bi.ring_rows == int(P) + 31 && bi.splits >= 1);
    if (split) REQUIRE(bi.splits > 1);
    std::vector<float> y(O * N);
    conv.process(x.data(), N, y.data(), N, nb);
    double err = 0;
    for (std::size_t k = 0; k < y.size(); ++k) err = std::max(err, std::abs(double(y[k]) - ref[k]));
    std::printf("%zu x %zu B %zu P %zu %s batched, %d splits: peak err %.3g\n", I, O, B, P, ola ? "upola" : "upols",
                bi.splits, err / peak);
    REQUIRE(err <= 1e-5 * peak);
    // again after reset(): the same bits; then in two calls with batching off between them
    conv.reset();
    std::vector<float> y2(O * N);
    conv.process(x.data(), N, y2.data(), N, nb);
    REQUIRE(y2 == y);
    conv.reset();
    std::size_t const n0 = 33;
    conv.process(x.data(), N, y2.data(), N, n0);
    conv.batch(false);
    REQUIRE(conv.batch_info().blocks_per_pass == 1 && conv.batch_info().ring_rows == int(P) + 31);
    conv.process(x.data() + n0 * B, N, y2.data() + n0 * B, N, nb - n0);
    err = 0;
    for (std::size_t k = 0; k < y2.size(); ++k) err = std::max(err, std::abs(double(y2[k]) - ref[k]));
    REQUIRE(err <= 1e-5 * peak);
    REQUIRE(conv.info().fdl_bytes == std::int64_t(I * (P + 31) * B * 8));
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
    std::vector<matrix_route> r35;  // 3 inputs to 5 outputs, output 3 fed by input 1 alone, listed backwards
    for (int o = 4; o >= 0; --o)
        for (int i = 2; i >= 0; --i)
            if (o != 3 || i == 1) r35.push_back({o, i});
    against_oracle<neo::convolution::upols_matrix_convolver>(2, 2, 256, 11, 70, stereo, 0, 0, 1900);
    against_oracle<neo::convolution::upola_matrix_convolver>(2, 2, 256, 11, 70, stereo, 1, 6, 1910);
    against_oracle<neo::convolution::upols_matrix_convolver>(3, 5, 64, 7, 45, r35, 0, 15, 1920);
    against_oracle<neo::convolution::upola_matrix_convolver>(3, 5, 64, 7, 45, r35, 1, 0, 1930);
    std::printf(failures ? "FAILED (%d)\n" : "matrix batch C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
