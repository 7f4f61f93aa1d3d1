// The matrix convolvers of include/neo/convolution.hpp (upols_matrix_convolver,
// upola_matrix_convolver). Host part (no GPU): the header compiles, the plan of a hand-checked
// route list, the argument checks. GPU part: a 2 x 2 and a 3 x 5 case against the oracle's
// dense_convolve applied route by route and summed in double in ascending input order.
#include <neo/convolution.hpp>

#include "../../oracle/neo_oracle.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <stdexcept>
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

static std::vector<float> rnoise(std::uint64_t seed, std::size_t n)
{
    std::vector<float> v(n);
    oracle_noise(seed, v.data(), n);
    return v;
}

static void test_host()
{
    // lower-triangular 4 x 4 in tiles of two outputs: unions {0, 1} and {0, 1, 2, 3}
    std::vector<int> ro, ri;
    for (int o = 0; o < 4; ++o)
        for (int i = 0; i <= o; ++i) ro.push_back(o), ri.push_back(i);
    neo_hip_matrix_opts opts{-1, 0, 2};
    neo_hip_matrix_plan_info info{};
    int first[4], count[4], rows[4], uoff[5], uin[16];
    REQUIRE(neo_hip_matrix_plan(4, 4, 64, 5, ro.data(), ri.data(), int(ro.size()), &opts, &info, first, count, rows, uoff,
                                uin, nullptr) == NEO_HIP_OK);
    REQUIRE(info.out_tile == 2 && info.tiles == 2);
    REQUIRE(first[0] == 0 && count[0] == 2 && rows[0] == 10 && first[1] == 2 && count[1] == 2 && rows[1] == 20);
    REQUIRE(uoff[0] == 0 && uoff[1] == 2 && uoff[2] == 6);
    for (int k = 0; k < 6; ++k) REQUIRE(uin[k] == (k < 2 ? k : k - 2));
    REQUIRE(info.fdl_row_loads == 30 && info.filter_row_loads == 50);
    // argument checks need no device
    ri[1] = ri[2] = 0, ro[1] = ro[2] = 1;
    REQUIRE(neo_hip_matrix_plan(4, 4, 64, 5, ro.data(), ri.data(), int(ro.size()), nullptr, &info, nullptr, nullptr,
                                nullptr, nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(std::string(neo_hip_last_error()).find("duplicate") != std::string::npos);
    neo_hip_matrix* m = nullptr;
    REQUIRE(neo_hip_matrix_create(2, 2, 64, 3, 0, 2, nullptr, &m) == NEO_HIP_EINVAL && !m);
    REQUIRE(neo_hip_matrix_create(2, 2, 500, 3, 0, 0, nullptr, &m) == NEO_HIP_EINVAL && !m);
    bool threw = false;
    try {
        neo::convolution::upols_matrix_convolver bad(2, 2, 48, 3);
    } catch (std::runtime_error const&) {
        threw = true;
    }
    REQUIRE(threw);
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
    // the reference, route by route
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
    std::vector<float> y(O * N), in(I * B), out(O * B);
    for (std::size_t t = 0; t < nb; ++t) {  // block by block through the call operator
        for (std::size_t i = 0; i < I; ++i) std::copy_n(x.data() + i * N + t * B, B, in.data() + i * B);
        conv(in.data(), out.data());
        for (std::size_t o = 0; o < O; ++o) std::copy_n(out.data() + o * B, B, y.data() + o * N + t * B);
    }
    double err = 0;
    for (std::size_t k = 0; k < y.size(); ++k) err = std::max(err, std::abs(double(y[k]) - ref[k]));
    std::printf("%zu x %zu B %zu P %zu %s: peak err %.3g\n", I, O, B, P, ola ? "upola" : "upols", err / peak);
    REQUIRE(err <= 1e-5 * peak);
    // all blocks in one call after reset(): the same bits
    conv.reset();
    std::vector<float> y2(O * N);
    conv.process(x.data(), N, y2.data(), N, nb);
    REQUIRE(y2 == y);
    auto const d = conv.info();
    REQUIRE(d.inputs == int(I) && d.outputs == int(O) && d.routes == int(R) && d.method == ola);
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
    against_oracle<neo::convolution::upols_matrix_convolver>(2, 2, 256, 11, 24, stereo, 0, 900);
    against_oracle<neo::convolution::upola_matrix_convolver>(2, 2, 256, 11, 24, stereo, 1, 910);
    against_oracle<neo::convolution::upols_matrix_convolver>(3, 5, 64, 7, 30, r35, 0, 920);
    against_oracle<neo::convolution::upola_matrix_convolver>(3, 5, 64, 7, 30, r35, 1, 930);
    std::printf(failures ? "FAILED (%d)\n" : "matrix C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
