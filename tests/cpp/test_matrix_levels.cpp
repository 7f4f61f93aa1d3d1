// Window levels of the matrix convolvers of include/neo/convolution.hpp (levels(), levels_info()).
// Host part (no GPU): the header compiles, neo_hip_matrix_level_plan on a hand-checked case, the
// argument checks. GPU part: a 2 x 2 and a 3 x 5 case with levels(true), one block per call, against
// the block step of a second convolver of the same type at 1e-5 of the peak, and the info call.
#include <neo/convolution.hpp>

#include "../../oracle/neo_oracle.h"

#include <algorithm>
#include <array>
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
using neo::convolution::matrix_route;

static void test_host()
{
    REQUIRE(neo_hip_version() == NEO_HIP_VERSION && NEO_HIP_VERSION >= 1000);
    // dense 2 x 2, P = 70, the windows 4, 8, 16, 32: head 8, bands [8, 16) [16, 32) [32, 64) [64, 70)
    int const ro[] = {0, 0, 1, 1}, ri[] = {0, 1, 0, 1};
    neo_hip_matrix_level_plan_info info{};
    std::vector<int> cuts(5 * 33), off(5 * (64 * 2 + 1)), rin(5 * (4 + 63 * 2)), first(rin.size()), last(rin.size());
    int const four[] = {4, 8, 16, 32};
    REQUIRE(neo_hip_matrix_level_plan(2, 2, 32, 70, ro, ri, 4, four, 4, 0, &info, cuts.data(), off.data(), rin.data(),
                                      first.data(), last.data()) == NEO_HIP_OK);
    REQUIRE(info.levels == 4 && info.head == 8 && info.ring_rows == 70 && info.chunks == 1);
    int const T[] = {4, 8, 16, 32}, a[] = {8, 16, 32, 64}, b[] = {16, 32, 64, 70};
    std::int64_t partial = 0;
    for (int l = 0; l < 4; ++l) {
        REQUIRE(info.window[l] == T[l] && info.first[l] == a[l] && info.last[l] == b[l]);
        REQUIRE(info.workgroups[l] == 2 * info.splits[l] && info.filter_rows[l] == 4 * (b[l] - a[l]));
        REQUIRE(cuts[33 * l] == 0 && cuts[33 * l + T[l]] == info.workgroups[l]);
        // the first run of output 0: input 0 from the band's first partition
        REQUIRE(rin[l * (4 + 63 * 2)] == 0 && first[l * (4 + 63 * 2)] == a[l]);
        partial += 2 * 2 * std::int64_t(info.splits[l]) * T[l] * 32 * 8;
    }
    REQUIRE(info.partial_bytes == partial && info.head_bank_bytes == 4 * 8 * 32 * 8);
    int const one[] = {32};
    REQUIRE(neo_hip_matrix_level_plan(2, 2, 32, 70, ro, ri, 4, one, 1, 0, &info, nullptr, nullptr, nullptr, nullptr,
                                      nullptr) == NEO_HIP_OK);
    REQUIRE(info.levels == 1 && info.head == 64 && info.first[0] == 64 && info.last[0] == 70);
    REQUIRE(neo_hip_matrix_level_plan(2, 2, 32, 8, ro, ri, 4, nullptr, 0, 0, &info, nullptr, nullptr, nullptr, nullptr,
                                      nullptr) == NEO_HIP_OK);
    REQUIRE(info.levels == 0 && info.head == 8);
    // the default list is (8, 32)
    REQUIRE(neo_hip_matrix_level_plan(2, 2, 32, 70, ro, ri, 4, nullptr, 0, 0, &info, nullptr, nullptr, nullptr, nullptr,
                                      nullptr) == NEO_HIP_OK);
    REQUIRE(info.levels == 2 && info.head == 16 && info.window[0] == 8 && info.last[0] == 64 && info.window[1] == 32);
    // argument checks need no device
    int const bad[] = {8, 4};
    REQUIRE(neo_hip_matrix_level_plan(2, 2, 32, 70, ro, ri, 4, bad, 2, 0, &info, nullptr, nullptr, nullptr, nullptr,
                                      nullptr) == NEO_HIP_EINVAL);
    REQUIRE(std::string(neo_hip_last_error()).find("windows must ascend") != std::string::npos);
    REQUIRE(neo_hip_matrix_level_plan(2, 2, 32, 70, ro, ri, 4, nullptr, 0, -1, &info, nullptr, nullptr, nullptr, nullptr,
                                      nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_set_levels(nullptr, 1, nullptr, 0, 0) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_matrix_levels_info(nullptr, nullptr) == NEO_HIP_EINVAL);
}

template<typename Conv>
static void against_block_step(std::size_t I, std::size_t O, std::size_t B, std::size_t P, std::size_t nb,
                               std::vector<matrix_route> const& routes, std::vector<int> const& windows, int split,
                               std::uint64_t seed, char const* name)
{
    std::size_t const R = routes.size(), L = B * P, N = B * nb;
    std::vector<float> ir(R * L);
    for (std::size_t r = 0; r < R; ++r) oracle_noise(seed + r, ir.data() + r * L, L);
    oracle_normalize_impulse(ir.data(), R, L);  // one factor over all routes
    std::vector<float> parts(R * P * (B + 1) * 2);
    oracle_uniform_partition(ir.data(), R, L, B, parts.data());
    std::vector<float> x(I * N);
    for (std::size_t i = 0; i < I; ++i) oracle_noise(seed + 100 + i, x.data() + i * N, N);

    Conv plain(I, O, B, P);
    plain.filter(reinterpret_cast<cf const*>(parts.data()), routes);
    std::vector<float> ref(O * N);
    plain.process(x.data(), N, ref.data(), N, nb);
    double peak = 0;
    for (float v : ref) peak = std::max(peak, std::abs(double(v)));
    REQUIRE(peak > 0);

    Conv conv(I, O, B, P);
    REQUIRE(conv.levels_info().enabled == 0 && conv.levels_info().levels == 0);  // no filter yet
    conv.filter(reinterpret_cast<cf const*>(parts.data()), routes);
    conv.levels(true, windows, split);
    auto const li = conv.levels_info();
    REQUIRE(li.enabled == 1 && li.levels >= 1 && li.ring_rows == int(P) && li.primed == 1);
    REQUIRE(li.head == 2 * (windows.empty() ? 8 : windows[0]) && li.first[0] == li.head && li.last[li.levels - 1] == int(P));
    REQUIRE(li.partial_bytes > 0 && li.head_bank_bytes == std::int64_t(R * std::size_t(li.head) * B * 8));
    if (split) REQUIRE(li.splits[li.levels - 1] > 1);
    std::vector<float> y(O * N), in(I * B), out(O * B);
    for (std::size_t n = 0; n < nb; ++n) {  // one block per call, as a plugin calls it
        for (std::size_t i = 0; i < I; ++i) std::copy_n(x.data() + i * N + n * B, B, in.data() + i * B);
        conv(in.data(), out.data());
        for (std::size_t o = 0; o < O; ++o) std::copy_n(out.data() + o * B, B, y.data() + o * N + n * B);
    }
    double err = 0;
    for (std::size_t k = 0; k < y.size(); ++k) err = std::max(err, std::abs(double(y[k]) - double(ref[k])));
    std::printf("%zu x %zu B %zu P %zu %s levels %d, head %d: peak err %.3g\n", I, O, B, P, name, li.levels, li.head, err / peak);
    REQUIRE(err <= 1e-5 * peak);
    REQUIRE(conv.levels_info().primed == 1);
    // again after reset(), all blocks in one call: the same bits; then off mid-stream
    conv.reset();
    std::vector<float> y2(O * N);
    conv.process(x.data(), N, y2.data(), N, nb);
    REQUIRE(y2 == y);
    conv.reset();
    std::size_t const n0 = 13;
    conv.process(x.data(), N, y2.data(), N, n0);
    conv.levels(false);
    REQUIRE(conv.levels_info().enabled == 0);
    conv.process(x.data() + n0 * B, N, y2.data() + n0 * B, N, nb - n0);
    err = 0;
    for (std::size_t k = 0; k < y2.size(); ++k) err = std::max(err, std::abs(double(y2[k]) - double(ref[k])));
    REQUIRE(err <= 1e-5 * peak);
    REQUIRE(conv.info().fdl_bytes == std::int64_t(I * P * B * 8));
    bool threw = false;
    try {
        std::array<int, 2> const bad{8, 4};
        conv.levels(true, bad);
    } catch (std::runtime_error const&) {
        threw = true;
    }
    REQUIRE(threw && conv.levels_info().enabled == 0);
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
    against_block_step<neo::convolution::upols_matrix_convolver>(2, 2, 256, 70, 100, stereo, {}, 0, 2900, "upols");
    against_block_step<neo::convolution::upola_matrix_convolver>(2, 2, 256, 70, 100, stereo, {8, 32}, 3, 2910, "upola");
    against_block_step<neo::convolution::upols_matrix_convolver>(3, 5, 64, 37, 60, r35, {2, 8}, 4, 2920, "upols");
    against_block_step<neo::convolution::upola_matrix_convolver>(3, 5, 64, 37, 60, r35, {4, 8, 16, 32}, 0, 2930, "upola");
    std::printf(failures ? "FAILED (%d)\n" : "matrix levels C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
