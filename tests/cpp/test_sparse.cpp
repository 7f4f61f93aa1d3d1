// The sparse convolver aliases of include/neo/convolution.hpp (sparse_upols_convolver,
// sparse_upola_convolver; the reference instantiates both next to the dense ones,
// uniform_partitioned_convolver_test.cpp:35-75). Host part (no GPU): the header compiles, the
// sparsity predicate is applied to the right (row, col, value), and the host plan of that mask
// counts what it keeps. GPU part: the reference's identity test through both aliases, and a
// predicate against the dense alias on the zeroed filter.
#include <neo/convolution.hpp>

#include "../../oracle/neo_oracle.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
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

static std::vector<float> rnoise(std::uint64_t seed, std::size_t n)
{
    std::vector<float> v(n);
    oracle_noise(seed, v.data(), n);
    return v;
}

static double max_abs_diff(std::vector<float> const& a, std::vector<float> const& b)
{
    double m = 0;
    for (std::size_t i = 0; i < a.size(); ++i) m = std::max(m, double(std::abs(a[i] - b[i])));
    return m;
}

static bool keep_thirds(std::size_t row, std::size_t col, cf) { return row == 0 || col % 3 == 0; }

static void test_predicate_host()
{
    std::size_t const P = 4, B = 32;
    std::vector<cf> filt(P * (B + 1));
    for (std::size_t p = 0; p < P; ++p)
        for (std::size_t k = 0; k <= B; ++k) filt[p * (B + 1) + k] = cf{float(p), float(k)};
    // the predicate sees (row, col, filter(row, col))
    std::size_t calls = 0;
    bool right_value = true;
    auto mask = neo::convolution::sparsity_mask(neo::hip::make_matrix_view(filt.data(), P, B + 1),
                                                [&](std::size_t r, std::size_t c, cf v) {
                                                    ++calls;
                                                    right_value = right_value && v == cf{float(r), float(c)};
                                                    return keep_thirds(r, c, v);
                                                });
    REQUIRE(calls == P * (B + 1));
    REQUIRE(right_value);
    REQUIRE(mask.size() == P * (B + 1));
    std::int64_t want = 0;
    for (std::size_t p = 0; p < P; ++p)
        for (std::size_t k = 0; k <= B; ++k) {
            REQUIRE(mask[p * (B + 1) + k] == (keep_thirds(p, k, cf{}) ? 1 : 0));
            want += keep_thirds(p, k, cf{});
        }
    // the host plan of that mask: every tile kept (each holds a multiple of 3), offsets 0, 2, 4, 6, 8
    std::vector<std::uint32_t> bits(P), off(P + 1);
    std::int64_t bins = 0, tiles = 0;
    REQUIRE(neo_hip_upols_sparse_plan(mask.data(), 1, int(B), int(P), bits.data(), off.data(), &bins, &tiles) == NEO_HIP_OK);
    REQUIRE(bins == want);
    REQUIRE(tiles == std::int64_t(P * (B / 16)));
    for (std::size_t p = 0; p < P; ++p) REQUIRE(bits[p] == 3u && off[p] == 2 * p);
    REQUIRE(off[P] == 2 * P);
    // argument checks need no device
    neo_hip_upols* h = nullptr;
    REQUIRE(neo_hip_upols_create_sparse(1, 500, 3, 0, 0, nullptr, &h) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_create_sparse(1, 512, 3, 0, 2, nullptr, &h) == NEO_HIP_EINVAL);
}

template<typename Conv>
static void identity()
{
    for (std::size_t B : {128, 256, 512, 1024}) {
        std::vector<cf> filt(3 * (B + 1), cf{0, 0});
        for (std::size_t k = 0; k <= B; ++k) filt[k] = cf{1, 0};  // generate_identity_impulse
        auto const signal = rnoise(B, B * 20);
        auto output = signal;
        Conv conv;
        conv.filter(neo::hip::make_matrix_view(filt.data(), 3, B + 1), [](auto, auto, auto) { return true; });
        for (std::size_t i = 0; i < output.size(); i += B) conv(neo::hip::make_view(output.data() + i, B));
        REQUIRE(max_abs_diff(output, signal) <= 1e-5);
    }
}

template<typename Sparse, typename Dense>
static void predicate_vs_dense(std::uint64_t seed)
{
    std::size_t const B = 256, P = 11, nb = 30;
    auto ir = rnoise(seed, B * P);
    oracle_normalize_impulse(ir.data(), 1, B * P);
    std::vector<float> parts(P * (B + 1) * 2);
    oracle_uniform_partition(ir.data(), 1, B * P, B, parts.data());
    auto* filt = reinterpret_cast<cf*>(parts.data());
    std::vector<cf> zeroed(filt, filt + P * (B + 1));
    for (std::size_t p = 0; p < P; ++p)
        for (std::size_t k = 0; k <= B; ++k)
            if (!keep_thirds(p, k, cf{})) zeroed[p * (B + 1) + k] = cf{0, 0};
    auto const signal = rnoise(seed + 1, B * nb);
    auto a = signal, b = signal;
    Sparse sp;
    sp.filter(neo::hip::make_matrix_view(filt, P, B + 1), keep_thirds);
    Dense de;
    de.filter(neo::hip::make_matrix_view(zeroed.data(), P, B + 1));
    for (std::size_t i = 0; i < a.size(); i += B) {
        sp(neo::hip::make_view(a.data() + i, B));
        de(neo::hip::make_view(b.data() + i, B));
    }
    double peak = 0;
    for (float r : b) peak = std::max(peak, double(std::abs(r)));
    REQUIRE(peak > 0);
    REQUIRE(max_abs_diff(a, b) <= 1e-5 * peak);
}

int main()
{
    test_predicate_host();
    int n = 0;
    if (neo_hip_device_count(&n) != NEO_HIP_OK || n < 1) {
        std::printf("no GPU: only host-side checks ran\n");
        return failures ? 1 : 0;
    }
    identity<neo::convolution::sparse_upols_convolver<cf>>();
    identity<neo::convolution::sparse_upola_convolver<cf>>();
    predicate_vs_dense<neo::convolution::sparse_upols_convolver<cf>, neo::convolution::split_upols_convolver<cf>>(71);
    predicate_vs_dense<neo::convolution::sparse_upola_convolver<cf>, neo::convolution::split_upola_convolver<cf>>(73);
    std::printf(failures ? "FAILED (%d)\n" : "sparse C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
