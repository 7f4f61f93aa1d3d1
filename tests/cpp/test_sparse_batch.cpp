// The C++ sparse_convolve (include/neo/convolution.hpp: the plugin's loop on a sparse handle with
// batched passes) against the oracle on the masked filter, both overloads (a mask of the caller's,
// the plugin's perceptual rule) and both methods; upols_multichannel::batch on a sparse handle.
// Without a GPU only the host-side checks run.
#include <neo/convolution.hpp>

#include "../../oracle/neo_oracle.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

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
namespace nc = neo::convolution;

static std::vector<float> rnoise(std::uint64_t seed, std::size_t n)
{
    std::vector<float> v(n);
    oracle_noise(seed, v.data(), n);
    return v;
}

static void test_window_plan_host()
{
    // rows keep tiles {0}, {1}, {}, {0, 1}: windows of 2 rows
    std::uint32_t const bits[4] = {1u, 2u, 0u, 3u};
    std::uint32_t win[4] = {9, 9, 9, 9};
    std::int64_t tiles = -1;
    REQUIRE(neo_hip_upols_sparse_window_plan(bits, 1, 32, 4, 2, win, &tiles) == NEO_HIP_OK);
    REQUIRE(win[0] == 3u && win[1] == 2u && win[2] == 3u && win[3] == 3u && tiles == 7);
    REQUIRE(neo_hip_upols_sparse_window_plan(bits, 1, 32, 4, 3, win, &tiles) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_sparse_batch_info(nullptr, nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
}

// peak-normalized error of got against the oracle's dense_convolve on parts * mask, N samples
static double oracle_err(std::vector<float> const& signal, std::vector<float> const& got, std::vector<cf> const& parts,
                         std::vector<std::uint8_t> const& mask, std::size_t C, std::size_t N, std::size_t P,
                         std::size_t B, bool ola)
{
    std::size_t const nb = (N + B - 1) / B, M = nb * B;
    std::vector<cf> masked(parts);
    for (std::size_t i = 0; i < masked.size(); ++i)
        if (!mask[i]) masked[i] = cf{0, 0};
    std::vector<float> pad(C * M, 0.0F), ref(C * M);
    for (std::size_t c = 0; c < C; ++c) std::copy(signal.begin() + c * N, signal.begin() + (c + 1) * N, pad.begin() + c * M);
    REQUIRE(oracle_dense_convolve_method(pad.data(), ref.data(), reinterpret_cast<float const*>(masked.data()), C, M, P, B, 1,
                                         ola ? 1 : 0) == 0);
    double peak = 0, err = 0;
    for (std::size_t c = 0; c < C; ++c)
        for (std::size_t i = 0; i < N; ++i) {
            peak = std::max(peak, double(std::abs(ref[c * M + i])));
            err = std::max(err, double(std::abs(ref[c * M + i] - got[c * N + i])));
        }
    REQUIRE(peak > 0);
    return err / peak;
}

static void test_sparse_convolve()
{
    // 38 blocks: batches of 32, 4 and 2; the last block zero-padded
    std::size_t const C = 2, B = 256, L = 2560, N = B * 37 + 77, P = nc::num_partitions(L, B);
    std::vector<float> ir(C * L), signal(C * N);
    for (std::size_t c = 0; c < C; ++c) {
        auto const a = rnoise(60 + c, L), s = rnoise(70 + c, N);
        std::copy(a.begin(), a.end(), ir.begin() + c * L);
        std::copy(s.begin(), s.end(), signal.begin() + c * N);
    }
    // the filter as sparse_convolve makes it
    auto h = ir;
    REQUIRE(neo_hip_normalize_impulse(h.data(), int(C), std::int64_t(L), 0, 0) == NEO_HIP_OK);
    std::vector<cf> parts(C * P * (B + 1));
    REQUIRE(neo_hip_uniform_partition(h.data(), int(C), std::int64_t(L), int(B), parts.data(), 0, 0) == NEO_HIP_OK);
    // a threshold on the bins, as the plugin's: the stronger half
    std::vector<float> mag(parts.size());
    for (std::size_t i = 0; i < parts.size(); ++i) mag[i] = std::abs(parts[i]);
    auto sorted = mag;
    std::nth_element(sorted.begin(), sorted.begin() + sorted.size() / 2, sorted.end());
    std::vector<std::uint8_t> mask(parts.size());
    for (std::size_t i = 0; i < parts.size(); ++i) mask[i] = mag[i] > sorted[sorted.size() / 2];
    for (auto m : {nc::method::upola, nc::method::upols}) {
        std::vector<float> out(C * N, -1.0F);
        nc::sparse_convolve(signal.data(), C, N, ir.data(), L, B, mask.data(), out.data(), m);
        double const e = oracle_err(signal, out, parts, mask, C, N, P, B, m == nc::method::upola);
        std::printf("sparse_convolve mask %s: peak err %.3g\n", m == nc::method::upola ? "upola" : "upols", e);
        REQUIRE(e <= 1e-5);
    }
    {
        std::vector<float> out(C * N, -1.0F);
        nc::sparse_convolve(signal.data(), C, N, ir.data(), L, B, mask.data(), out.data());  // method::upola by default
        REQUIRE(oracle_err(signal, out, parts, mask, C, N, P, B, true) <= 1e-5);
    }
    // the plugin's own rule: the mask the device makes from the same partitions
    nc::perceptual_sparsity const sp{48000.0, -40.0F, 2, 1};
    auto const pc = sp.c_struct();
    std::vector<std::uint8_t> pmask(parts.size());
    REQUIRE(neo_hip_perceptual_mask(parts.data(), int(C), int(B), int(P), &pc, pmask.data(), 0, 0) == NEO_HIP_OK);
    std::size_t kept = 0;
    for (auto v : pmask) kept += v;
    REQUIRE(kept > 0 && kept < pmask.size());
    for (auto m : {nc::method::upola, nc::method::upols}) {
        std::vector<float> out(C * N, -1.0F);
        nc::sparse_convolve(signal.data(), C, N, ir.data(), L, B, sp, out.data(), m);
        double const e = oracle_err(signal, out, parts, pmask, C, N, P, B, m == nc::method::upola);
        std::printf("sparse_convolve perceptual %s: peak err %.3g\n", m == nc::method::upola ? "upola" : "upols", e);
        REQUIRE(e <= 1e-5);
    }
    // batch(bool) on a handle of one's own: on, off, on again across one signal
    {
        std::size_t const M = B * 38;
        nc::upols_multichannel conv{nc::sparse, C, B, P, 0, nc::method::upols};
        conv.filter_sparse(parts.data(), mask.data());
        std::vector<float> pad(C * M, 0.0F);
        for (std::size_t c = 0; c < C; ++c) std::copy(signal.begin() + c * N, signal.begin() + (c + 1) * N, pad.begin() + c * M);
        auto run = [&](std::size_t b0, std::size_t b1) {
            std::size_t const n = (b1 - b0) * B;
            std::vector<float> buf(C * n);
            for (std::size_t c = 0; c < C; ++c) std::copy_n(pad.begin() + c * M + b0 * B, n, buf.begin() + c * n);
            conv.process_checked(buf.data(), n);
            for (std::size_t c = 0; c < C; ++c) std::copy_n(buf.begin() + c * n, n, pad.begin() + c * M + b0 * B);
        };
        conv.batch(true);
        run(0, 20);
        conv.batch(false);
        run(20, 23);
        conv.batch(true);
        run(23, 38);
        std::vector<float> got(C * N);
        for (std::size_t c = 0; c < C; ++c) std::copy_n(pad.begin() + c * M, N, got.begin() + c * N);
        REQUIRE(oracle_err(signal, got, parts, mask, C, N, P, B, false) <= 1e-5);
    }
}

int main()
{
    test_window_plan_host();
    int n = 0;
    if (neo_hip_device_count(&n) != NEO_HIP_OK || n < 1) {
        std::printf("no GPU: only host-side checks ran\n");
        return failures ? 1 : 0;
    }
    test_sparse_convolve();
    std::printf(failures ? "FAILED (%d)\n" : "sparse batch C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
