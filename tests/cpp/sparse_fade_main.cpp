// Live filter updates of the sparse convolvers of include/neo/convolution.hpp. Host part (no GPU):
// the header compiles, null handles are EINVAL. GPU part, B = 32, P = 5, 24 blocks:
//   1. sparse_upola_convolver (one channel): filter(A, predicate), 7 blocks, update_filter(B, another
//      predicate, 3 blocks, cosine), 17 blocks more; an update before filter() and one while a fade
//      runs throw;
//   2. upols_multichannel (sparse, 3 channels): impulse_perceptual(A), 7 blocks,
//      update_impulse_perceptual(B under another threshold, 2 blocks, linear), 17 blocks more (the
//      impulses normalised on the host).
// The outputs go to the two files named on the command line (raw float32 [1][24 * 32] and
// [3][24 * 32]), where tests/test_sparse_fade_cpp.py compares them with the Python path's bits.
#include <neo/convolution.hpp>

#include "../../oracle/neo_oracle.h"

#include <complex>
#include <cstdio>
#include <cstring>
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
using neo::convolution::method;
using neo::convolution::perceptual_sparsity;

static void test_host()
{
    REQUIRE(neo_hip_version() == NEO_HIP_VERSION && NEO_HIP_VERSION >= 1400);
    float x[8] = {};
    std::uint8_t m[8] = {};
    neo_hip_perceptual const pp{48000.0, -40.0F, 0, 1};
    std::int64_t t = 0;
    REQUIRE(neo_hip_upols_update_filter_sparse(nullptr, x, m, 0, 1, 0, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_update_filter_perceptual(nullptr, x, &pp, 0, 1, 0, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_update_impulse_perceptual(nullptr, x, 8, 1, &pp, 0, 1, 0, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_sparse_fade_plan(nullptr, m, 1, 16, 1, &t, nullptr, nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
}

// the seeds and shapes tests/test_sparse_fade_cpp.py repeats
constexpr std::size_t kB = 32, kP = 5, kBlocks = 24, kAt = 7, kBins = kB + 1;
constexpr std::size_t kL = kB * kP, kN = kB * kBlocks;

static std::vector<float> impulse(std::uint64_t seed, std::size_t C)
{
    std::vector<float> ir(C * kL);
    for (std::size_t c = 0; c < C; ++c) oracle_noise(seed + c, ir.data() + c * kL, kL);
    oracle_normalize_impulse(ir.data(), C, kL);
    return ir;
}

static std::vector<float> partitions(std::uint64_t seed)
{
    auto const ir = impulse(seed, 1);
    std::vector<float> parts(kP * kBins * 2);
    oracle_uniform_partition(ir.data(), 1, kL, kB, parts.data());
    return parts;
}

static void write(char const* path, std::vector<float> const& y)
{
    bool any = false;
    for (float v : y) any = any || v != 0.0f;
    REQUIRE(any);
    std::FILE* f = std::fopen(path, "wb");
    REQUIRE(f != nullptr);
    if (f) {
        REQUIRE(std::fwrite(y.data(), sizeof(float), y.size(), f) == y.size());
        std::fclose(f);
    }
}

static void run_predicate(char const* path)
{
    auto pa = partitions(6100), pb = partitions(6200);
    auto A = neo::hip::make_matrix_view(reinterpret_cast<cf*>(pa.data()), kP, kBins);
    auto Bm = neo::hip::make_matrix_view(reinterpret_cast<cf*>(pb.data()), kP, kBins);
    auto keep_a = [](std::size_t r, std::size_t c, cf) { return (r + c) % 3 != 0; };
    auto keep_b = [](std::size_t r, std::size_t c, cf) { return c % 2 == 0 || r == 1; };
    neo::convolution::sparse_upola_convolver<cf> conv;
    bool threw = false;
    try {
        conv.update_filter(Bm, keep_b);  // before filter()
    } catch (std::runtime_error const&) {
        threw = true;
    }
    REQUIRE(threw);
    conv.filter(A, keep_a);
    REQUIRE(conv.fade_info().remaining_blocks == 0 && conv.fade_info().bank_bytes == 0);
    std::vector<float> y(kN);
    oracle_noise(6400, y.data(), kN);
    for (std::size_t b = 0; b < kBlocks; ++b) {
        if (b == kAt) {
            conv.update_filter(Bm, keep_b, 3, fade_curve::cosine);
            auto const fi = conv.fade_info();
            REQUIRE(fi.remaining_blocks == 3 && fi.fade_blocks == 3 && fi.bank_bytes > 0);
        }
        if (b == kAt + 1) {
            threw = false;
            try {
                conv.update_filter(A, keep_a);  // a fade is running
            } catch (std::runtime_error const&) {
                threw = true;
            }
            REQUIRE(threw && conv.fade_info().remaining_blocks == 2);
        }
        conv(neo::hip::make_view(y.data() + b * kB, kB));
    }
    REQUIRE(conv.fade_info().remaining_blocks == 0);
    write(path, y);
}

static void run_impulse(char const* path)
{
    constexpr std::size_t C = 3;
    auto const ira = impulse(6500, C), irb = impulse(6600, C);
    perceptual_sparsity const sa{48000.0, -20.0F, 0, 1}, sb{48000.0, -8.0F, 2, 1};
    neo::convolution::upols_multichannel conv(neo::convolution::sparse, C, kB, kP, 0, method::upols);
    conv.impulse_perceptual(ira.data(), kL, sa, false);
    auto const kept_a = conv.sparse_kept();
    std::vector<float> x(C * kN), y(C * kN);
    for (std::size_t c = 0; c < C; ++c) oracle_noise(6700 + c, x.data() + c * kN, kN);
    auto stretch = [&](std::size_t b0, std::size_t b1) {
        std::size_t const n = (b1 - b0) * kB;
        std::vector<float> io(C * n);
        for (std::size_t c = 0; c < C; ++c) std::memcpy(io.data() + c * n, x.data() + c * kN + b0 * kB, n * sizeof(float));
        conv.process(io.data(), n);
        for (std::size_t c = 0; c < C; ++c) std::memcpy(y.data() + c * kN + b0 * kB, io.data() + c * n, n * sizeof(float));
    };
    stretch(0, kAt);
    conv.update_impulse_perceptual(irb.data(), kL, sb, false, 2, fade_curve::linear);
    REQUIRE(conv.fade_info().remaining_blocks == 2 && conv.fade_info().bank_bytes > 0);
    auto const kept_b = conv.sparse_kept();  // the bank being faded to
    REQUIRE(kept_b != kept_a && kept_b.first > 0);
    stretch(kAt, kBlocks);
    REQUIRE(conv.fade_info().remaining_blocks == 0 && conv.sparse_kept() == kept_b);
    write(path, y);
}

int main(int argc, char** argv)
{
    test_host();
    int n = 0;
    if (neo_hip_device_count(&n) != NEO_HIP_OK || n < 1) {
        std::printf("no GPU: only host-side checks ran\n");
        return failures ? 1 : 0;
    }
    if (argc != 3) {  // sparse_fade_main <predicate output file> <impulse output file> runs the device part
        std::printf("no output files named: only host-side checks ran\n");
        return failures ? 1 : 0;
    }
    run_predicate(argv[1]);
    run_impulse(argv[2]);
    std::printf(failures ? "FAILED (%d)\n" : "sparse fade C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
