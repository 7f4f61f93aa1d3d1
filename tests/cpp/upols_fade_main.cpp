// Live filter updates of the dense convolvers of include/neo/convolution.hpp
// (upols_multichannel / upols_multidevice: update_filter(), update_impulse(), fade_info()) against
// the C calls they wrap. Host part (no GPU): the header compiles, null handles are EINVAL. GPU
// part: 3 channels, B = 32, P = 5: filter A, 7 blocks, update_filter(B, 3 blocks, cosine), 6 blocks,
// update_impulse(C, 2 blocks, linear; the impulse normalised on the host), 8 blocks more -- once through the C++ classes and once
// through neo_hip_upols_* directly; the two must agree bit for bit, and the sharded class (devices
// {0, 0}) with the unsharded one. The C++ outputs go to the files named on the command line (upols,
// upola: raw float32 [3][24 * 32]), where tests/test_upols_fade_cpp.py compares them with the
// Python path's bits.
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

static void test_host()
{
    REQUIRE(neo_hip_version() == NEO_HIP_VERSION && NEO_HIP_VERSION >= 1300);
    float x[8] = {};
    REQUIRE(neo_hip_upols_update_filter(nullptr, x, 0, 1, 0, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_update_impulse(nullptr, x, 8, 1, 0, 1, 0, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_fade_info(nullptr, nullptr, nullptr, nullptr) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_multi_update_filter(nullptr, x, 1, 0) == NEO_HIP_EINVAL);
    REQUIRE(neo_hip_upols_multi_update_impulse(nullptr, x, 8, 1, 1, 0) == NEO_HIP_EINVAL);
    neo::convolution::fade_desc d{1, 2, 3};
    REQUIRE(d.remaining_blocks == 1 && d.fade_blocks == 2 && d.bank_bytes == 3);
}

// the seeds and shapes tests/test_upols_fade_cpp.py repeats
constexpr std::size_t kC = 3, kB = 32, kP = 5, kBlocks = 24, kAt1 = 7, kAt2 = 16;
constexpr int kFade1 = 3, kFade2 = 2;
constexpr std::size_t kL = kB * kP, kN = kB * kBlocks;

static std::vector<float> impulse(std::uint64_t seed)
{
    std::vector<float> ir(kC * kL);
    for (std::size_t c = 0; c < kC; ++c) oracle_noise(seed + c, ir.data() + c * kL, kL);
    return ir;
}

static std::vector<float> partitions(std::uint64_t seed)
{
    auto ir = impulse(seed);
    oracle_normalize_impulse(ir.data(), kC, kL);
    std::vector<float> parts(kC * kP * (kB + 1) * 2);
    oracle_uniform_partition(ir.data(), kC, kL, kB, parts.data());
    return parts;
}

template<typename Conv>
static std::vector<float> run_cpp(Conv& conv, std::vector<float> const& x)
{
    auto const pa = partitions(5100), pb = partitions(5200);
    auto irc = impulse(5300);
    oracle_normalize_impulse(irc.data(), kC, kL);
    bool threw = false;
    try {
        conv.update_filter(reinterpret_cast<cf const*>(pb.data()));  // before a filter is set
    } catch (std::runtime_error const&) {
        threw = true;
    }
    REQUIRE(threw);
    conv.filter(reinterpret_cast<cf const*>(pa.data()));
    REQUIRE(conv.fade_info().remaining_blocks == 0 && conv.fade_info().bank_bytes == 0);
    // process() takes contiguous [C][n]: cut the signal into the three stretches
    std::vector<float> y(kC * kN);
    auto stretch = [&](std::size_t b0, std::size_t b1) {
        std::size_t const n = (b1 - b0) * kB;
        std::vector<float> io(kC * n);
        for (std::size_t c = 0; c < kC; ++c) std::memcpy(io.data() + c * n, x.data() + c * kN + b0 * kB, n * sizeof(float));
        conv.process(io.data(), n);
        for (std::size_t c = 0; c < kC; ++c) std::memcpy(y.data() + c * kN + b0 * kB, io.data() + c * n, n * sizeof(float));
    };
    stretch(0, kAt1);
    conv.update_filter(reinterpret_cast<cf const*>(pb.data()), kFade1, fade_curve::cosine);
    auto const fi = conv.fade_info();
    REQUIRE(fi.remaining_blocks == kFade1 && fi.fade_blocks == kFade1 && fi.bank_bytes > 0);
    threw = false;
    try {
        conv.update_impulse(irc.data(), kL);  // a fade is running
    } catch (std::runtime_error const&) {
        threw = true;
    }
    REQUIRE(threw);
    stretch(kAt1, kAt2);
    REQUIRE(conv.fade_info().remaining_blocks == 0 && conv.fade_info().fade_blocks == 0);
    conv.update_impulse(irc.data(), kL, false, kFade2, fade_curve::linear);
    REQUIRE(conv.fade_info().remaining_blocks == kFade2 && conv.fade_info().bank_bytes == fi.bank_bytes);
    stretch(kAt2, kBlocks);
    REQUIRE(conv.fade_info().remaining_blocks == 0);
    return y;
}

static std::vector<float> run_c(int ola, std::vector<float> const& x)
{
    auto const pa = partitions(5100), pb = partitions(5200);
    auto irc = impulse(5300);
    oracle_normalize_impulse(irc.data(), kC, kL);
    neo_hip_upols* h = nullptr;
    REQUIRE((ola ? neo_hip_upola_create : neo_hip_upols_create)(int(kC), int(kB), int(kP), 0, &h) == NEO_HIP_OK);
    std::vector<float> y = x;
    if (!h) return y;
    REQUIRE(neo_hip_upols_set_filter(h, pa.data(), 0) == NEO_HIP_OK);
    auto go = [&](std::size_t b0, std::size_t b1) {
        REQUIRE(neo_hip_upols_process_samples(h, y.data() + b0 * kB, std::int64_t(kN), y.data() + b0 * kB, std::int64_t(kN),
                                              std::int64_t((b1 - b0) * kB), 0, nullptr) == NEO_HIP_OK);
    };
    go(0, kAt1);
    REQUIRE(neo_hip_upols_update_filter(h, pb.data(), 0, kFade1, 1, nullptr) == NEO_HIP_OK);
    go(kAt1, kAt2);
    REQUIRE(neo_hip_upols_update_impulse(h, irc.data(), std::int64_t(kL), 0, 0, kFade2, 0, nullptr) == NEO_HIP_OK);
    go(kAt2, kBlocks);
    int left = -1;
    REQUIRE(neo_hip_upols_fade_info(h, &left, nullptr, nullptr) == NEO_HIP_OK && left == 0);
    neo_hip_upols_destroy(h);
    return y;
}

static void run(method m, char const* path)
{
    std::vector<float> x(kC * kN);
    for (std::size_t c = 0; c < kC; ++c) oracle_noise(5400 + c, x.data() + c * kN, kN);
    neo::convolution::upols_multichannel one(kC, kB, kP, 0, m);
    auto const y = run_cpp(one, x);
    auto const yc = run_c(m == method::upola, x);
    REQUIRE(std::memcmp(y.data(), yc.data(), y.size() * sizeof(float)) == 0);  // the C++ calls are the C ones
    neo::convolution::upols_multidevice two(kC, kB, kP, std::vector<int>{0, 0}, m);
    auto const ym = run_cpp(two, x);
    REQUIRE(std::memcmp(y.data(), ym.data(), y.size() * sizeof(float)) == 0);  // shards change no bit
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

int main(int argc, char** argv)
{
    test_host();
    int n = 0;
    if (neo_hip_device_count(&n) != NEO_HIP_OK || n < 1) {
        std::printf("no GPU: only host-side checks ran\n");
        return failures ? 1 : 0;
    }
    if (argc != 3) {  // upols_fade_main <upols output file> <upola output file> runs the device part
        std::printf("no output files named: only host-side checks ran\n");
        return failures ? 1 : 0;
    }
    run(method::upols, argv[1]);
    run(method::upola, argv[2]);
    std::printf(failures ? "FAILED (%d)\n" : "upols fade C++ tests passed\n", failures);
    return failures ? 1 : 0;
}
