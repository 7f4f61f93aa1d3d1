// Stand-alone host program for neo-dsp_amd/csrc/sparse_plan.hpp (no GPU, no HIP header): the
// plan of a set of masks against a per-tile restatement of the format, with guard words around
// every output so that a write past an array shows (build with -fsanitize=address,undefined).
// Exit status 0 = every case agrees.
#include "../../neo-dsp_amd/csrc/sparse_plan.hpp"

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

using mask_fn = std::function<bool(int c, int p, int k)>;

static std::uint64_t mix(std::uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static bool bernoulli(double prob, int c, int p, int k)
{
    auto const z = mix((std::uint64_t(c) << 40) ^ (std::uint64_t(p) << 20) ^ std::uint64_t(k));
    return double(z >> 11) * (1.0 / 9007199254740992.0) < prob;
}

static int run(std::string const& name, int C, int B, int P, mask_fn const& f)
{
    int const NW = B / 512 > 1 ? B / 512 : 1, NT = B / 16;
    std::vector<std::uint8_t> mask(std::size_t(C) * P * (B + 1));
    for (int c = 0; c < C; ++c)
        for (int p = 0; p < P; ++p)
            for (int k = 0; k <= B; ++k) mask[(std::size_t(c) * P + p) * (B + 1) + k] = f(c, p, k) ? 1 : 0;
    constexpr std::uint32_t guard = 0xDEADBEEFu;
    std::vector<std::uint32_t> bits(std::size_t(C) * P * NW + 2, guard), off(std::size_t(C) * (P + 1) + 2, guard);
    std::int64_t bins = -1, tiles = -1;
    if (!neo_hip::sparse_plan(mask.data(), C, B, P, bits.data() + 1, off.data() + 1, &bins, &tiles)) {
        std::printf("FAIL %s: plan refused\n", name.c_str());
        return 1;
    }
    int bad = 0;
    if (bits.front() != guard || bits.back() != guard || off.front() != guard || off.back() != guard) ++bad;
    std::int64_t want_bins = 0, want_tiles = 0;
    for (int c = 0; c < C; ++c) {
        std::uint32_t run = 0;
        for (int p = 0; p < P; ++p) {
            auto const* m = &mask[(std::size_t(c) * P + p) * (B + 1)];
            if (off[1 + std::size_t(c) * (P + 1) + p] != run) ++bad;
            for (int t = 0; t < NT; ++t) {
                bool keep = false;
                for (int j = 0; j < 16; ++j) keep = keep || m[t * 16 + j];
                if (t == 0) keep = keep || m[B];
                bool const got = (bits[1 + (std::size_t(c) * P + p) * NW + t / 32] >> (t % 32)) & 1u;
                if (got != keep) ++bad;
                run += keep;
            }
            for (int t = NT; t < 32 * NW; ++t)  // no bit past the row's tiles
                if ((bits[1 + (std::size_t(c) * P + p) * NW + t / 32] >> (t % 32)) & 1u) ++bad;
            for (int k = 0; k <= B; ++k) want_bins += m[k];
        }
        if (off[1 + std::size_t(c) * (P + 1) + P] != run) ++bad;
        want_tiles += run;
    }
    if (bins != want_bins || tiles != want_tiles) ++bad;
    if (bad) std::printf("FAIL %s: C %d B %d P %d: %d mismatches\n", name.c_str(), C, B, P, bad);
    return bad ? 1 : 0;
}

int main()
{
    int failed = 0, cases = 0;
    int const P = 5;
    for (int B : {16, 32, 512, 1024, 4096}) {
        for (int C : {1, 2}) {
            std::vector<std::pair<std::string, mask_fn>> const masks = {
                {"all-true", [](int, int, int) { return true; }},
                {"all-false", [](int, int, int) { return false; }},
                {"dc-only", [](int, int, int k) { return k == 0; }},
                {"nyquist-only", [B](int, int, int k) { return k == B; }},
                {"dc-dropped-nyquist-kept", [B](int, int, int k) { return k == B || (k > 0 && k % 5 == 0); }},
                {"one-column-per-tile", [](int, int p, int k) { return k % 16 == (3 + p) % 16; }},
                {"bernoulli-0.5", [](int c, int p, int k) { return bernoulli(0.5, c, p, k); }},
                {"bernoulli-0.01", [](int c, int p, int k) { return bernoulli(0.01, c, p, k); }},
                {"empty-row-middle", [](int c, int p, int k) { return p != 2 && bernoulli(0.3, c, p, k); }},
                {"empty-row-end", [](int c, int p, int k) { return p != 4 && bernoulli(0.3, c, p, k); }},
            };
            for (auto const& [name, f] : masks) {
                failed += run(name, C, B, P, f);
                ++cases;
            }
        }
    }
    // refused arguments write nothing
    std::uint8_t m[17] = {};
    std::uint32_t w[1] = {7}, o[2] = {7, 7};
    if (neo_hip::sparse_plan(m, 1, 500, 1, w, o, nullptr, nullptr) || neo_hip::sparse_plan(m, 0, 16, 1, w, o, nullptr, nullptr) ||
        neo_hip::sparse_plan(nullptr, 1, 16, 1, w, o, nullptr, nullptr) || w[0] != 7 || o[0] != 7 || o[1] != 7)
        ++failed;
    if (!neo_hip::sparse_plan(m, 1, 16, 1, w, o, nullptr, nullptr) || w[0] != 0 || o[0] != 0 || o[1] != 0) ++failed;
    std::printf("%d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
