// Stand-alone host program for sparse_window_plan in neo-dsp_amd/csrc/sparse_plan.hpp (no GPU, no
// HIP header): the window bitmaps of a set of masks against a per-tile restatement (tile t of
// win[c][p] set iff some row q in [p, min(P, p + window)) keeps tile t), with guard words around
// the output so that a write past it shows (build with -fsanitize=address,undefined).
// Exit status 0 = every case agrees.
#include "../../neo-dsp_amd/csrc/sparse_plan.hpp"

#include <cstdio>
#include <vector>

static std::uint64_t mix(std::uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// mask family f of (c, p, k): 0 all-true, 1 all-false, 2 bernoulli 0.3, 3 bernoulli 0.01,
// 4 only the last row's last column below B, 5 only row 0
static bool keep(int f, int c, int p, int k, int B, int P)
{
    auto const z = mix((std::uint64_t(c) << 40) ^ (std::uint64_t(p) << 20) ^ std::uint64_t(k));
    double const u = double(z >> 11) * (1.0 / 9007199254740992.0);
    switch (f) {
        case 0: return true;
        case 1: return false;
        case 2: return u < 0.3;
        case 3: return u < 0.01;
        case 4: return p == P - 1 && k == B - 1;
        default: return p == 0;
    }
}

static int run(int f, int C, int B, int P, int W)
{
    int const NW = neo_hip::sparse_words(B), NT = B / 16;
    std::vector<std::uint8_t> mask(std::size_t(C) * P * (B + 1));
    for (int c = 0; c < C; ++c)
        for (int p = 0; p < P; ++p)
            for (int k = 0; k <= B; ++k) mask[(std::size_t(c) * P + p) * (B + 1) + k] = keep(f, c, p, k, B, P) ? 1 : 0;
    std::vector<std::uint32_t> bits(std::size_t(C) * P * NW), off(std::size_t(C) * (P + 1));
    if (!neo_hip::sparse_plan(mask.data(), C, B, P, bits.data(), off.data(), nullptr, nullptr)) return 1;
    constexpr std::uint32_t guard = 0xDEADBEEFu;
    std::vector<std::uint32_t> win(std::size_t(C) * P * NW + 2, guard);
    std::int64_t tiles = -1;
    if (!neo_hip::sparse_window_plan(bits.data(), C, B, P, W, win.data() + 1, &tiles)) {
        std::printf("FAIL family %d: plan refused\n", f);
        return 1;
    }
    int bad = 0;
    if (win.front() != guard || win.back() != guard) ++bad;
    std::int64_t want = 0;
    for (int c = 0; c < C; ++c)
        for (int p = 0; p < P; ++p)
            for (int t = 0; t < 32 * NW; ++t) {
                bool any = false;
                for (int q = p; q < P && q < p + W; ++q)
                    any = any || ((bits[(std::size_t(c) * P + q) * NW + t / 32] >> (t % 32)) & 1u);
                if (t >= NT && any) ++bad;  // no bit past the row's tiles
                bool const got = (win[1 + (std::size_t(c) * P + p) * NW + t / 32] >> (t % 32)) & 1u;
                if (got != any) ++bad;
                want += any;
            }
    if (tiles != want) ++bad;
    if (bad) std::printf("FAIL family %d: C %d B %d P %d W %d: %d mismatches\n", f, C, B, P, W, bad);
    return bad ? 1 : 0;
}

int main()
{
    int failed = 0, cases = 0;
    for (int B : {16, 512, 1024, 4096})
        for (int W : {2, 16, 32})
            for (int P : {W - 1, W, 2 * W + 5})
                for (int f = 0; f < 6; ++f) {
                    failed += run(f, f == 2 ? 2 : 1, B, P, W);
                    ++cases;
                }
    // refused arguments write nothing
    std::uint32_t b[2] = {1, 2}, w[2] = {7, 7};
    std::int64_t t = -5;
    for (int W : {0, 1, 3, 64, -2})
        if (neo_hip::sparse_window_plan(b, 1, 16, 2, W, w, &t)) ++failed;
    if (neo_hip::sparse_window_plan(nullptr, 1, 16, 2, 2, w, &t) || neo_hip::sparse_window_plan(b, 1, 16, 2, 2, nullptr, &t) ||
        neo_hip::sparse_window_plan(b, 0, 16, 2, 2, w, &t) || neo_hip::sparse_window_plan(b, 1, 16, 0, 2, w, &t) ||
        neo_hip::sparse_window_plan(b, 1, 500, 2, 2, w, &t) || w[0] != 7 || w[1] != 7 || t != -5)
        ++failed;
    if (!neo_hip::sparse_window_plan(b, 1, 16, 2, 2, w, nullptr) || w[0] != 3 || w[1] != 2) ++failed;
    std::printf("%d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
