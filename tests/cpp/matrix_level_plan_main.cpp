// csrc/matrix_plan.hpp alone (it includes no HIP header), for a build with the address and
// undefined-behaviour sanitizers: random route lists and window lists through make_matrix_plan and
// make_matrix_level_plan, the level plan checked against a plain restatement (head, bands, splits,
// part cuts, totals, the bytes model), and the walk of k_matrix_lvl_mac (upols_matrix_levels.hip)
// replayed on the host, part by part, for a window in the future with row NUMBERS in place of the
// rows: every (route, partition of the band, block of the window) is multiplied exactly once, by FDL
// row (w + j - p) mod ring of the route's input, which is a block written before the window before
// began and still inside a ring of the plan's size; every row index a load uses is inside the ring
// and the filter; every workgroup belongs to exactly one part.
#include "../../neo-dsp_amd/csrc/matrix_plan.hpp"

#include <cstdio>
#include <random>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

using neo_hip::make_matrix_level_plan;
using neo_hip::make_matrix_plan;
using neo_hip::matrix_level;
using neo_hip::matrix_level_plan;
using neo_hip::matrix_plan;

static int failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return false;                                                 \
        }                                                                 \
    } while (0)

static bool one_case(std::mt19937& rng, int n)
{
    auto pick = [&](int lo, int hi) { return int(std::uniform_int_distribution<int>(lo, hi)(rng)); };
    const int blocks[] = {16, 64, 256, 512, 1024, 4096};
    const int I = pick(1, 6), O = pick(1, 7), B = blocks[pick(0, 5)], P = pick(1, 150);
    const int wgs = pick(0, 3) ? pick(1, 300) : 0;
    std::vector<std::pair<int, int>> all;
    for (int o = 0; o < O; ++o)
        for (int i = 0; i < I; ++i) all.push_back({o, i});
    std::shuffle(all.begin(), all.end(), rng);
    const int R = pick(1, int(all.size()));
    std::vector<int> ro(static_cast<size_t>(R)), ri(static_cast<size_t>(R));
    for (int r = 0; r < R; ++r) ro[size_t(r)] = all[size_t(r)].first, ri[size_t(r)] = all[size_t(r)].second;
    // a window list: a random subset of 2 .. 32 (ascending powers of two are each twice the one before
    // or more), or the default
    std::vector<int> win;
    const bool dflt = pick(0, 4) == 0;
    if (dflt) win = {8, 32};
    else
        while (win.empty())
            for (int T = 2; T <= 32; T *= 2)
                if (pick(0, 1)) win.push_back(T);

    matrix_plan p;
    CHECK(make_matrix_plan(I, O, B, P, ro.data(), ri.data(), R, -1, 0, 0, p) == nullptr);
    matrix_level_plan lp;
    CHECK(make_matrix_level_plan(p, dflt ? nullptr : win.data(), int(win.size()), wgs, lp) == nullptr);
    const int G = B > 256 ? B / 256 : 1;
    CHECK(lp.G == G && lp.O == O && lp.ring == P);

    // head and bands: a restatement
    const int head = std::min(P, 2 * win[0]);
    std::vector<std::tuple<int, int, int>> bands;  // T, a, b
    for (size_t k = 0; k < win.size(); ++k) {
        const int a = 2 * win[k], b = k + 1 < win.size() ? std::min(P, 2 * win[k + 1]) : P;
        if (a < b) bands.push_back({win[k], a, b});
    }
    CHECK(lp.levels.size() == bands.size());
    if (bands.empty()) {
        CHECK(lp.head == P && lp.partial_bytes == 0 && lp.head_bank_bytes == 0);
        CHECK(lp.bytes == 8 * int64_t(B) * (p.filter_loads + p.fdl_loads) + 4 * int64_t(B) * (I + O));
        return true;
    }
    CHECK(lp.head == head && lp.hplan.P == head && !lp.hplan.fused && lp.hplan.nroutes == R);
    CHECK(lp.hplan.rt == p.rt);
    CHECK(lp.head_bank_bytes == int64_t(R) * head * B * 8);
    CHECK(std::get<1>(bands[0]) == head);

    int maxin = 1;
    std::vector<int> nin(size_t(O), 0);
    for (int o = 0; o < O; ++o) {
        for (int i = 0; i < I; ++i) nin[size_t(o)] += p.rt[size_t(o) * I + i] >= 0;
        maxin = std::max(maxin, nin[size_t(o)]);
    }
    int64_t bytes = 8 * int64_t(B) * (int64_t(R) * head + lp.hplan.fdl_loads + 2 * int64_t(O) * lp.hplan.S) +
                    4 * int64_t(B) * (I + O);
    int64_t prows = 0;
    std::vector<int> cover(size_t(R) * P, 0);  // every (route, partition): once over head and levels
    for (int r = 0; r < R; ++r)
        for (int q = 0; q < head; ++q) ++cover[size_t(r) * P + q];
    int prev_T = 0;
    for (size_t l = 0; l < bands.size(); ++l) {
        const matrix_level& lv = lp.levels[l];
        const auto [T, a, b] = bands[l];
        const int D = T < 8 ? T : 8, len = b - a, longest = maxin * len;
        CHECK(lv.T == T && lv.a == a && lv.b == b && T > prev_T && a >= 2 * T && P > 2 * T);
        prev_T = T;
        CHECK(lv.S >= 1 && lv.S <= neo_hip::kMatrixLevelMaxSplits && lv.S <= longest);
        if (!wgs) {
            CHECK(lv.S == 1 || longest / lv.S >= T);  // no split of the longest output shorter than T rows
            CHECK(lv.S == std::max<int64_t>(1, std::min<int64_t>({(int64_t(512) * T + O * G - 1) / (O * G), std::max(1, longest / T), 64})));
        } else {
            CHECK(lv.S == std::max<int64_t>(1, std::min<int64_t>({(int64_t(wgs) * T + O * G - 1) / (O * G), longest, 64})));
        }
        CHECK(lv.nwg == O * lv.S * G && lv.slab_off == prows);
        prows += 2 * int64_t(O) * lv.S * T;
        CHECK(int(lv.run_off.size()) == O * lv.S + 1 && lv.run_off[0] == 0 && lv.run_off.back() == lv.nruns());
        CHECK(lv.runs.size() % 4 == 0 && lv.nruns() <= R + 63 * O);
        // the part cuts: monotone, equal counts to one, every workgroup once
        CHECK(int(lv.part_cut.size()) == T + 1 && lv.part_cut[0] == 0 && lv.part_cut[size_t(T)] == lv.nwg);
        std::vector<int> part_of(size_t(lv.nwg), -1);
        for (int k = 0; k < T; ++k) {
            const int c0 = lv.part_cut[size_t(k)], c1 = lv.part_cut[size_t(k) + 1];
            CHECK(c0 <= c1 && (c1 - c0 == lv.nwg / T || c1 - c0 == lv.nwg / T + 1));
            for (int g = c0; g < c1; ++g) part_of[size_t(g)] = k;
        }
        for (int g = 0; g < lv.nwg; ++g) CHECK(part_of[size_t(g)] >= 0);

        // a window W >= 1 at a random ring position; the parts run during window W - 1, the priming
        // of window W itself at block W T + m reads for the rows j >= m
        const int ring = lp.ring, Wn = pick(1, 9), w = pick(0, ring - 1);
        const int64_t first_block = int64_t(Wn) * T;  // ring row w holds it
        std::set<std::tuple<int, int, int>> met;      // (route, partition, block)
        int64_t fdl_rows = 0;
        // part by part, workgroup by workgroup, as the launches go (the bin chunk repeats the walk)
        for (int k = 0; k < T; ++k)
            for (int g = lv.part_cut[size_t(k)]; g < lv.part_cut[size_t(k) + 1]; ++g) {
                const int os = g / G, chunk = g % G;
                CHECK(os < O * lv.S);
                if (chunk) continue;
                const int o = os / lv.S, s = os % lv.S;
                const int rows = nin[size_t(o)] * len;
                const int r0 = int(int64_t(s) * rows / lv.S), r1 = int(int64_t(s + 1) * rows / lv.S);
                if (rows == longest) CHECK(r1 > r0);
                const int k0 = lv.run_off[size_t(os)], k1 = lv.run_off[size_t(os) + 1];
                CHECK(k0 <= k1 && (r1 > r0) == (k1 > k0));
                int walked = 0, last_in = -1;
                for (int q = k0; q < k1; ++q) {
                    const int i = lv.runs[size_t(4) * q], r = lv.runs[size_t(4) * q + 1];
                    const int pa = lv.runs[size_t(4) * q + 2], pb = lv.runs[size_t(4) * q + 3];
                    CHECK(i > last_in && i < I && r >= 0 && r < R && ro[size_t(r)] == o && ri[size_t(r)] == i);
                    CHECK(r == p.rt[size_t(o) * I + i] && a <= pa && pa < pb && pb <= b);
                    CHECK(q == k0 || pa == a);
                    CHECK(q == k1 - 1 || pb == b);
                    last_in = i;
                    walked += pb - pa;
                    fdl_rows += pb - pa + T - 1;
                    std::vector<int> f(size_t(T), -1), pf(size_t(D), -1), ph(size_t(D), -1);
                    auto frow = [&](int pp) { return w - pp < 0 ? w - pp + ring : w - pp; };
                    for (int sl = 1; sl < T; ++sl) {
                        int row = w + sl - pa;
                        row = row < 0 ? row + ring : (row >= ring ? row - ring : row);
                        CHECK(row >= 0 && row < ring);
                        f[size_t(sl)] = row;
                    }
                    for (int d = 0; d < D; ++d) {
                        const int pp = std::min(pa + d, P - 1);
                        CHECK(frow(pp) >= 0 && frow(pp) < ring);
                        pf[size_t(d)] = frow(pp), ph[size_t(d)] = pp;
                    }
                    for (int p0 = pa; p0 < pb; p0 += T)
                        for (int U = 0; U < T; ++U) {
                            const int pp = p0 + U, slot = U % D;
                            f[size_t((T - U) % T)] = pf[size_t(slot)];
                            const int hrow = ph[size_t(slot)];
                            const int pn = std::min(pp + D, P - 1);
                            CHECK(pn >= 0 && pn < P && frow(pn) >= 0 && frow(pn) < ring);
                            pf[size_t(slot)] = frow(pn), ph[size_t(slot)] = pn;
                            if (pp >= pb) continue;  // the skipped steps
                            CHECK(hrow == pp);
                            for (int j = 0; j < T; ++j) {
                                const int want = ((w + j - pp) % ring + ring) % ring;
                                CHECK(f[size_t((j - U + T) % T)] == want);
                                CHECK(met.insert({r, pp, j}).second);
                                // the block that row holds: written before window W - 1 began ...
                                const int64_t blk = first_block + j - pp;
                                CHECK(blk < first_block - T);
                                // ... and, run in its turn at block (W - 1) T + k, still in the ring
                                CHECK(blk > first_block - T + k - ring);
                                // priming window W itself at block W T + m, m <= j: still in the ring
                                CHECK(blk > first_block + j - ring);
                            }
                        }
                    CHECK(part_of[size_t(g)] == k);
                    for (int pp = pa; pp < pb; ++pp) ++cover[size_t(r) * P + pp];
                }
                CHECK(walked == r1 - r0);
            }
        CHECK(int64_t(met.size()) == int64_t(R) * len * T);
        CHECK(fdl_rows == lv.fdl_rows && lv.filter_rows == int64_t(R) * len);
        bytes += 8 * int64_t(B) * (lv.filter_rows + lv.fdl_rows) / T + 8 * int64_t(B) * 2 * O * lv.S;
    }
    for (int c : cover) CHECK(c == 1);
    CHECK(lp.partial_rows == prows && lp.partial_bytes == prows * B * 8);
    CHECK(lp.bytes == bytes);

    if (n % 10 == 0) {  // refusals
        matrix_level_plan q;
        const int bad[][3] = {{3, 0, 0}, {1, 0, 0}, {64, 0, 0}, {4, 4, 0}, {8, 4, 0}, {4, 6, 0}, {0, 0, 0}};
        CHECK(make_matrix_level_plan(p, bad[0], 1, 0, q) != nullptr);
        CHECK(make_matrix_level_plan(p, bad[1], 1, 0, q) != nullptr);
        CHECK(make_matrix_level_plan(p, bad[2], 1, 0, q) != nullptr);
        CHECK(make_matrix_level_plan(p, bad[3], 2, 0, q) != nullptr);
        CHECK(make_matrix_level_plan(p, bad[4], 2, 0, q) != nullptr);
        CHECK(make_matrix_level_plan(p, bad[5], 2, 0, q) != nullptr);
        CHECK(make_matrix_level_plan(p, bad[6], 1, 0, q) != nullptr);
        CHECK(make_matrix_level_plan(p, win.data(), 0, 0, q) != nullptr);
        CHECK(make_matrix_level_plan(p, win.data(), 6, 0, q) != nullptr);
        CHECK(make_matrix_level_plan(p, win.data(), int(win.size()), -1, q) != nullptr);
    }
    return true;
}

int main()
{
    std::mt19937 rng(20241020);
    const int cases = 300;
    for (int n = 0; n < cases; ++n)
        if (!one_case(rng, n)) ++failed;
    std::printf("%d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
