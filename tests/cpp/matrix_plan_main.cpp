// csrc/matrix_plan.hpp alone (it includes no HIP header), for a build with the address and
// undefined-behaviour sanitizers: random route lists through make_matrix_plan, checked against a
// plain restatement, and the row walk of k_matrix_step (upols_matrix.hip) replayed on the host for
// every (tile, split): every (route, partition) is met exactly once, every index stays in range,
// and the loads add up to the plan's totals. The two device tables the handle uploads
// (matrix_tile_table, matrix_route_table) are checked against the plan and the caller's list.
#include "../../neo-dsp_amd/csrc/matrix_plan.hpp"

#include <cstdio>
#include <random>
#include <set>
#include <utility>
#include <vector>

using neo_hip::make_matrix_plan;
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
    const int blocks[] = {16, 64, 512, 1024, 4096};
    const int I = pick(1, 9), O = pick(1, 11), B = blocks[pick(0, 4)], P = pick(1, 40);
    const int tiles_opt[] = {0, 1, 2, 4};
    const int ot = tiles_opt[pick(0, 3)], fused = pick(-1, 1), wgs = pick(0, 3) ? pick(1, 300) : 0;
    // a random subset of the pairs, in random order
    std::vector<std::pair<int, int>> all;
    for (int o = 0; o < O; ++o)
        for (int i = 0; i < I; ++i) all.push_back({o, i});
    std::shuffle(all.begin(), all.end(), rng);
    const int R = pick(1, int(all.size()));
    std::vector<int> ro(static_cast<size_t>(R)), ri(static_cast<size_t>(R));
    for (int r = 0; r < R; ++r) ro[size_t(r)] = all[size_t(r)].first, ri[size_t(r)] = all[size_t(r)].second;

    matrix_plan p;
    CHECK(make_matrix_plan(I, O, B, P, ro.data(), ri.data(), R, fused, wgs, ot, p) == nullptr);
    const int cap = neo_hip::matrix_max_tile(B);
    if (ot) CHECK(p.OT == std::min(ot, cap));
    else CHECK(p.OT == 1 || (p.OT == 4 && B == neo_hip::kMatrixAutoTileBlock));
    CHECK(p.ntiles == (O + p.OT - 1) / p.OT);
    CHECK(p.S >= 1 && p.S <= neo_hip::kMatrixMaxSplits);
    CHECK(int(p.rt.size()) == I * O && int(p.uni_off.size()) == p.ntiles + 1);
    CHECK(p.filter_loads == int64_t(R) * P);
    if (fused >= 0) CHECK(p.fused == (fused != 0));

    // the walk of k_matrix_step, workgroup (t, s)
    std::set<std::pair<int, int>> met;  // (route, partition)
    int64_t fdl = 0, filt = 0;
    bool nonempty_longest = false;
    int longest = 0;
    for (int t = 0; t < p.ntiles; ++t) longest = std::max(longest, p.rows(t));
    for (int t = 0; t < p.ntiles; ++t) {
        const int first = p.tile_first[size_t(t)], count = p.tile_count[size_t(t)];
        CHECK(first == t * p.OT && count >= 1 && count <= p.OT && first + count <= O);
        const int nuni = p.uni_off[size_t(t) + 1] - p.uni_off[size_t(t)];
        const int* uni = p.uni.data() + p.uni_off[size_t(t)];
        for (int k = 0; k < nuni; ++k) {
            CHECK(uni[k] >= 0 && uni[k] < I && (k == 0 || uni[k] > uni[k - 1]));
            bool any = false;
            for (int o = first; o < first + count; ++o) any = any || p.rt[size_t(o) * I + uni[k]] >= 0;
            CHECK(any);
        }
        const int nrows = nuni * P, per = (nrows + p.S - 1) / p.S;
        CHECK(nrows == p.rows(t));
        int covered = 0;
        for (int s = 0; s < p.S; ++s) {
            const int r0 = std::min(nrows, s * per), r1 = std::min(nrows, r0 + per);
            CHECK(r0 == p.cut(t, s) && r1 == p.cut(t, s + 1) && r0 == covered);
            covered = r1;
            if (nrows == longest && longest > 0) nonempty_longest = nonempty_longest || r1 > r0;
            if (nrows == longest && longest > 0) CHECK(r1 > r0);
            for (int seg = r1 > r0 ? r0 / P : nuni; seg < nuni && seg * P < r1; ++seg) {
                const int i = uni[seg];
                const int pbeg = std::max(r0, seg * P) - seg * P, pend = std::min(r1, (seg + 1) * P) - seg * P;
                CHECK(pbeg >= 0 && pbeg < pend && pend <= P);
                for (int pp = pbeg; pp < pend; ++pp) {
                    ++fdl;
                    for (int o = 0; o < p.OT; ++o) {
                        const int r = o < count ? p.rt[size_t(first + o) * I + i] : -1;
                        if (r < 0) continue;
                        CHECK(r < R && ro[size_t(r)] == first + o && ri[size_t(r)] == i);
                        CHECK(met.insert({r, pp}).second);
                        ++filt;
                    }
                }
            }
        }
        CHECK(covered == nrows && p.cut(t, p.S) == nrows);
    }
    CHECK(fdl == p.fdl_loads && filt == p.filter_loads && int64_t(met.size()) == int64_t(R) * P);
    (void)nonempty_longest;

    // the device tables. The tile table, read as k_matrix_step reads it, reproduces the plan
    const std::vector<int> tt = neo_hip::matrix_tile_table(p);
    CHECK(tt.size() == size_t(4) * p.ntiles + p.uni.size() + p.rt.size());
    for (int t = 0; t < p.ntiles; ++t) {
        const int nuni = tt[size_t(4) * t + 2];
        CHECK(tt[size_t(4) * t] == p.tile_first[size_t(t)] && tt[size_t(4) * t + 1] == p.tile_count[size_t(t)]);
        CHECK(nuni == p.uni_off[size_t(t) + 1] - p.uni_off[size_t(t)] && tt[size_t(4) * t + 3] == p.uni_off[size_t(t)]);
        for (int k = 0; k < nuni; ++k)
            CHECK(tt[size_t(4) * p.ntiles + tt[size_t(4) * t + 3] + k] == p.uni[size_t(p.uni_off[size_t(t)]) + k]);
    }
    const size_t rt0 = size_t(4) * p.ntiles + tt[size_t(4) * (p.ntiles - 1) + 3] + tt[size_t(4) * (p.ntiles - 1) + 2];
    CHECK(rt0 + p.rt.size() == tt.size());
    for (size_t k = 0; k < p.rt.size(); ++k) CHECK(tt[rt0 + k] == p.rt[k]);
    // the route table: per output exactly its routes (each route of the caller's list once, under
    // its own output, with its own input and index), inputs strictly ascending, offsets up to R
    const std::vector<int> rtab = neo_hip::matrix_route_table(p);
    CHECK(rtab.size() == size_t(O) + 1 + size_t(2) * R && rtab[0] == 0 && rtab[size_t(O)] == R);
    std::vector<bool> seen(size_t(R), false);
    for (int o = 0; o < O; ++o) {
        CHECK(rtab[size_t(o)] <= rtab[size_t(o) + 1]);
        for (int e = rtab[size_t(o)]; e < rtab[size_t(o) + 1]; ++e) {
            const int i = rtab[size_t(O) + 1 + size_t(2) * e], r = rtab[size_t(O) + 2 + size_t(2) * e];
            CHECK(r >= 0 && r < R && ro[size_t(r)] == o && ri[size_t(r)] == i && !seen[size_t(r)]);
            seen[size_t(r)] = true;
            CHECK(e == rtab[size_t(o)] || i > rtab[size_t(O) + 1 + size_t(2) * (e - 1)]);
        }
    }

    // refusals leave no plan behind that could be used: the reasons
    if (n % 10 == 0) {
        matrix_plan q;
        std::vector<int> o2 = ro, i2 = ri;
        o2.push_back(ro[0]), i2.push_back(ri[0]);
        CHECK(make_matrix_plan(I, O, B, P, o2.data(), i2.data(), R + 1, fused, wgs, ot, q) != nullptr);  // duplicate
        o2.back() = O;
        CHECK(make_matrix_plan(I, O, B, P, o2.data(), i2.data(), R + 1, fused, wgs, ot, q) != nullptr);  // out of range
        CHECK(make_matrix_plan(I, O, B, P, ro.data(), ri.data(), 0, fused, wgs, ot, q) != nullptr);
        CHECK(make_matrix_plan(I, O, B + 1, P, ro.data(), ri.data(), R, fused, wgs, ot, q) != nullptr);
        CHECK(make_matrix_plan(I, O, B, P, ro.data(), ri.data(), R, fused, wgs, 3, q) != nullptr);
        CHECK(make_matrix_plan(I, O, B, P, nullptr, ri.data(), R, fused, wgs, ot, q) != nullptr);
    }
    return true;
}

int main()
{
    std::mt19937 rng(20240607);
    const int cases = 300;
    for (int n = 0; n < cases; ++n)
        if (!one_case(rng, n)) ++failed;
    std::printf("%d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
