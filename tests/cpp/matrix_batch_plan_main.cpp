// csrc/matrix_plan.hpp alone (it includes no HIP header), for a build with the address and
// undefined-behaviour sanitizers: random route lists through make_matrix_plan and
// make_matrix_batch_plan, the batch plan checked against a plain restatement, and the walk of
// k_matrix_batch_mac (upols_matrix_batch.hip) replayed on the host for every (output, split) with row
// NUMBERS in place of the rows: the window slots, the prefetch ring and the clamped loads. Every
// (route, partition, block) is multiplied exactly once, by FDL row (w + j - p) mod ring of the
// route's input, every row index a load uses is inside the ring and the filter, and the loads add
// up to the plan's totals.
#include "../../neo-dsp_amd/csrc/matrix_plan.hpp"

#include <cstdio>
#include <random>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

using neo_hip::make_matrix_batch_plan;
using neo_hip::make_matrix_plan;
using neo_hip::matrix_batch_plan;
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
    const int I = pick(1, 7), O = pick(1, 9), B = blocks[pick(0, 5)], P = pick(1, 75);
    const int T = 2 << pick(0, 4), D = T < 8 ? T : 8;
    const int wgs = pick(0, 3) ? pick(1, 600) : 0;
    std::vector<std::pair<int, int>> all;
    for (int o = 0; o < O; ++o)
        for (int i = 0; i < I; ++i) all.push_back({o, i});
    std::shuffle(all.begin(), all.end(), rng);
    const int R = pick(1, int(all.size()));
    std::vector<int> ro(static_cast<size_t>(R)), ri(static_cast<size_t>(R));
    for (int r = 0; r < R; ++r) ro[size_t(r)] = all[size_t(r)].first, ri[size_t(r)] = all[size_t(r)].second;

    matrix_plan p;
    CHECK(make_matrix_plan(I, O, B, P, ro.data(), ri.data(), R, -1, 0, 0, p) == nullptr);
    matrix_batch_plan bp;
    CHECK(make_matrix_batch_plan(p, T, wgs, bp) == nullptr);
    CHECK(bp.T == T && bp.O == O && bp.G == (B > 256 ? B / 256 : 1));
    CHECK(bp.Sb >= 1 && bp.Sb <= neo_hip::kMatrixMaxSplits);
    CHECK(int(bp.run_off.size()) == O * bp.Sb + 1 && bp.run_off[0] == 0 && bp.run_off.back() == bp.nruns());
    CHECK(bp.runs.size() % 4 == 0 && bp.nruns() <= R + 63 * O);

    // the splits: equal row counts, none empty in the longest output, the automatic rule
    int longest = 1;
    for (int o = 0; o < O; ++o) {
        int nin = 0;
        for (int i = 0; i < I; ++i) nin += p.rt[size_t(o) * I + i] >= 0;
        CHECK(bp.rows[size_t(o)] == nin * P);
        longest = std::max(longest, nin * P);
    }
    CHECK(bp.Sb <= longest);
    if (!wgs) CHECK(bp.Sb == 1 || longest / bp.Sb >= neo_hip::kMatrixBatch);
    else CHECK(bp.Sb == std::max(1, std::min({(wgs + O * bp.G - 1) / (O * bp.G), longest, neo_hip::kMatrixMaxSplits})));

    const int ring = P + neo_hip::kMatrixBatch - 1, w = pick(0, ring - 1);
    std::set<std::tuple<int, int, int>> met;  // (route, partition, block)
    int64_t fdl_rows = 0;
    for (int o = 0; o < O; ++o) {
        const int rows = bp.rows[size_t(o)];
        int covered = 0;
        for (int s = 0; s < bp.Sb; ++s) {
            const int r0 = bp.cut(o, s), r1 = bp.cut(o, s + 1);
            CHECK(r0 == covered && r1 >= r0 && r1 - r0 <= rows / bp.Sb + 1 && r1 - r0 >= rows / bp.Sb);
            if (rows == longest) CHECK(r1 > r0);
            covered = r1;
            const int k0 = bp.run_off[size_t(o) * bp.Sb + s], k1 = bp.run_off[size_t(o) * bp.Sb + s + 1];
            CHECK(k0 <= k1 && (r1 > r0) == (k1 > k0));
            int walked = 0, last_in = -1;
            for (int k = k0; k < k1; ++k) {
                const int i = bp.runs[size_t(4) * k], r = bp.runs[size_t(4) * k + 1];
                const int pa = bp.runs[size_t(4) * k + 2], pb = bp.runs[size_t(4) * k + 3];
                CHECK(i > last_in && i < I && r >= 0 && r < R && ro[size_t(r)] == o && ri[size_t(r)] == i);
                CHECK(r == p.rt[size_t(o) * I + i] && 0 <= pa && pa < pb && pb <= P);
                CHECK(k == k0 || pa == 0);       // only a split's first run starts inside an input
                CHECK(k == k1 - 1 || pb == P);   // only its last one ends inside one
                last_in = i;
                walked += pb - pa;
                fdl_rows += pb - pa + T - 1;
                // the kernel's walk of this run with row numbers: window slots f, prefetch slots pf (FDL
                // row) and ph (filter row)
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
                        }
                    }
            }
            CHECK(walked == r1 - r0);
        }
        CHECK(covered == rows);
    }
    CHECK(int64_t(met.size()) == int64_t(R) * P * T);
    CHECK(fdl_rows == bp.fdl_rows && bp.filter_rows == int64_t(R) * P && bp.slab_rows == int64_t(O) * bp.Sb * T);
    CHECK(bp.bytes == 8 * int64_t(B) * (bp.filter_rows + bp.fdl_rows + 2 * bp.slab_rows) + 4 * int64_t(B) * T * (I + O));

    if (n % 10 == 0) {  // refusals
        matrix_batch_plan q;
        CHECK(make_matrix_batch_plan(p, 1, wgs, q) != nullptr);
        CHECK(make_matrix_batch_plan(p, 3, wgs, q) != nullptr);
        CHECK(make_matrix_batch_plan(p, 64, wgs, q) != nullptr);
        CHECK(make_matrix_batch_plan(p, T, -1, q) != nullptr);
    }
    return true;
}

int main()
{
    std::mt19937 rng(20240911);
    const int cases = 300;
    for (int n = 0; n < cases; ++n)
        if (!one_case(rng, n)) ++failed;
    std::printf("%d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
