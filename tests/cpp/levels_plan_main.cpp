// csrc/levels_plan.hpp alone (it includes no HIP header), for a build with the address and
// undefined-behaviour sanitizers: the real schedule of the dense convolver's streaming levels
// (make_level_sched, plan_parts, prime_round, block_rows, block_levels, slice_part) walked over
// 2 P + 3 * 128 + 60 blocks per configuration -- history by plain steps, a prime, streaming steps,
// plain steps in mid-stream off the group grid, a second prime -- with block NUMBERS in place of
// the blocks. No numerics. Block t lives in ring row t mod ring. Checked for every launch:
//   reads     every FDL row a role reads is a block before its launch's guarantee and is not
//             overwritten by a block that may run beside the launch
//   coverage  at the first block of every window (and at the first block after a prime) every unit
//             of every level and class holds that window, computed exactly once by a launch the
//             block is ordered after; the far level by phase 1, 2a and 2b (2c; the recomputed form)
//             in that order, every segment of the window exactly once, from slots that hold the
//             row pair the segment needs
//   buffers   a role overwrites a slab or far-field buffer only when every block of the window it
//             held is complete; the block role's selectors (per class for staggered levels, by the
//             kernel's own formula) name the buffer and row the covering role wrote
//   shape     nwg of every role is what its units need; a launch's far roles do not overlap
// --mutate band | early | cut: a staggered band (and a far band at 128 + 4 G) one partition
// earlier; the even groups' classes own their windows one group sooner; one part's last unit
// dropped. Each must fail. Exit status 1 if any case failed.
#include "../../neo-dsp_amd/csrc/levels_plan.hpp"

#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

using namespace neo_hip;

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            if (verbose) std::printf("FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, what.c_str()); \
            return false;                                                                 \
        }                                                                                 \
    } while (0)

static bool verbose = true;
enum mutation { kMutNone, kMutBand, kMutEarly, kMutCut };
constexpr int64_t kNever = INT64_MIN / 2;

// what a launch may rely on
struct launch_ctx {
    int64_t limit;  // the blocks before `limit` are written
    int64_t lo, hi; // the blocks [lo, hi) may run beside the launch
    int64_t ready;  // the first block ordered after the launch
    bool prime;     // a prime launch (window 0 of a class)
    bool even_bg;   // the background launch of an even group
};

struct world {
    level_sched s;
    int mut = kMutNone;
    std::string what;
    int64_t t = 0, t0 = 0, n = -1, seq = 0;
    bool cut_done = false;
    struct cell {
        int64_t start = kNever, ready = 0;
        bool primed = false;  // by a prime launch: window 1 of a level with an offset, whose parts then run again
    };
    struct acc_cell {
        int64_t win = kNever, seq = 0;
        int first = 0;
    };
    struct xf_cell {
        int64_t r0 = kNever, seq = 0;
    };
    std::vector<cell> slab[kLvToep][2], ff[2];
    std::vector<acc_cell> acc[kFarKMax];
    std::vector<std::vector<xf_cell>> xf;
    struct cur_win {
        int64_t start = kNever;
        int buf = 0;
    };
    std::vector<cur_win> cur[kLvToep + 1];  // per level and class; [kLvToep]: the far level

    int ring_row(int64_t blk) const { return int(pmod<int64_t>(blk, s.ring)); }
    // the block nearest to `now` that lives in ring row r
    int64_t block_of(int r, int64_t now) const
    {
        int64_t d = pmod<int64_t>(r - now, s.ring);
        if (d > s.ring / 2) d -= s.ring;
        return now + d;
    }
    static int upw(int T) { return T <= 8 ? 16 : (T <= 32 ? 32 / T : 1); }
    int jh(int T) const { return T == 128 ? 8 : (T == 32 ? (s.toep_jh ? s.toep_jh : (s.C * (s.B / 16) < 256 ? 2 : 1)) : 1); }
    int far_class(int u) const
    {
        if (!s.lv.stag) return 0;
        const int c = u / (s.B / 16);
        int k = 0;
        while (s.st_fcut[size_t(k) + 1] <= c) ++k;
        return k;
    }
    int64_t far_start(int64_t W, int u) const
    {
        return t0 + W * kFarT - (s.lv.stag ? stag_phi(kFarT, s.lv.stag, far_class(u)) : 0);
    }
    static int far_first(int c, int K) { return 1 + pmod(c - 1, K); }

    bool reads(int64_t newest, int64_t oldest, const launch_ctx& c)
    {
        CHECK(newest < c.limit);
        CHECK(oldest + s.ring >= c.hi);  // block oldest + ring, which takes its row, cannot have run yet
        return true;
    }

    void reset()
    {
        const level_plan& lp = s.lv;
        for (int l = 0; l < lp.n; ++l) {
            const size_t U = size_t(s.C) * size_t(s.B / 16) * size_t(jh(lp.T[l]));
            for (auto& b : slab[l]) b.assign(U, cell{});
            cur[l].assign(stag_level(lp, l) ? size_t(lp.T[l] / lp.stag) : 1, cur_win{});
        }
        const size_t FU = size_t(far_units(s));
        for (auto& b : ff) b.assign(FU, cell{});
        for (auto& a : acc) a.assign(FU, acc_cell{});
        xf.assign(size_t(std::max(1, lp.nseg)), std::vector<xf_cell>(FU));
        cur[kLvToep].assign(lp.stag && lp.nseg ? size_t(kFarT / lp.stag) : 1, cur_win{});
    }

    // -- roles ---------------------------------------------------------------------------
    bool toep(const slice_args& a, const level_sel& sel, int l, const launch_ctx& c)
    {
        const level_plan& lp = s.lv;
        toep_arg ta = a.tp[l];
        if (ta.u1 <= ta.u0) {
            CHECK(ta.nwg == 0);
            return true;
        }
        const int T = lp.T[l];
        CHECK(ta.T == T && ta.a == lp.a[l] && ta.b == lp.b[l] && ta.jh == jh(T) && ta.cs == slab_cs(T, s.B));
        if (mut == kMutCut && !cut_done && !c.prime && n > 40) {
            --ta.u1;  // the part's last unit dropped (nwg left as it is)
            cut_done = true;
        } else {
            CHECK(ta.nwg == (ta.u1 - ta.u0 + upw(T) - 1) / upw(T));
        }
        CHECK(ta.u0 >= 0 && size_t(ta.u1) <= slab[l][0].size());
        int buf = sel.tp[l];
        CHECK(buf == 0 || buf == 1);
        int64_t S = block_of(ta.tw, c.prime ? t0 : c.ready);
        if (mut == kMutEarly && stag_level(lp, l)) {
            // the even classes own their windows one group sooner: they start where (n + phi2) mod T = 0
            const int G = lp.stag, upc = (s.B / 16) * jh(T);
            int k = 0;
            while (s.st_cut[l][size_t(k)] * upc != ta.u0 || s.st_cut[l][size_t(k) + 1] * upc != ta.u1) ++k;
            if (k % 2 == 0) {
                const int phi2 = (stag_phi(T, G, k) + G) & (T - 1);
                S = c.prime ? t0 - phi2 : S - G;
                buf = int(((S - t0 + phi2) / T) & 1);
            }
        }
        // rows S + j - p, j < T, p in [a, b)
        if (!reads(S + T - 1 - ta.a, S - (ta.b - 1), c)) return false;
        for (int u = ta.u0; u < ta.u1; ++u) {
            cell& x = slab[l][buf][size_t(u)];
            CHECK(x.start != S || x.primed);                                  // computed once
            CHECK(x.start == kNever || x.start == S || x.start + T <= c.lo);  // the window it held is over
            x = cell{S, c.ready, c.prime};
        }
        return true;
    }

    bool far2a(const slice_args& a, int u0, int u1, int64_t S, int64_t W, const launch_ctx& c)
    {
        const int ns = s.lv.nseg, nf = std::min(a.fnfresh, ns);
        for (int sg = 0; sg < nf; ++sg) {
            const int64_t r0 = S - a.fA - (sg + 1) * int64_t(kFarT);
            CHECK(r0 + kFN - 1 < c.limit);
            const int64_t need = std::max(r0, S - s.P + 1);  // older rows meet the zero padding past P
            if (need <= r0 + kFN - 1) CHECK(need + s.ring >= c.hi);
            for (int u = u0; u < u1; ++u) xf[size_t(pmod<int64_t>(W - sg - 1, a.M))][size_t(u)] = xf_cell{r0, seq};
        }
        return true;
    }

    bool far2b(const slice_args& a, const level_sel& sel, int u0, int u1, int64_t W, bool own2a, const launch_ctx& c)
    {
        const int ns = s.lv.nseg, nf = std::min(a.fnfresh, ns), K = a.fK;
        CHECK(sel.f3 == 0 || sel.f3 == 1);
        for (int u = u0; u < u1; ++u) {
            const int64_t S = far_start(W, u);
            const acc_cell& p1 = acc[size_t(pmod<int64_t>(W, K))][size_t(u)];
            CHECK(p1.win == W && p1.seq < seq);  // phase 1 of this window, in an earlier launch
            int j = 0;
            if (a.f2grp) {
                const int cl = (u / kF1UG) % K;
                j = W >= far_first(cl, K) ? int(pmod<int64_t>(W - cl, K)) : 0;
            }
            CHECK(p1.first == std::max(nf, j + 1));  // with the segments taken here: every segment once
            for (int sg = 0; sg < ns; ++sg) {
                if (!(sg < nf || (sg >= 1 && sg <= std::min(j, ns - 1)))) continue;
                const xf_cell& x = xf[size_t(pmod<int64_t>(W - sg - 1, a.M))][size_t(u)];
                CHECK(x.r0 == S - a.fA - (sg + 1) * int64_t(kFarT));
                CHECK(x.seq < seq || (own2a && sg < nf && x.seq == seq));
            }
            cell& f = ff[sel.f3][size_t(u)];
            CHECK(f.start != S);
            CHECK(f.start == kNever || f.start + kFarT <= c.lo);
            f = cell{S, c.ready, false};
        }
        return true;
    }

    bool far1(const slice_args& a)
    {
        const int ns = s.lv.nseg, nf = std::min(a.fnfresh, ns), K = a.fK, per = kFN / (4 * a.f1fpl);
        CHECK(a.f1fpl == far1_fpl(s) && a.f1nwg % per == 0 && a.f1u0 >= 0 && a.f1u1 <= a.fU);
        const int ng = a.f1nwg / per, ga = a.f1u0 / kF1UG, gb = (a.f1u1 - 1) / kF1UG;
        const int64_t wn = a.f1wn;
        std::vector<char> seen(size_t(gb - ga + 1), 0);
        for (int i = 0; i < ng; ++i) {
            const int g = a.f1g0 + i * a.f1gs;
            CHECK(g >= ga && g <= gb);  // no workgroup without units
            seen[size_t(g - ga)] = 1;
            const int cl = g % K;
            for (int u = std::max(a.f1u0, g * kF1UG); u < std::min(a.f1u1, (g + 1) * kF1UG); ++u) {
                int nw = 1;
                if (a.f1mode && cl != a.f1cls) {
                    if (a.f1mode == 1) CHECK(false && "a group of another class");
                    if (far_first(cl, K) <= wn) continue;  // inside a group started earlier
                } else if (a.f1mode) {
                    nw = K;
                }
                const int64_t S = far_start(wn, u);
                for (int j = 0; j < nw; ++j) {
                    for (int sg = std::max(nf, j + 1); sg < ns; ++sg) {
                        const xf_cell& x = xf[size_t(pmod<int64_t>(wn - (sg - j) - 1, a.M))][size_t(u)];
                        CHECK(x.r0 == S + int64_t(kFarT) * j - a.fA - (sg + 1) * int64_t(kFarT) && x.seq < seq);
                    }
                    acc_cell& p = acc[size_t(pmod<int64_t>(wn + j, K))][size_t(u)];
                    CHECK(p.win != wn + j);
                    p = acc_cell{wn + j, seq, std::max(nf, j + 1)};
                }
            }
        }
        if (a.f1mode != 1)
            for (char v : seen) CHECK(v);  // every group that holds slice units
        else
            for (int g = ga; g <= gb; ++g) CHECK(seen[size_t(g - ga)] == (g % K == a.f1cls));
        return true;
    }

    bool apply(const slice_args& a, const level_sel& sel, const launch_ctx& c)
    {
        ++seq;
        const level_plan& lp = s.lv;
        CHECK(a.ntp <= lp.n);
        for (int l = 0; l < a.ntp; ++l)
            if (!toep(a, sel, l, c)) return false;
        if (!(a.f1nwg || a.f2nwg || a.f3nwg)) return true;
        CHECK(lp.nseg && a.M == lp.nseg && a.fU == int(far_units(s)) && a.fA == lp.farA && a.fK == far_group(s));
        const int f1a = a.f1nwg ? a.f1u0 : 0, f1b = a.f1nwg ? a.f1u1 : 0;
        const int f2a = a.f2u0, f2b = a.f2u0 + a.f2nwg, f3a = a.f3u0, f3b = a.f3u0 + a.f3nwg;
        CHECK(f2a >= 0 && f2b <= a.fU && f3a >= 0 && f3b <= a.fU);
        if (a.f3nwg) {  // phase 2 shares no unit with phase 1 and 2a of its launch
            CHECK(f1b <= f1a || f3b <= f1a || f1b <= f3a);
            CHECK(f2b <= f2a || f3b <= f2a || f2b <= f3a);
        }
        if (a.f3nwg && a.f2comb == 2) {  // recomputed: every segment's rows
            const int64_t S = block_of(a.f2tw, c.prime ? t0 : c.ready);
            CHECK(s.far_raw && (sel.f3 == 0 || sel.f3 == 1));
            if (!reads(S - a.fA + kFarT - 1, S - s.P + 1, c)) return false;
            for (int u = f3a; u < f3b; ++u) {
                CHECK(S == far_start(a.f3wn, u));
                cell& f = ff[sel.f3][size_t(u)];
                CHECK(f.start != S);
                CHECK(f.start == kNever || f.start + kFarT <= c.lo);
                f = cell{S, c.ready, false};
            }
        } else if (a.f3nwg && a.f2comb == 1) {
            const int64_t S = block_of(a.f2tw, c.prime ? t0 : c.ready);
            for (int u = f3a; u < f3b; ++u) CHECK(S == far_start(a.f3wn, u));
            if (!far2a(a, f3a, f3b, S, a.f3wn, c)) return false;
            if (!far2b(a, sel, f3a, f3b, a.f3wn, true, c)) return false;
        } else if (a.f3nwg) {
            if (!far2b(a, sel, f3a, f3b, a.f3wn, false, c)) return false;
        }
        if (a.f1nwg && !far1(a)) return false;
        if (a.f2nwg) {
            const int64_t S = block_of(a.f2tw, c.prime ? t0 : c.ready);
            for (int u = f2a; u < f2b; ++u) CHECK(S == far_start(a.f2wn, u));
            if (!far2a(a, f2a, f2b, S, a.f2wn, c)) return false;
        }
        return true;
    }

    // -- the block role of step n: every class's window, by the selectors ----------------
    bool block_reads(const slice_args& a, const level_sel& sel)
    {
        const level_plan& lp = s.lv;
        CHECK(a.nsl == lp.n && a.a0 == lp.a0);
        for (int l = 0; l <= lp.n; ++l) {
            const bool far = l == lp.n;
            if (far && !lp.nseg) break;
            const int T = far ? kFarT : lp.T[l], lt = log2i(T), L = far ? kLvToep : l;
            const int sh = far ? a.fsh : a.ssh[l], ef = far ? a.fef : a.sef[l];
            const std::vector<int>* cuts = far ? &s.st_fcut : &s.st_cut[l];
            const int upc = far ? s.B / 16 : (s.B / 16) * jh(T);
            CHECK((sh >= 0) == (far ? stag_far(lp) : stag_level(lp, l)));
            for (size_t k = 0; k < cur[L].size(); ++k) {
                int buf = far ? sel.ff : sel.sl[l], row = far ? sel.ff_row : sel.sl_row[l];
                int u0 = 0, u1 = far ? int(ff[0].size()) : int(slab[l][0].size());
                if (sh >= 0) {  // the kernel's row of a channel of class k (block_role)
                    CHECK(buf == 0 && row == 0 && a.stag == lp.stag && a.snm == int(n % (2 * kFarT)));
                    const int c0 = (*cuts)[k], c1 = (*cuts)[k + 1];
                    if (c1 <= c0) continue;
                    for (int c = c0; c < c1; ++c) CHECK(stag_class(a.sM, ef, c, sh) == int(k));
                    int m = a.snm + stag_phi(T, a.stag, int(k));
                    if (mut == kMutEarly && !far && k % 2 == 0) m = a.snm + ((stag_phi(T, a.stag, int(k)) + a.stag) & (T - 1));
                    buf = (m >> lt) & 1;
                    row = m & (T - 1);
                    u0 = c0 * upc;
                    u1 = c1 * upc;
                }
                CHECK((buf == 0 || buf == 1) && row >= 0 && row < T);
                cur_win& cw = cur[L][k];
                if (n == 0 || row == 0) {  // a window's first block: every unit holds it, from a launch ordered before
                    const std::vector<cell>& v = far ? ff[buf] : slab[l][buf];
                    for (int u = u0; u < u1; ++u) {
                        CHECK(v[size_t(u)].start == t - row);
                        CHECK(v[size_t(u)].ready <= t);
                    }
                    cw = cur_win{t - row, buf};
                } else {
                    CHECK(cw.start == t - row && cw.buf == buf);
                }
            }
        }
        return true;
    }

    // -- the walk ------------------------------------------------------------------------
    bool prime()
    {
        t0 = t;
        n = -1;
        plan_parts(s);
        reset();
        const int w = ring_row(t0);
        const launch_ctx c{t0, t0, t0, t0, true, false};
        for (int r = 0; r < prime_rounds(s); ++r) {
            slice_args a = base(), f = base();
            level_sel sa, sf;
            prime_round(s, r, w, a, sa, f, sf);
            if (!apply(a, sa, c) || !apply(f, sf, c)) return false;
        }
        for (int g = -3; s.lv.stag && g < 0; ++g) {
            slice_args b = base();
            level_sel sb;
            slice_part(s, int64_t(g) * s.sg, ring_add(w, int64_t(g) * s.sg, s.ring), b, sb);
            launch_ctx cb = c;
            cb.prime = false;
            cb.even_bg = (g & 1) == 0;
            if (!apply(b, sb, cb)) return false;
        }
        n = 0;
        return true;
    }

    slice_args base() const
    {
        slice_args a{};
        a.ring = s.ring;
        a.C = s.C;
        a.B = s.B;
        if (s.lv.nseg) {
            a.M = a.nseg = s.lv.nseg;
            a.fnfresh = 1;
            a.fU = int(far_units(s));
            a.fK = far_group(s);
            a.P = s.P;
            a.fA = s.lv.farA;
        }
        return a;
    }

    bool step()
    {
        if (n < 0 && !prime()) return false;
        const int G = s.sg, w = ring_row(t);
        slice_args a = base();
        level_sel sel;
        block_rows(s, n, a, sel);
        block_levels(s, n, w, a, sel);
        if (!block_reads(a, sel)) return false;
        if (G > 1 && n % G == 0) {
            const int64_t g = n / G;
            const bool odd = g & 1;
            slice_args b = base();
            level_sel sb;
            slice_part(s, n, w, b, sb);
            const int64_t lim = t0 + std::max<int64_t>(0, (g - (odd ? 1 : 2)) * G), due = t + (odd ? G : 2 * G);
            if (!apply(b, sb, launch_ctx{lim, lim, due, due, false, !odd})) return false;
        }
        if (!apply(a, sel, launch_ctx{t, t, t + 1, t + 1, false, false})) return false;
        ++t;
        ++n;
        return true;
    }

    bool walk()
    {
        const int64_t nb = 2 * int64_t(s.P) + 3 * kFarT + 60;
        for (int64_t i = 0; i < nb; ++i) {
            if (i < 37 || (i >= nb / 2 + 1 && i < nb / 2 + 4)) {  // a plain step: the levels re-prime after it
                ++t;
                n = -1;
            } else if (!step()) {
                if (verbose) std::printf("  at block %lld, step %lld\n", (long long)t, (long long)n);
                return false;
            }
        }
        return true;
    }
};

// persist_far_args over 5 far windows: with kFarT - 2 slices every unit of every window gets phase
// 1, then phase 2 (far2c_role) in a later step, two steps before the window's first block at the
// latest, into the buffer the window's parity names
static bool persist_case(int C, int B, int nseg, int K)
{
    std::string what = "persist_far_args C " + std::to_string(C) + " B " + std::to_string(B) + " K " + std::to_string(K);
    const int U = C * (B / 16), fpl = nseg - 1 <= 4 ? 4 : (nseg - 1 <= 8 ? 2 : 1), ring = 1024;
    std::vector<cf> field(1);
    std::vector<std::vector<int64_t>> p1(size_t(K), std::vector<int64_t>(size_t(U), -1)), p1n = p1;
    std::vector<int64_t> done(size_t(U), 0);
    for (int64_t n = 0; n < 5 * kFarT; ++n) {
        slice_args a{};
        a.C = C;
        a.B = B;
        a.ring = ring;
        persist_far_args(a, n, int(n % ring), U, K, fpl, field.data());
        const int64_t W = n / kFarT + 1;
        if (a.f3nwg) {
            CHECK(a.f2comb == 1 && a.f3wn == W && a.f2grp == (K > 1) && a.f2tw == int((W * kFarT) % ring));
            CHECK(a.f3ff - field.data() == (W & 1) * int64_t(C) * ff_cs(B));
            CHECK(n <= W * kFarT - 2);
            for (int u = a.f3u0; u < a.f3u0 + a.f3nwg; ++u) {
                CHECK(u >= 0 && u < U && done[size_t(u)] == W - 1);
                CHECK(p1[size_t(W % K)][size_t(u)] == W && p1n[size_t(W % K)][size_t(u)] < n);
                done[size_t(u)] = W;
            }
        }
        if (a.f1nwg) {
            const int per = kFN / (4 * fpl), ng = a.f1nwg / per;
            CHECK(a.f1wn == W && a.f1nwg % per == 0 && a.f1u0 >= 0 && a.f1u1 <= U);
            CHECK(!a.f3nwg || a.f3u0 + a.f3nwg <= a.f1u0 || a.f1u1 <= a.f3u0);
            for (int i = 0; i < ng; ++i) {
                const int g = a.f1g0 + i * a.f1gs, cl = g % K;
                for (int u = std::max(a.f1u0, g * kF1UG); u < std::min(a.f1u1, (g + 1) * kF1UG); ++u) {
                    int nw = 1;
                    if (a.f1mode && cl != a.f1cls) {
                        CHECK(a.f1mode == 2);
                        if (world::far_first(cl, K) <= W) continue;
                    } else if (a.f1mode) {
                        nw = K;
                    }
                    for (int j = 0; j < nw; ++j) {
                        CHECK(p1[size_t((W + j) % K)][size_t(u)] != W + j);
                        p1[size_t((W + j) % K)][size_t(u)] = W + j;
                        p1n[size_t((W + j) % K)][size_t(u)] = n;
                    }
                }
            }
        }
        if (n % kFarT == kFarT - 1)
            for (int u = 0; u < U; ++u) CHECK(done[size_t(u)] == W);
    }
    return true;
}

int main(int argc, char** argv)
{
    int mut = kMutNone;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--mutate") && i + 1 < argc) {
            const std::string m = argv[++i];
            mut = m == "band" ? kMutBand : m == "early" ? kMutEarly : m == "cut" ? kMutCut : -1;
        } else if (!std::strcmp(argv[i], "--quiet")) {
            verbose = false;
        }
    }
    if (mut < 0) return 2;
    if (mut != kMutNone) verbose = false;  // every case fails: the counts say it
    for (int i = 1; i < argc; ++i)
        if (!std::strcmp(argv[i], "--verbose")) verbose = true;
    int cases = 0, failed = 0;
    std::set<std::string> seen;  // option values that change nothing of a schedule run once
    for (int C : {1, 4, 24, 32})
        for (int B : {16, 64})
            for (int P : {9, 17, 33, 60, 65, 150, 257, 300, 450, 700, 938})
                for (int G : {1, 2, 4, 8})
                    for (int windows = 1; windows <= (G > 1 ? 2 : 1); ++windows)
                        for (int far_level = 0; far_level <= 2; ++far_level)
                            for (int far_grp = 0; far_grp <= 4; ++far_grp)
                                for (int split = 0; split <= 2; ++split)
                                    for (int ph2 = 0; ph2 <= (G == 1 ? 2 : 0); ++ph2) {
                                        world wd;
                                        wd.mut = mut;
                                        const neo_hip_upols_opts o{-1, 0, 0, 0, -1, far_level, far_grp, split, G, ph2, windows};
                                        // the ring the create path asks for: the batched passes' P + 31 rows and,
                                        // from 128 partitions, the offline windows' 128 (segments + 2) + 1 (the
                                        // staggered prime relies on it: it reads P + 127 rows back)
                                        const int ring = std::max(P + 31, P >= kFarT ? kFarT * ((P + kFarT - 1) / kFarT + 2) + 1 : 0);
                                        if (make_level_sched(C, B, P, ring, o, false, false, wd.s)) continue;  // rejected
                                        level_sched& s = wd.s;
                                        if (mut == kMutBand || mut == kMutEarly) {
                                            if (!s.lv.stag) continue;
                                            int l = 0;
                                            while (l < s.lv.n && !stag_level(s.lv, l)) ++l;
                                            if (l == s.lv.n) continue;
                                            if (mut == kMutBand) {
                                                --s.lv.a[l];
                                                --s.lv.b[l - 1];
                                                if (s.lv.nseg && s.lv.farA == kFarT + 4 * G) {
                                                    --s.lv.farA;
                                                    --s.lv.b[s.lv.n - 1];
                                                }
                                            }
                                        }
                                        std::string key;
                                        for (int v : {C, B, P, s.ring, s.sg, int(s.far_raw), s.lv.n, s.lv.nseg, s.lv.farA, s.lv.stag,
                                                      s.lv.nseg ? far_group(s) : 0, P > 64 ? wd.jh(32) : 0,
                                                      s.lv.nseg && !s.far_raw && s.sg == 1 ? int(far2_whole(s)) : 2})
                                            key += std::to_string(v) + ",";
                                        for (int l = 0; l < s.lv.n; ++l)
                                            key += std::to_string(s.lv.T[l]) + ":" + std::to_string(s.lv.a[l]) + ":" + std::to_string(s.lv.b[l]) + ",";
                                        if (!seen.insert(key).second) continue;
                                        wd.what = key;
                                        ++cases;
                                        if (!wd.walk()) ++failed;
                                    }
    if (mut == kMutNone)
        for (int C : {1, 2, 16})
            for (int B : {16, 64, 512})
                for (int nseg : {1, 2, 6, 13})
                    for (int K : {1, 2}) {
                        if (nseg < 2 && K > 1) continue;
                        ++cases;
                        if (!persist_case(C, B, nseg, K)) ++failed;
                    }
    std::printf("%d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
