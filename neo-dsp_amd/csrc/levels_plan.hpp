// levels_plan.hpp — the streaming levels of the dense convolver, host side: the level plan, the
// step groups' background plan, the staggered classes, and the schedule (which role computes which
// units of which window in which launch), as pure functions on level_sched. No HIP header: a
// plain C++ compiler builds it (tests/cpp/levels_plan_main.cpp walks the schedule under the
// sanitizers), and nothing here sees a device address -- the schedule fills the non-pointer fields
// of the kernel arguments (slice_args, toep_arg) and names every buffer and row in a level_sel,
// which bind (upols_levels.hip) turns into pointers. The kernels, the launches and the streams:
// upols_levels.hip.
//
//   constants, level_plan, strides        the shapes of the levels and of their buffers
//   slice_args, toep_arg, level_sel       the kernel arguments and the pointer selectors
//   level_sched, make_level_sched         what plan and schedule read; the create path's defaults
//   plan_levels, plan_levels_stag         bands per level
//   part_plan, stag_classes, plan_parts   background parts per step group, classes of channels
//   toep_fill, far1_args, far2_fill ...   one helper per kind of role
//   block_rows, block_levels, slice_part  the roles of a step's launch, of a background launch
//   prime_rounds, prime_round             window 0 of every level and class
#pragma once

#include "../../include/neo_hip.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define NEO_LV_HD __host__ __device__
#else
#define NEO_LV_HD
namespace neo_hip {
struct alignas(8) cf {  // the host build: the kernels' complex type (fft_device.hpp), only pointed to
    float x, y;
};
}  // namespace neo_hip
#endif

namespace neo_hip {

constexpr int kLvA0 = 8;     // partitions the block itself MACs (p < kLvA0)
constexpr int kLvToep = 5;   // Toeplitz level slots: l < 4 window kLvT0 << l; slot 4 the big level
constexpr int kLvT0 = 4;
constexpr int kBigT = 128;   // big Toeplitz level: window, band [2 kBigT, P) instead of the far level (opt-in:
                             // 26.9 vs 19.2 us per C5 step, its 89 M complex MACs per step are VALU / LDS bound)
constexpr int kBigJH = 8;    // its window parts per column group
constexpr int kFarT = 128;   // far level: blocks per window (256-point partition-axis transform)
constexpr int kFarA = 256;   // far level: first partition (2 kFarT)
constexpr int kFarRing = 2 * kFarA;  // far level: FDL ring rows needed (a slice reads back 383 blocks)
constexpr int kFN = 2 * kFarT;       // far level: partition-axis transform length
constexpr int kT32BandMax = 192;     // the T = 32 level's LDS tile (kT32Band)
// far phase 1: units per group (a group's classes share a pass), the most windows per pass
constexpr int kF1UG = 4;
constexpr int kFarKMax = 4;
// windows per far phase-1 pass (far1_mac): K ~ sqrt(2 (nseg - 1)) minimizes the spectra read per
// window and column, 2 (nseg - 1) / K + K - 1; but phase 2 takes up to K - 1 extra segments in
// its one-workgroup-per-unit chain, which bounds the step where a step has few far units
// (measured: K = 3 / 4 instead of 2 at 64 / 32 units per step, C5 / C4: 13 % / 25 % slower; at
// 512, the 2048-channel headline: 3 % faster; round 5, the 4-GPU shard of the headline, 512
// channels = 128 units per step: K = 3 2-3.5 % faster, tools/gpu_shard_sweep.sh), so K = 2 below
// kFarGroupUnits units
constexpr int64_t kFarGroupUnits = 16384;  // 128 units per step
// steps per background launch of the level slices (launch_levels): 4 from kStepGroupUnits
// 16-column units (same-box A/B, ms per step at G = 1 / 4: C5 0.0183 / 0.0165, C4 0.0155 / 0.0134,
// c5full 0.1213 / 0.1215 with the host round trip per block 133 -> 63 us; at one channel, C3, the
// block launch and the cross-stream waits cost more than the overlap gives: 0.0063 / 0.0083)
constexpr int64_t kStepGroupUnits = 2048;
// Far phase 2 at G = 1 in one workgroup per unit (far2c_role, one step after phase 1) or in
// two (2a: the fresh transform -> its slot, beside phase 1; 2b: the products and the inverse one
// step later). One workgroup reads the fresh spectrum back from registers instead of its slot,
// fewer bytes; two halve the chain, which bounds the step where a step has few far units.
// Step groups always run one (their background launches have a group of slack).
constexpr int64_t kFarWholeUnits = 32768;  // 256 units per step
constexpr int64_t kStaggerUnits = 65536;   // 16-column units from which windows = 0 (auto) staggers

struct level_plan {
    int a0 = 1;                      // the block step takes partitions [0, a0)
    int n = 0;                       // Toeplitz levels
    int T[kLvToep] = {}, a[kLvToep] = {}, b[kLvToep] = {};  // window (blocks) and partition band [a, b) per level
    int nseg = 0;                    // far segments of kFarT partitions from farA (0: no far level)
    int farA = kFarA;                // the far level's first partition (staggered windows: plan_levels_stag)
    int stag = 0;                    // staggered windows: the step group G they are planned for (0: aligned)
};

// Staggered windows (plan_levels_stag): a level of window T >= 4 G (and the far level) is cut
// into T / G classes of channels, class k computed in the background launches of the
// groups g = k mod T / G for the window starting at block (g + 2) G, so its band starts at T + 4 G.
// A channel's class: its position in 1/1024ths of a pair of far classes is (c M) >> 20 with
// M = ((64 / G) << 30) / C, shifted right by log2(128 / T) for a level of window T; the even class
// of a pair takes the first ef of its 1024 parts.
NEO_LV_HD inline int stag_class(unsigned long long M, int ef, int c, int shift)
{
    const int p = int((static_cast<unsigned long long>(c) * M) >> 20) >> shift;
    return 2 * (p >> 10) + ((p & 1023) >= ef ? 1 : 0);
}
// windows of class k start where (n + phi) mod T = 0
NEO_LV_HD inline int stag_phi(int T, int G, int k) { return (-(k + 2) * G) & (T - 1); }

// Channel strides (complex units) of the level buffers: kPad rows more than the data, so that no
// channel stride is a multiple of a large power of two -- every channel's row n of a slab, of the
// far field or of a segment spectrum would otherwise sit at the same offset modulo 512 KB .. 8 MB
// (an FDL ring of 1280 rows, 5 x 2^20 bytes per channel at B = 512, cost the c5full step 4 %)
#ifndef NEO_PAD
#define NEO_PAD 1  // diagnostic builds (A/B): 0 = unpadded strides
#endif
constexpr int kPad = NEO_PAD;
NEO_LV_HD constexpr int64_t slab_cs(int T, int B) { return int64_t(T + kPad) * B; }
NEO_LV_HD constexpr int64_t ff_cs(int B) { return int64_t(kFarT + kPad) * B; }
NEO_LV_HD constexpr int64_t spec_cs(int nseg, int B) { return (int64_t(nseg) * kFN + kPad) * B; }

// x mod n in [0, n) for any sign of x
template<class I>
NEO_LV_HD constexpr I pmod(I x, I n)
{
    return ((x % n) + n) % n;
}
inline int ring_add(int64_t r, int64_t d, int R) { return int(pmod<int64_t>(r + d, R)); }
inline int log2i(int v) { return v <= 1 ? 0 : 1 + log2i(v >> 1); }

// ---------------------------------------------------------------------------------------
// The arguments of the step kernels (k_lvl_step, k_lvl_block, k_lvl_slices): one launch, workgroups
// by role.
//   block     this step's block: its spectrum's partitions 0 .. a0 - 1 plus the level slabs and the
//             far field of this block (their windows finished in earlier launches)
//   Toeplitz  a slice of the next window of each Toeplitz level (some of its 16-column units)
//   far       a slice of the next far window (some of its 16-column units), in phases
// No role reads what another role of the same launch writes.
struct toep_arg {
    cf* slab;           // the target window's slabs [C][T][B]
    int T, a, b;        // window, band [a, b)
    int tw;             // ring row of the window's first block
    int u0, u1, nwg;    // units (16 columns x one of JH window parts) of this slice, workgroups
    int jh;             // window parts per column group (toep_geom)
    int64_t cs;         // the slab's channel stride (slab_cs)
};

struct slice_args {
    const cf* H;
    cf* fdl;
    int ring, C, B;
    int64_t cstride, pstride;
    // block role: this step's block, one workgroup per channel (nblk = 0 in priming launches)
    // from channel blk_c0 on
    int nblk, blk_c0;
    const float* in;
    int64_t ld_in;
    float* out;
    int64_t ld_out;
    float* prev;
    float* snap;            // not null: a copy of each channel's input block, [C][B] (upols_group.hip: the
                            // frame the leader's launch read in place, for the later members' comparisons)
    const cf* twg;
    int w, a0;              // ring row of the block; partitions the block role MACs directly
    int nsl;
    const cf* sl[kLvToep];  // slab row of this block per level, channel 0
    int64_t scs[kLvToep];   // channel strides
    const cf* ff;           // far field row of this block, channel 0 (null: no far level)
    int64_t fcs;
    // staggered windows (stag = G, else 0): the row depends on the channel's class (stag_class, stag_phi).
    // A level with ssh[l] >= 0 (the far level: fsh) gives its slab's base in sl[l] (ff) and the block
    // role adds the buffer and row of step snm = n mod 256 in the class's window
    int stag, snm, fsh, fef;
    int ssh[kLvToep], sef[kLvToep];  // per level: position shift, the even classes' share (1/1024ths)
    unsigned long long sM;
    // Toeplitz roles
    int ntp;
    toep_arg tp[kLvToep];
    // far level (16-column units), common
    int M, nseg, fnfresh, P;
    int fA;       // the far level's first partition (level_plan::farA)
    int64_t fsc;  // segment / row-pair spectra channel stride (spec_cs; M = nseg slots)
    const cf* hf;
    cf* xf;
    const cf* twf;
    int fU;     // units (16 columns) of all channels
    // far phase 1: stored-segment MAC, groups of kF1UG units; in pair mode a group takes two
    // windows at once (far1_role)
    int f1nwg, f1u0, f1u1, f1wn, f1fpl;  // slice units [f1u0, f1u1); target window; f rows per lane
    int fK;                              // windows per phase-1 pass (1: one window per pass)
    int f1g0, f1gs, f1mode, f1cls;       // first group, group step; 0 single, 1 the class's groups, 2 every group; class
    cf* f1acc;  // partial sums [fK (window mod fK)][fU][256 f][16]
    // far phase 2a (the slice phase 1 takes in the same launch): the fresh row pairs'
    // transforms, stored to their ring slots
    int f2nwg, f2u0, f2tw, f2wn;
    // far phase 2b (the slice of the previous launch): the stored fresh spectra's products,
    // phase 1's partial sums, the window group's extra segments, the inverse transform
    int f3nwg, f3u0, f3wn;
    int f2grp;    // phase-1 window groups on: a unit in window j of its group takes segments 1..j in 2b
    int f2comb;   // 1: 2b also runs 2a's fresh transform for its units (f2tw: its rows), no slot read-back (far2c_role);
                  // 2: the recomputed far level (far2r_role, every segment from the filter and FDL rows)
    cf* f2acc;    // as f1acc
    cf* f3ff;     // 2b's target far window [C][128][B]
    void* tl;     // timeline builds (NEO_TIMELINE): per-workgroup records of the launch
    int bid0;     // paced background pieces: the first workgroup of the launch this piece runs
};

// Where the schedule points four kinds of pointer field of a launch's slice_args, by buffer (the
// slabs and the far field are double-buffered: 0 / 1) and row; -1: the field stays null.
struct level_sel {
    int tp[kLvToep] = {-1, -1, -1, -1, -1};  // tp[l].slab: the buffer of level l's slabs the role writes
    int sl[kLvToep] = {-1, -1, -1, -1, -1};  // sl[l]: buffer and row of the block's slab row; a staggered level
    int sl_row[kLvToep] = {};                // (ssh[l] >= 0) gets the slabs' base, buffer 0 row 0
    int ff = -1, ff_row = 0;                 // ff: the block's far-field row, as sl
    int f3 = -1;                             // f3ff: the far-field buffer phase 2 writes
};

// ---------------------------------------------------------------------------------------
// What the plan and the schedule read of a handle, and nothing that lives on the device.
struct level_sched {
    int C = 0, B = 0, P = 0;
    int ring = 0;  // FDL ring rows R = P + kMaxBatch - 1 (at least kFarRing with a far level)
    // step groups (neo_hip_upols_opts.step_group, G = sg): G = 1 runs a step as ONE launch (the
    // block and 1/T of every level's next window); G > 1 runs the block of every call alone on the
    // caller's stream and the level slices of G steps as one launch on the handle's background
    // stream, one step group ahead
    int sg = 1;
    bool persist = false;  // latency mode requested (neo_hip_upols_set_persistent): its own schedule
    bool far_raw = false;  // far level recomputed every window from the filter and FDL rows
                           // (neo_hip_upols_opts.far_level 2; far2r_role): no stored spectra or sums
    int far_k = 0;         // far phase-1 windows per pass forced by neo_hip_upols_opts.far_group (0: auto)
    int toep_jh = 0;       // T = 32 window parts forced by neo_hip_upols_opts.toep_split (0: auto)
    int f2mode = 0;        // far phase 2 at G = 1 forced by neo_hip_upols_opts.far_phase2 (0: auto)
    level_plan lv;
    // step groups (plan_parts, when the levels prime): per Toeplitz level the window offset phi
    // (windows start at t0 + W T - phi) and the unit cuts of its background parts per window of a
    // cycle of lv_cyc groups
    int lv_phi[kLvToep] = {};
    int lv_cyc = 1;
    std::vector<int> lv_cut[kLvToep];
    std::vector<int> fv_cut;  // step groups: the far slices' first units (ns + 1 cuts; empty: equal slices)
    // staggered windows (lv.stag): the first channel of every class per level and of the far level
    // (T / G + 1 cuts), the even classes' share of a pair in 1/1024ths per level and of the far level
    std::vector<int> st_cut[kLvToep], st_fcut;
    int st_ef[kLvToep] = {}, st_fef = 512;
};

// ---------------------------------------------------------------------------------------
// The level plan. The partitions are cut into bands:
//   p in [0, 8)                   the block itself (its own FDL row and 7 older ones)
//   Toeplitz  [8, 16) [16, 32) [32, 64) [64, 256): windows of T = 4, 8, 16, 32 blocks
//   far       p in [256, P)       T = 128, by a 256-point transform along the partition axis
// far: -1 auto (= 1), 0 the big Toeplitz level, 1 the far level
inline void plan_levels(int P, level_plan& lp, int far = -1)
{
    lp = level_plan{};
    lp.a0 = std::min(P, kLvA0);
    constexpr int T[4] = {4, 8, 16, 32}, A[4] = {8, 16, 32, 64}, Bd[4] = {16, 32, 64, kFarA};
    for (int l = 0; l < 4; ++l) {
        if (P <= A[l]) break;
        lp.T[lp.n] = T[l];
        lp.a[lp.n] = A[l];
        lp.b[lp.n] = std::min(P, Bd[l]);
        ++lp.n;
    }
    if (P <= kFarA) return;
    if (far != 0) {
        lp.nseg = (P - kFarA + kFarT - 1) / kFarT;
    } else {  // [256, P) by the big Toeplitz level (slot 4)
        lp.T[lp.n] = kBigT;
        lp.a[lp.n] = 2 * kBigT;
        lp.b[lp.n] = P;
        ++lp.n;
    }
}

inline int far_group_auto(int C, int B, int ns)
{
    if (ns < 2) return 1;
    if (int64_t(C) * (B / 16) < kFarGroupUnits) return 2;
    const int K = int(std::lround(std::sqrt(2.0 * (ns - 1))));
    return std::min(kFarKMax, std::max(2, K));
}

// the automatic far phase-1 window group / T = 32 window parts / step group a handle of C channels
// would use. T = 32 splits its window in two where a step has fewer than 8 of its units (few
// channels: the part halves the step's longest chain).
inline int far_group_for(int C, int B, int P)
{
    level_plan lp;
    plan_levels(P, lp);
    return lp.nseg ? far_group_auto(C, B, lp.nseg) : 0;
}
inline int toep_split_for(int C, int B) { return C * (B / 16) < 8 * 32 ? 2 : 1; }
inline int step_group_for(int C, int B, int P)
{
    (void)P;
    return int64_t(C) * (B / 16) >= kStepGroupUnits && B <= 1024 ? 4 : 1;
}

// The byte model (bench.algorithmic_bytes), in rows of one channel column:
// a Toeplitz window reads its band of the filter and the FDL rows it meets and writes T rows;
// far phase 1 reads the stored spectra and writes the partial sums, phase 2 the fresh pair, the
// products, the field and the sums; the recomputed form every segment's rows and the band.
inline double toep_rows(int a, int b, int T) { return 2.0 * (b - a) + 2 * T - 1; }
inline double far1_rows(int nseg, int K) { return 256.0 * 2 * (nseg - 1) / K + 256; }
inline double far2_rows(int K) { return 256.0 * (3 + K - 1) + 128 + 256; }
inline double far_raw_rows(int nseg, int P) { return (nseg + 1) * 128.0 + (P - 256) + 128; }

// Staggered windows (step groups of G blocks). In the aligned plan every slice of a window shares
// the window's start, so the band starts at 2 T: a slice computed early in the previous window
// waits up to T - 1 steps for its first read. Here a level of window T >= 4 G is cut into T / G
// classes of channels and class k has a window phase of its own: it is computed whole in the
// background launch of group g = k mod T / G, for the window that starts at block s = (g + 2) G.
// That launch is guaranteed the FDL rows before (g - 2) G = s - 4 G (an even group's launch only
// follows its odd predecessor, which waited for the blocks before the group before it) and is
// first waited for at block (g + 2) G (launch_levels), and the window's rows s + j - p end at
// s + T - 1 - a: the band may start at a = T + 4 G. The far level likewise (phase 1 of a class two
// groups before its phase 2, whose fresh row pair ends at s - F + 127): F >= 128 + 4 G. A class's
// slab buffer is rewritten T / G groups after it was written, T - 2 G >= 2 G steps after the block
// launch that waited for it was issued.
// G = 4: [8, 16) [16, 32) as aligned, T = 16 [32, 48), T = 32 [48, F), far from F in [144, 240]:
// the F with the fewest bytes by the model of DESIGN 5 (the T = 32 band's 2 (F - 48) + 63 rows per
// 32 steps against the far level's 512 (nseg - 1) / K + 256 (K + 3) + 384 per 128; the sum is kept
// in this order, which decides between two F), the fewer segments where two are within half a percent.
// far_k: the forced far window group, 0 auto.
inline void plan_levels_stag(int P, int C, int B, int G, int far_k, level_plan& lp)
{
    lp = level_plan{};
    lp.stag = G;
    lp.a0 = std::min(P, kLvA0);
    int A[5];
    for (int l = 0; l < 4; ++l) A[l] = (kLvT0 << l) > 4 * G ? (kLvT0 << l) + 4 * G : 2 * (kLvT0 << l);
    const int Fmin = kFarT + 4 * G, Fmax = A[3] + kT32BandMax;
    int F = P, nseg = 0;
    if (P > Fmin) {
        double best = 1e300;
        for (int ns = std::max(1, (P - Fmax + kFarT - 1) / kFarT); ns <= (P - Fmin + kFarT - 1) / kFarT; ++ns) {
            const int f = std::max(Fmin, P - kFarT * ns), K = ns < 2 ? 1 : (far_k ? far_k : far_group_auto(C, B, ns));
            const double rows = toep_rows(A[3], f, 32) / 32 + (512.0 * (ns - 1) / K + 256.0 * (K + 3) + 384) / kFarT;
            if (rows < best * 0.995) {
                best = rows;
                F = f;
                nseg = ns;
            }
        }
    }
    A[4] = F;
    for (int l = 0; l < 4; ++l) {
        if (P <= A[l]) break;
        lp.T[lp.n] = kLvT0 << l;
        lp.a[lp.n] = A[l];
        lp.b[lp.n] = std::min(P, A[l + 1]);
        ++lp.n;
    }
    lp.farA = F;
    lp.nseg = nseg;
}

// ---------------------------------------------------------------------------------------
// What the schedule derives from a level_sched

inline int64_t far_units(const level_sched& s) { return int64_t(s.C) * (s.B / 16); }

// phase 1 f rows per lane: one load round covers the stored segments (far1_role)
inline int far1_fpl(const level_sched& s)
{
#ifdef NEO_FAR_FPL  // diagnostic builds
    return NEO_FAR_FPL;
#endif
    return s.lv.nseg - 1 <= 4 ? 4 : (s.lv.nseg - 1 <= 8 ? 2 : 1);
}

inline int far_group(const level_sched& s)
{
    const int ns = s.lv.nseg;
    if (ns < 2 || s.far_raw) return 1;  // recomputed: every window on its own
    if (s.far_k) return s.far_k;  // neo_hip_upols_opts.far_group (tests, A/B runs)
    return far_group_auto(s.C, s.B, ns);
}

// Toeplitz role geometry per window T (k_lvl_step's level roles): window parts per column
// group and units per workgroup
inline void toep_geom(const level_sched& s, int T, int& JH, int& UPW)
{
    JH = T == kBigT ? kBigJH : (T == 32 ? (s.toep_jh ? s.toep_jh : toep_split_for(s.C, s.B)) : 1);
    UPW = T <= 8 ? 16 : (T <= 32 ? 32 / T : 1);  // toep_role<T, 2T, 1, 1>: 16 units; toep_tile: 32 / T
}

inline int64_t toep_units(const level_sched& s, int T)
{
    int JH, UPW;
    toep_geom(s, T, JH, UPW);
    return int64_t(s.C) * (s.B / 16) * JH;
}

// Step groups: the Toeplitz levels stepped in the block launches, 1/T of the next window per step
// (the others in the background launches, T / G - 1 parts per window). T < 2 G must (a background
// launch may not read the blocks of its own group); larger windows may (diagnostic builds).
#ifndef NEO_BLOCK_TMAX
#define NEO_BLOCK_TMAX 0
#endif
inline bool block_level(const level_sched& s, int T) { return T < 2 * s.sg || T <= NEO_BLOCK_TMAX; }

// The far level's units are cut into slices per window. G = 1: kFarT - 1 slices, slice q of
// window W runs phase 1 and 2a at step q of window W - 1 (2a reads FDL rows up to the last block
// before that window) and 2b at step q + 1 (<= the window's last: the far field is complete when
// window W's first block runs). G > 1 (step groups, slice_part): kFarT / G - 2 slices, phase 1
// of slice q at step group q + 1 of window W - 1 (its launch waits only for the blocks before the
// previous group), phase 2 (far2c_role: 2a and 2b in one workgroup) at group q + 2.
inline int far_nslices(const level_sched& s) { return s.sg == 1 ? kFarT - 1 : kFarT / s.sg - 2; }

inline int far_u(int64_t U, int q, int ns) { return int(q * U / ns); }

// the first unit of far slice q: step groups take the planned cuts (part_plan), G = 1 equal slices
inline int far_cut(const level_sched& s, int q)
{
    if (!s.fv_cut.empty()) return s.fv_cut[size_t(q)];
    return far_u(far_units(s), q, far_nslices(s));
}

inline bool far2_whole(const level_sched& s)
{
    if (s.sg > 1) return true;
    if (s.f2mode) return s.f2mode == 1;  // neo_hip_upols_opts.far_phase2
    return far_units(s) >= kFarWholeUnits;
}

// staggered windows: level l has classes of its own (plan_levels_stag)
inline bool stag_level(const level_plan& lp, int l) { return lp.stag && lp.T[l] >= 4 * lp.stag; }
inline bool stag_far(const level_plan& lp) { return lp.stag && lp.nseg; }
inline unsigned long long stag_mul(const level_sched& s) { return ((64ull / unsigned(s.lv.stag)) << 30) / unsigned(s.C); }

// ---------------------------------------------------------------------------------------
// Step groups: the background levels' window offsets and part sizes. A window's first group
// carries none of its level's parts (they read the window's rows), so with every window starting at
// a multiple of its length the groups at multiples of 8 (G = 4) had no Toeplitz work at all and
// the odd ones all of the 8-block level's: background launches of 0.9 to 2.1 GB at c5full, and a
// 20-step sample of the stream 5-8 % above or below the far window's mean. So a level of window
// T >= 4 G (up to 32 blocks: its prime reads at most 16 rows further back) starts its windows half a
// window later (phi = T / 2; still at even groups, which the events need), which puts the groups it
// skips apart from every other level's (2 G: odd groups carry it, 4 G: skips 2 mod 4, 8 G: 4 mod 8,
// the far level: 0 mod kFarT / G); and each window's units are cut into parts of unequal sizes so
// that, over a cycle of groups (the far window, else the longest level window), every group's
// background bytes come as close to equal as the slots allow: min-max water filling of one window
// at a time against the rest (the far slices' bytes fixed), swept until it settles.
inline int part_phi(int T, int G, bool bg) { return bg && G > 1 && T >= 4 * G && T <= 32 ? T / 2 : 0; }

struct part_level {
    int T = 0, UPW = 1;
    bool bg = false;
    int64_t U = 0;
    double wbytes = 0;  // bytes per window
};

// phi, cycle length (groups), cuts [k][j] (k < cyc / (T / G) windows of the cycle, j <= T / G - 1)
// per level and the far slices' unit cuts fcut[0 .. ns] (ns > 0); loads: the predicted background
// bytes per group of the cycle (null: not wanted). balance = false: equal parts, no offsets.
inline void part_plan(const part_level* lv, int nl, int G, int64_t FU, int ns, double c1, double c2, bool far_raw,
                      bool balance, int* phi, int& cyc, std::vector<int>* cut, std::vector<int>& fcut,
                      std::vector<double>* loads)
{
    cyc = 1;
    for (int l = 0; l < nl; ++l) {
        phi[l] = balance ? part_phi(lv[l].T, G, lv[l].bg) : 0;
        cut[l].clear();
        if (lv[l].bg) cyc = std::max(cyc, lv[l].T / G);
    }
    if (ns) cyc = std::max(cyc, kFarT / G);
    // the far slices (slice_part): slice q's phase 1 at group q + 1, phase 2 at q + 2 (recomputed:
    // all of it at q + 2), s[q] units each
    std::vector<double> fs(size_t(ns), ns ? double(FU) / ns : 0.0), load(size_t(cyc), 0.0);
    auto far_add = [&](std::vector<double>& L, const std::vector<double>& sq, double sign) {
        for (int q = 0; q < ns; ++q) {
            if (!far_raw) L[size_t(q + 1)] += sign * c1 * sq[size_t(q)];
            L[size_t(q + 2)] += sign * c2 * sq[size_t(q)];
        }
    };
    far_add(load, fs, 1.0);
    struct win {
        int l, np;
        double c;
        std::vector<int> grp;
        std::vector<double> x;  // units per part
    };
    std::vector<win> ws;
    for (int l = 0; l < nl; ++l) {
        if (!lv[l].bg || lv[l].U <= 0) continue;
        const int Tg = lv[l].T / G, np = Tg - 1, s0 = pmod(-phi[l] / G, Tg);
        for (int k = 0; k < cyc / Tg; ++k) {
            win w{l, np, lv[l].wbytes / double(lv[l].U), {}, std::vector<double>(size_t(np), double(lv[l].U) / np)};
            for (int j = 1; j <= np; ++j) w.grp.push_back((s0 + k * Tg + j) % cyc);
            for (int j = 0; j < np; ++j) load[size_t(w.grp[size_t(j)])] += w.c * w.x[size_t(j)];
            ws.push_back(std::move(w));
        }
    }
    std::vector<double> base, sb, grad, y;
    for (int round = 0; round < (balance ? 4 : 0); ++round) {
        // the Toeplitz windows, one at a time against the rest: min-max water filling
        for (int sweep = 0; sweep < 32; ++sweep)
            for (auto& w : ws) {
                const int np = w.np;
                base.assign(size_t(np), 0.0);
                for (int j = 0; j < np; ++j) {
                    load[size_t(w.grp[size_t(j)])] -= w.c * w.x[size_t(j)];
                    base[size_t(j)] = load[size_t(w.grp[size_t(j)])];
                }
                sb = base;
                std::sort(sb.begin(), sb.end());
                const double total = w.c * double(lv[w.l].U);
                double h = sb[0], acc = 0;  // water level: sum of max(0, h - base) = the window's bytes
                for (int i = 0; i < np; ++i) {
                    const double next = i + 1 < np ? sb[size_t(i + 1)] : 1e300;
                    const double need = (next - sb[size_t(i)]) * (i + 1);
                    if (acc + need >= total) {
                        h = sb[size_t(i)] + (total - acc) / (i + 1);
                        break;
                    }
                    acc += need;
                }
                for (int j = 0; j < np; ++j) {
                    w.x[size_t(j)] = std::max(0.0, h - base[size_t(j)]) / w.c;
                    load[size_t(w.grp[size_t(j)])] += w.c * w.x[size_t(j)];
                }
            }
        if (!ns) break;
        // the far slices against the rest: least squares around the mean, projected gradient on
        // {s >= 0, sum s = FU} (the min-max recurrence is unstable: phase 2 bytes > phase 1's)
        double mean = 0;
        for (double v : load) mean += v;
        mean /= cyc;
        const double eta = 1.0 / (2.0 * (c1 + c2) * (c1 + c2));
        for (int it = 0; it < 400; ++it) {
            grad.assign(size_t(ns), 0.0);
            for (int q = 0; q < ns; ++q) {
                if (!far_raw) grad[size_t(q)] += 2 * c1 * (load[size_t(q + 1)] - mean);
                grad[size_t(q)] += 2 * c2 * (load[size_t(q + 2)] - mean);
            }
            far_add(load, fs, -1.0);
            y.resize(size_t(ns));
            for (int q = 0; q < ns; ++q) y[size_t(q)] = fs[size_t(q)] - eta * grad[size_t(q)];
            sb = y;  // projection onto the simplex: subtract tau, clip at 0
            std::sort(sb.begin(), sb.end(), std::greater<double>());
            double cs = 0, tau = 0;
            for (int i = 0; i < ns; ++i) {
                cs += sb[size_t(i)];
                const double t = (cs - double(FU)) / (i + 1);
                if (sb[size_t(i)] - t > 0) tau = t;
            }
            for (int q = 0; q < ns; ++q) fs[size_t(q)] = std::max(0.0, y[size_t(q)] - tau);
            far_add(load, fs, 1.0);
        }
    }
    for (int l = 0; l < nl; ++l)
        if (lv[l].bg) cut[l].assign(size_t(cyc / (lv[l].T / G) * (lv[l].T / G)), 0);
    std::vector<int> kcount(size_t(nl), 0);
    for (const auto& w : ws) {  // cuts on workgroup multiples, the last at U
        const int64_t U = lv[w.l].U, q = lv[w.l].UPW;
        int* c = cut[w.l].data() + size_t(kcount[size_t(w.l)]++) * size_t(w.np + 1);
        double cum = 0;
        c[0] = 0;
        for (int j = 1; j <= w.np; ++j) {
            cum += w.x[size_t(j - 1)];
            const int64_t r = j == w.np ? U : std::min<int64_t>(U, std::llround(cum / double(q)) * q);
            c[j] = int(std::max<int64_t>(c[j - 1], r));
        }
    }
    fcut.assign(ns ? size_t(ns + 1) : 0, 0);
    if (ns) {
        double cum = 0;
        for (int q = 1; q <= ns; ++q) {
            cum += fs[size_t(q - 1)];
            const int64_t r = q == ns ? FU : std::min<int64_t>(FU, std::llround(cum));
            fcut[size_t(q)] = int(std::max<int64_t>(fcut[size_t(q - 1)], r));
        }
    }
    if (loads) {  // from the integer cuts
        loads->assign(size_t(cyc), 0.0);
        std::vector<double> fi(static_cast<size_t>(ns));
        for (int q = 0; q < ns; ++q) fi[size_t(q)] = double(fcut[size_t(q + 1)] - fcut[size_t(q)]);
        far_add(*loads, fi, 1.0);
        std::fill(kcount.begin(), kcount.end(), 0);
        for (const auto& w : ws) {
            const int* c = cut[w.l].data() + size_t(kcount[size_t(w.l)]++) * size_t(w.np + 1);
            for (int j = 1; j <= w.np; ++j) (*loads)[size_t(w.grp[size_t(j - 1)])] += w.c * double(c[j] - c[j - 1]);
        }
    }
}

// The staggered levels' classes: every background launch carries one class of every staggered
// level, phase 2 of one far class and phase 1 of the next, the same work in every group -- but the
// aligned levels of window 2 G ride on the odd groups alone (X bytes per two groups). Classes come
// in pairs of an even and an odd one (class parity = group parity of its Toeplitz slice and both
// its far phases), so the even classes take the share e / 2 of every pair with e = 1 + X / (2 D),
// D the staggered bytes per group: both parities then carry the same bytes. Classes are whole
// channels, so the far level (the most classes) takes its share first and every level after it
// the rest that the rounding of those before it left.
inline void stag_classes(level_sched& s, std::vector<double>* loads)
{
    const level_plan& lp = s.lv;
    const int G = lp.stag, C = s.C;
    const double col = double(s.B) * 8;  // bytes of one row of one channel
    double X = 0, St = 0, c1 = 0, c2 = 0;
    for (int l = 0; l < lp.n; ++l) {
        const double wb = col * toep_rows(lp.a[l], lp.b[l], lp.T[l]);  // per channel and window
        if (stag_level(lp, l)) St += wb * G / lp.T[l];
        else if (!block_level(s, lp.T[l]) && lp.T[l] == 2 * G) X += wb;
    }
    if (lp.nseg) {
        const int K = far_group(s);
        c1 = col * far1_rows(lp.nseg, K) * G / kFarT;
        c2 = col * far2_rows(K) * G / kFarT;
    }
    double Drest = St + c2 + c1, Xrest = X;  // what the levels not yet cut can still move
    const unsigned long long M = stag_mul(s);
    auto cuts = [&](int T, double Dl, std::vector<int>& cut) {
        const int ncls = T / G, sh = log2i(kFarT / T);
        const double e = Drest > 0 ? std::max(0.5, std::min(1.5, 1.0 + Xrest / (2.0 * Drest))) : 1.0;
        const int ef = int(std::lround(512.0 * e));
        cut.assign(size_t(ncls) + 1, C);
        cut[0] = 0;
        for (int c = C - 1; c >= 0; --c) {
            const int k = stag_class(M, ef, c, sh);
            for (int j = k; j >= 1 && cut[size_t(j)] > c; --j) cut[size_t(j)] = c;  // first channel of class >= j
        }
        int even = 0;
        for (int k = 0; k < ncls; k += 2) even += cut[size_t(k) + 1] - cut[size_t(k)];
        Xrest -= (4.0 * even / C - 2.0) * Dl;  // the share the whole channels gave
        Drest -= Dl;
        return ef;
    };
    s.st_fcut.clear();
    s.st_fef = 512;
    if (lp.nseg) s.st_fef = cuts(kFarT, c1 + c2, s.st_fcut);
    for (int l = lp.n - 1; l >= 0; --l) {
        s.st_cut[l].clear();
        s.st_ef[l] = 512;
        if (stag_level(lp, l)) s.st_ef[l] = cuts(lp.T[l], col * toep_rows(lp.a[l], lp.b[l], lp.T[l]) * G / lp.T[l], s.st_cut[l]);
    }
    if (loads) {  // predicted background bytes per group over the far window, from the integer cuts
        const int cyc = kFarT / G;
        loads->assign(size_t(cyc), 0.0);
        for (int g = 0; g < cyc; ++g) {
            double& L = (*loads)[size_t(g)];
            for (int l = 0; l < lp.n; ++l) {
                const double wb = col * toep_rows(lp.a[l], lp.b[l], lp.T[l]);
                if (stag_level(lp, l)) {
                    const int k = g % (lp.T[l] / G);
                    L += wb * (s.st_cut[l][size_t(k) + 1] - s.st_cut[l][size_t(k)]);
                } else if (!block_level(s, lp.T[l])) {  // aligned: equal parts at the window's groups 1 .. T / G - 1
                    const int Tg = lp.T[l] / G, j = ((g * G + part_phi(lp.T[l], G, true)) % lp.T[l]) / G;
                    if (j >= 1) L += wb * C / (Tg - 1);
                }
            }
            if (lp.nseg) {
                const int k2 = g % cyc, k1 = (g + 2) % cyc;
                L += c2 * kFarT / G * (s.st_fcut[size_t(k2) + 1] - s.st_fcut[size_t(k2)]);
                L += c1 * kFarT / G * (s.st_fcut[size_t(k1) + 1] - s.st_fcut[size_t(k1)]);
            }
        }
    }
}

// the plan of a handle's background work (when the levels prime, and the plan exports): window
// offsets, part cuts, far slices, classes; loads: the predicted background bytes per group
inline void plan_parts(level_sched& s, std::vector<double>* loads = nullptr, bool balance = true)
{
    const level_plan& lp = s.lv;
    part_level pl[kLvToep];
    const double CB = double(s.C) * s.B;
    for (int l = 0; l < lp.n; ++l) {
        int JH, UPW;
        toep_geom(s, lp.T[l], JH, UPW);
        pl[l].T = lp.T[l];
        pl[l].UPW = UPW;
        pl[l].bg = s.sg > 1 && !s.persist && !block_level(s, lp.T[l]) && !stag_level(lp, l);  // latency mode: its own schedule
        pl[l].U = toep_units(s, lp.T[l]);
        pl[l].wbytes = CB * 8 * toep_rows(lp.a[l], lp.b[l], lp.T[l]);
    }
    const int ns = s.sg > 1 && !s.persist && lp.nseg && !lp.stag ? far_nslices(s) : 0;
    double c1 = 0, c2 = 0;  // bytes per far unit (16 columns) of phase 1 and 2 per window
    if (ns) {
        const int K = far_group(s);
        if (s.far_raw) {
            c2 = 16.0 * 8 * far_raw_rows(lp.nseg, s.P);
        } else {
            c1 = 16.0 * 8 * far1_rows(lp.nseg, K);  // stored spectra, partial sums out
            c2 = 16.0 * 8 * far2_rows(K);           // fresh pair, products, field, sums in
        }
    }
    part_plan(pl, lp.n, s.sg, far_units(s), ns, c1, c2, s.far_raw, balance, s.lv_phi, s.lv_cyc, s.lv_cut, s.fv_cut,
              lp.stag ? nullptr : loads);
    if (lp.stag) stag_classes(s, loads);
}

// ---------------------------------------------------------------------------------------
// The schedule of a convolver of C channels, blocks of B, P partitions with the options o (the
// create path and the plan exports): the far level's form, the step group, aligned or staggered
// windows, the FDL ring's rows. ring: the rows the caller's other paths need; raised to what the
// far level reads back. borrow: a convolver group's member; v2: sub-block input. Returns nullptr,
// or why the options cannot be had.
inline const char* make_level_sched(int C, int B, int P, int ring, const neo_hip_upols_opts& o, bool borrow, bool v2,
                                    level_sched& s)
{
    s = level_sched{};
    s.C = C;
    s.B = B;
    s.P = P;
    s.ring = ring;
    plan_levels(P, s.lv, o.far_level);
    s.far_k = o.far_group;
    s.toep_jh = o.toep_split;
    s.f2mode = o.far_phase2;
    s.sg = o.step_group ? o.step_group : step_group_for(C, B, P);
    // staggered level windows (plan_levels_stag): on request with any step group of 2, 4 or 8 and
    // the far level's stored form; automatic only from kStaggerUnits 16-column units with an
    // automatic step group, the one size measured to gain (c5full, 65536 units: 107.4 -> 99.4 us per
    // step; DESIGN 6, profiles/stagger_ab.json). Smaller handles and a group's members (borrow)
    // keep the aligned plan.
    const bool can = s.sg > 1 && o.far_level != 0 && o.far_level != 2 && !v2 && B <= 1024;
    if (o.windows == 2 && !can) return "staggered windows take step groups and the far level's stored form";
    if (o.windows == 2 || (o.windows == 0 && can && !o.step_group && !borrow && int64_t(C) * (B / 16) >= kStaggerUnits))
        plan_levels_stag(P, C, B, s.sg, o.far_group, s.lv);
    // the far level's form: the stored spectra (phase 1 + 2) by default; recomputed every window
    // (far2r_role) on request -- fewer bytes (C5: 15 instead of 23 rows per column and step) but
    // 2 nseg + 1 transforms per unit and window: same-box A/B with step groups, stored vs
    // recomputed, us per step: c5full 107-109 vs 115-124 (VALU), C5 15.9 vs 15.8-16.4, C4 12.4 vs
    // 18-20 (the 27-transform chain of 13 segments bounds the background launch)
    s.far_raw = s.lv.nseg && o.far_level == 2;
    if (s.lv.nseg) s.ring = std::max(s.ring, kFarRing);  // far slices read 383 blocks back
    // recomputed: a window's slices read the band's rows back to t_W - 128 (nseg + 2) > t_W - P - 128
    // while blocks up to t_W + 3 may be written beside them (step groups)
    if (s.far_raw) s.ring = std::max(s.ring, P + 2 * kFarT);
    return nullptr;
}

// neo_hip_upols_opts with every choice automatic, but the step group and the windows given
inline neo_hip_upols_opts plan_opts(int step_group, int windows, int far_group = 0)
{
    return neo_hip_upols_opts{-1, 0, 0, 0, -1, -1, far_group, 0, step_group, 0, windows};
}

// ---------------------------------------------------------------------------------------
// One helper per kind of role.

// A Toeplitz role: units [u0, u1) of level l's window whose first block is ring row tw, into the
// slab buffer buf. Slot l = level l (the kernel dispatches on it); empty slices allowed.
inline void toep_fill(const level_sched& s, int l, int buf, int tw, int64_t u0, int64_t u1, slice_args& a, level_sel& sel)
{
    const int T = s.lv.T[l];
    int JH, UPW;
    toep_geom(s, T, JH, UPW);
    toep_arg& ta = a.tp[l];
    ta.u0 = int(u0);
    ta.u1 = int(u1);
    sel.tp[l] = buf;
    ta.cs = slab_cs(T, s.B);
    ta.T = T;
    ta.a = s.lv.a[l];
    ta.b = s.lv.b[l];
    ta.tw = tw;
    ta.nwg = ta.u1 > ta.u0 ? (ta.u1 - ta.u0 + UPW - 1) / UPW : 0;
    ta.jh = JH;
    a.ntp = std::max(a.ntp, l + 1);
}

// far phase 1 over the slice units [u0, u1): mode 0 one window per group, 1 only the groups of
// class cls (K windows each), 2 every group (class cls: K windows; classes not started: one)
NEO_LV_HD inline void far1_range_k(slice_args& a, int u0, int u1, int mode, int cls, int K, int fpl)
{
    a.f1u0 = u0;
    a.f1u1 = u1;
    a.f1fpl = fpl;
    a.f1mode = mode;
    a.f1cls = cls;
    a.f1nwg = 0;
    if (u1 <= u0) return;
    const int ga = u0 / kF1UG, gb = (u1 - 1) / kF1UG;  // groups holding slice units
    a.f1g0 = mode == 1 ? ga + pmod(cls - ga % K, K) : ga;
    a.f1gs = mode == 1 ? K : 1;
    const int ng = a.f1g0 > gb ? 0 : (gb - a.f1g0) / a.f1gs + 1;
    a.f1nwg = ng * (kFN / (4 * fpl));
}

// far phase 1 of window W over the units [u0, u1): the unit groups of class W mod K for the
// windows W .. W + K - 1 (far1_mac); in the first windows after priming (W < K) the classes that
// have not started, for window W alone. prime: window 0, zero partial sums (no stored segments).
inline void far1_args(const level_sched& s, int64_t W, int u0, int u1, slice_args& a, bool prime = false)
{
    const int K = far_group(s);
    a.f1wn = int(W);
    far1_range_k(a, u0, u1, prime || K == 1 ? 0 : (W < K ? 2 : 1), prime ? 0 : int(W % K), K, far1_fpl(s));
}

// far phase 2a of window W over the units [u0, u1): the fresh row pair's transform (tw: the
// window's first block), stored to its slot
inline void far2a_fill(int u0, int u1, int64_t W, int tw, slice_args& a)
{
    a.f2u0 = u0;
    a.f2nwg = u1 - u0;
    a.f2tw = tw;
    a.f2wn = int(W);
}

// far phase 2 of window W over the units [u0, u1), into the field's buffer buf. comb 0: 2b alone
// (the products and the inverse; it reads no FDL row), 1: 2a and 2b in one workgroup per unit
// (far2c_role), 2: the recomputed form (far2r_role); tw: the window's first block, whose rows 1
// and 2 read. grp: units in window j of their phase-1 group take segments 1 .. j here.
inline void far2_fill(int u0, int u1, int64_t W, int buf, int comb, bool grp, int tw, slice_args& a, level_sel& sel)
{
    a.f3u0 = u0;
    a.f3nwg = u1 - u0;
    a.f3wn = int(W);
    a.f2grp = grp;
    sel.f3 = buf;
    if (comb) a.f2tw = tw;
    a.f2comb = comb;
}

// Latency mode's far level (persist_far): the far work of step n (block t0 + n, ring row w) in the
// one-launch schedule, with kFarT - 2 slices (one more step of slack: the field of window W is
// complete two steps before its first block, as the Toeplitz slabs): phase 1 of slice q and phase 2
// (far2c_role) of slice q - 1 of window W = n / kFarT + 1 at q = n mod kFarT. The kernel calls it
// too, so it fills the pointer itself.
NEO_LV_HD inline void persist_far_args(slice_args& a, int64_t n, int w, int U, int K, int fpl, cf* ff)
{
    constexpr int ns = kFarT - 2;
    const int64_t W = n / kFarT + 1;
    const int q = int(n % kFarT);
    a.f1nwg = a.f2nwg = a.f3nwg = 0;
    if (q < ns) {
        a.f1wn = int(W);
        far1_range_k(a, int(int64_t(q) * U / ns), int(int64_t(q + 1) * U / ns), K == 1 ? 0 : (W < K ? 2 : 1),
                     int(W % K), K, fpl);
    }
    if (q >= 1 && q <= ns) {
        a.f3u0 = int(int64_t(q - 1) * U / ns);
        a.f3nwg = int(int64_t(q) * U / ns) - a.f3u0;
        a.f3wn = int(W);
        a.f2grp = K > 1;
        a.f3ff = ff + (W & 1) * int64_t(a.C) * ff_cs(a.B);
        const int64_t t = (int64_t(w) + W * kFarT - n) % a.ring;
        a.f2tw = int(t < 0 ? t + a.ring : t);
        a.f2comb = 1;
    }
}

// ---------------------------------------------------------------------------------------
// The schedule.

// The block role of step n (block t0 + n): its slab row of every Toeplitz level and its far-field
// row (windows finished in earlier launches). Staggered levels: the block role picks buffer and
// row by the channel's class.
inline void block_rows(const level_sched& s, int64_t n, slice_args& a, level_sel& sel)
{
    const level_plan& lp = s.lv;
    a.a0 = lp.a0;
    if (lp.stag) {
        a.stag = lp.stag;
        a.sM = stag_mul(s);
        a.fef = s.st_fef;
        a.snm = int(n % (2 * kFarT));
    }
    for (int l = 0; l < lp.n; ++l) {
        const int T = lp.T[l];
        const int64_t m = n + s.lv_phi[l];  // window m / T, its row m mod T
        const bool st = stag_level(lp, l);
        a.ssh[a.nsl] = st ? log2i(kFarT / T) : -1;
        a.sef[a.nsl] = s.st_ef[l];
        sel.sl[a.nsl] = st ? 0 : int(m / T & 1);
        sel.sl_row[a.nsl] = st ? 0 : int(m % T);
        a.scs[a.nsl++] = slab_cs(T, s.B);
    }
    if (lp.nseg) {
        a.fsh = lp.stag ? 0 : -1;
        sel.ff = lp.stag ? 0 : int(n / kFarT & 1);
        sel.ff_row = lp.stag ? 0 : int(n % kFarT);
        a.fcs = ff_cs(s.B);
    }
}

// The slices the launch of step n (block t0 + n at ring row w) carries. G = 1: slice n mod T of
// window n / T + 1 of every Toeplitz level (its rows end before the window in progress, so every
// window's slabs are complete when its first block runs) and, with q = n mod 128 and W = n / 128 + 1,
// far phase 1 and 2a of slice q (q < 127) and far phase 2b of slice q - 1 (q >= 1) of window W.
// G > 1, block launches: the levels with T < 2 G, as for G = 1.
inline void block_levels(const level_sched& s, int64_t n, int w, slice_args& a, level_sel& sel)
{
    for (int l = 0; l < s.lv.n; ++l) {
        const int T = s.lv.T[l];
        if (s.sg > 1 && !block_level(s, T)) break;
        const int64_t U = toep_units(s, T), st = n % T, W = n / T + 1;
        toep_fill(s, l, int(W & 1), ring_add(w, W * T - n, s.ring), st * U / T, (st + 1) * U / T, a, sel);
    }
    if (s.sg > 1 || !s.lv.nseg) return;
    const int64_t U = far_units(s), W = n / kFarT + 1;
    const int q = int(n % kFarT), ns = far_nslices(s), tw = ring_add(w, W * kFarT - n, s.ring);
    const bool grp = far_group(s) > 1;
    if (s.far_raw) {  // recomputed: slice q - 1 of window W whole (far2r_role)
        if (q >= 1 && q <= ns) far2_fill(far_cut(s, q - 1), far_cut(s, q), W, int(W & 1), 2, false, tw, a, sel);
    } else if (far2_whole(s)) {  // phase 1 of slice q, phase 2 (far2c_role) of slice q - 1
        if (q < ns) far1_args(s, W, far_cut(s, q), far_cut(s, q + 1), a);
        if (q >= 1 && q <= ns) far2_fill(far_u(U, q - 1, ns), far_u(U, q, ns), W, int(W & 1), 1, grp, tw, a, sel);
    } else {  // phase 1 and 2a of slice q, 2b of slice q - 1
        if (q < ns) {
            far2a_fill(far_u(U, q, ns), far_u(U, q + 1, ns), W, tw, a);
            far1_args(s, W, far_cut(s, q), far_cut(s, q + 1), a);
        }
        if (q >= 1) far2_fill(far_u(U, q - 1, ns), far_u(U, q, ns), W, int(W & 1), 0, grp, tw, a, sel);
    }
}

// G > 1: the background launch issued at step n0 (a multiple of G; block t0 + n0 at ring row w0).
// It may read only the blocks before n0 - G (it waits for those, not for the group before it), and
// the block launch of step n0 + G waits for it. So a level of window T >= 2 G computes window W + 1
// in T / G - 1 parts at the steps t_W + G j, j = 1 .. T / G - 1 (part j - 1; its rows end at t_W - 1),
// the last due one group before t_{W+1}; the far level's slice q (kFarT / G - 2 of them) runs
// phase 1 at group q + 1 and phase 2 (2a and 2b in one workgroup) at group q + 2 of the window before.
// Staggered windows (plan_levels_stag): the launch of group g = n0 / G carries class g mod T / G of
// every staggered level, whole, for the window starting at s = n0 + 2 G; of the far level phase 2
// of class g mod 128 / G for its window starting at s and phase 1 of the class after the next, whose
// window starts two groups later (a class's two phases in groups of one parity). n0 < 0: the
// launches before step 0 that priming replays -- only the staggered roles, and only windows that
// start after step 0.
inline void slice_part(const level_sched& s, int64_t n0, int w0, slice_args& a, level_sel& sel)
{
    const level_plan& lp = s.lv;
    const int G = s.sg;
    const int64_t g = n0 / G;  // n0 is a multiple of G
    for (int l = 0; l < lp.n; ++l) {
        const int T = lp.T[l], Tg = T / G;
        if (block_level(s, T)) continue;  // in the block launches
        if (stag_level(lp, l)) {
            const int64_t st = n0 + 2 * G;
            if (st <= 0) continue;
            const int k = int(pmod<int64_t>(g, Tg)), phi = stag_phi(T, G, k);
            const int64_t upc = toep_units(s, T) / s.C, W = (st + phi) / T;  // units per channel
            toep_fill(s, l, int(W & 1), ring_add(w0, W * T - (n0 + phi), s.ring), s.st_cut[l][size_t(k)] * upc,
                      s.st_cut[l][size_t(k) + 1] * upc, a, sel);
            continue;
        }
        if (n0 < 0) continue;
        const int64_t m0 = n0 + s.lv_phi[l], j = (m0 % T) / G, W = m0 / T;  // group j of window W
        if (j < 1) continue;
        const int64_t gw = (W * T - s.lv_phi[l]) / G, cyc = s.lv_cyc;  // window W's first group
        const int k = int(pmod(gw, cyc) / Tg);
        const int* cut = s.lv_cut[l].data() + size_t(k) * size_t(Tg);  // the window's cuts [0, Tg)
        // tw from m0: block t_{W+1} = (W + 1) T - phi
        toep_fill(s, l, int((W + 1) & 1), ring_add(w0, (W + 1) * T - m0, s.ring), cut[j - 1], cut[j], a, sel);
    }
    if (!lp.nseg) return;
    const bool grp = far_group(s) > 1;
    if (stag_far(lp)) {
        const int nc = kFarT / G, gpc = s.B / 16;
        const int64_t s2 = n0 + 2 * G, s1 = n0 + 4 * G;
        if (s1 > 0) {  // phase 1 of the class whose phase 2 runs two launches later (the same group parity)
            const int k = int(pmod<int64_t>(g + 2, nc));
            far1_args(s, (s1 + stag_phi(kFarT, G, k)) / kFarT, s.st_fcut[size_t(k)] * gpc, s.st_fcut[size_t(k) + 1] * gpc, a);
        }
        if (s2 > 0) {  // phase 2, 2a and 2b in one workgroup per unit (far2c_role)
            const int k = int(pmod<int64_t>(g, nc));
            const int64_t W = (s2 + stag_phi(kFarT, G, k)) / kFarT;
            far2_fill(s.st_fcut[size_t(k)] * gpc, s.st_fcut[size_t(k) + 1] * gpc, W, int(W & 1), 1, grp,
                      ring_add(w0, 2 * G, s.ring), a, sel);
        }
        return;
    }
    const int64_t W = n0 / kFarT + 1;
    const int q = int(n0 % kFarT) / G, ns = far_nslices(s), tw = ring_add(w0, W * kFarT - n0, s.ring);
    if (s.far_raw) {  // recomputed: slice q - 2 of window W whole, at phase 2's time
        if (q >= 2 && q - 2 < ns) far2_fill(far_cut(s, q - 2), far_cut(s, q - 1), W, int(W & 1), 2, false, tw, a, sel);
        return;
    }
    if (q >= 1 && q <= ns) far1_args(s, W, far_cut(s, q - 1), far_cut(s, q), a);  // phase 1 of slice q - 1
    // phase 2 of slice q - 2, 2a and 2b in one workgroup per unit (far2c_role)
    if (q >= 2) far2_fill(far_cut(s, q - 2), far_cut(s, q - 1), W, int(W & 1), 1, grp, tw, a, sel);
}

// First streaming step after a reset / filter change / batched pass (block t0 at ring row w):
// window 0 of every level, the window that holds step 0, computed whole in rounds of two launches
// (a: the Toeplitz levels, far phase 1 and 2a with every segment transformed, or the recomputed
// field; f: far 2b, and window 1 of a level with an offset). One walk over (level, class): an
// aligned level, or far level, is one class of all its units whose window 0 began phi = lv_phi[l]
// steps ago, in round 0; of a level with an offset window 1 too, whole: its parts before step 0
// never ran (the rest run again). Class k of a staggered level began stag_phi steps ago, in round
// 1 + k. Every row read is before t0. After the rounds a staggered plan runs the background
// launches of the groups -3 .. -1 as they would have run (slice_part: the windows that start at
// steps G .. 3 G, far phase 1 two groups before phase 2).
inline int prime_rounds(const level_sched& s)
{
    const level_plan& lp = s.lv;
    if (!lp.stag) return 1;
    return 1 + (lp.nseg ? kFarT / lp.stag : (lp.n ? lp.T[lp.n - 1] / lp.stag : 0));
}

inline void prime_round(const level_sched& s, int r, int w, slice_args& a, level_sel& sa, slice_args& f, level_sel& sf)
{
    const level_plan& lp = s.lv;
    const int G = lp.stag, k = r - 1;  // the staggered class of rounds >= 1
    for (int l = 0; l < lp.n; ++l) {
        const int T = lp.T[l];
        if (stag_level(lp, l) ? (r == 0 || k >= T / G) : r != 0) continue;
        const int64_t upc = toep_units(s, T) / s.C;
        const bool st = stag_level(lp, l);
        const int phi = st ? stag_phi(T, G, k) : s.lv_phi[l];
        const int64_t u0 = st ? s.st_cut[l][size_t(k)] * upc : 0, u1 = st ? s.st_cut[l][size_t(k) + 1] * upc : s.C * upc;
        toep_fill(s, l, 0, ring_add(w, -phi, s.ring), u0, u1, a, sa);
        if (!st && phi) toep_fill(s, l, 1, ring_add(w, T - phi, s.ring), u0, u1, f, sf);
    }
    if (!lp.nseg || (stag_far(lp) ? r == 0 : r != 0)) return;
    const int gpc = s.B / 16;
    const int u0 = stag_far(lp) ? s.st_fcut[size_t(k)] * gpc : 0;
    const int u1 = stag_far(lp) ? s.st_fcut[size_t(k) + 1] * gpc : int(far_units(s));
    const int tw = ring_add(w, stag_far(lp) ? -stag_phi(kFarT, G, k) : 0, s.ring);
    if (s.far_raw) {
        far2_fill(u0, u1, 0, 0, 2, false, tw, a, sa);
    } else if (u1 > u0) {
        a.fnfresh = f.fnfresh = lp.nseg;  // every segment transformed
        far1_args(s, 0, u0, u1, a, true);
        far2a_fill(u0, u1, 0, tw, a);
        far2_fill(u0, u1, 0, 0, 0, false, tw, f, sf);
    }
}

}  // namespace neo_hip
