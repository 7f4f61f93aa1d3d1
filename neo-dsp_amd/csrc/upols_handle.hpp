// upols_handle.hpp — the UPOLS convolver handle (neo_hip_upols) and the host helpers
// shared by the translation units that implement it (upols.hip, upols_batch.hip,
// upols_setup.hip, upols_levels.hip).
//   the latency mode's mailbox and device helpers
//   neo_hip_upols: the handle. Its shape plan is an upols_shape (upols_plan.hpp, host only: the
//       create calls' checks, the split, cache and ring rules and their constants), which holds
//       the level schedule (level_sched, levels_plan.hpp); the handle adds buffers and state
//   what the translation units share: launches, setup helpers, the streaming levels' entry points
#pragma once

#include "common.hpp"
#include "upols_plan.hpp"

#include <cstdint>
#include <deque>
#include <utility>
#include <vector>

namespace neo_hip {
// Latency mode (neo_hip_upols_set_persistent, upols_levels.hip): one persistent kernel per handle
// polls a mailbox in mapped host memory. Step n's record (device addresses of its input and
// output blocks) goes to slot n mod kPsRing; both words carry the slot's lap tag in their low 4
// bits (the blocks are 16-B aligned), so a record read while the host rewrites it shows two
// different tags and is read again.
constexpr int kPsRing = 64;
__host__ __device__ inline uint64_t ps_tag(int64_t n) { return uint64_t((n / kPsRing) % 15 + 1); }
struct persist_rec {
    uint64_t in, out;
};
struct persist_mb {
    persist_rec rec[kPsRing];
    int64_t done;   // kernel -> host: steps completed (n + 1 of the last one)
    int32_t stop;   // host -> kernel: leave
    int32_t alive;  // kernel -> host: 0 once the kernel leaves (stop, idle timeout, error)
    int32_t err;    // kernel -> host: a wait passed its deadline
    int32_t pad;
};

// What both persistent kernels (k_lvl_persist, upols_levels.hip; k_plain_persist, upols.hip) share:
// the mailbox, the device flags (kPsFlag*), the step times, the idle limit and the deadline.
struct persist_ctl {
    persist_mb* mb;                 // the mapped mailbox (device address)
    int64_t* flags;                 // blk_done, quit, arrivals, records, sl_done (kPsFlag*)
    unsigned long long* tl;         // [kPsRing][2] record seen / done
    long long idle_ticks, dead_ticks;
    int64_t n0;                     // first step of this launch
    int w0;                         // its ring row
};
// device flags of the persistent kernels (int64 words): blk_done, quit, the per-step arrival
// counters of the block workgroups (a ring: a channel may run up to three steps ahead of another),
// the last step whose record block workgroup 0 handed on and those records (a ring), then
// sl_done per slice workgroup
constexpr int kPsArr = 8;
constexpr int kPsFlagArrive = 2, kPsFlagArriveFdl = kPsFlagArrive + kPsArr, kPsFlagGo = kPsFlagArriveFdl + kPsArr;
constexpr int kPsFlagIo = kPsFlagGo + 1;
constexpr int kPsFlagSlices = kPsFlagIo + 2 * kPsArr;

__device__ __forceinline__ int64_t ps_ld(const int64_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ps_st(int64_t* p, int64_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ps_acquire()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// thread 0: wait until cond() (quit and the deadline checked every round); false = leave
template<class F>
__device__ __forceinline__ bool ps_wait(const persist_ctl& pc, F cond)
{
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        if (cond()) return true;
        if (ps_ld(pc.flags + 1)) return false;
        if ((long long)(wall_clock64() - t0) > pc.dead_ticks) {
            __hip_atomic_store(&pc.mb->err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            ps_st(pc.flags + 1, 1);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// thread 0 of a block workgroup, ok = its own waits passed: step n's record into io[2]. Workgroup 0
// (lead) polls the mailbox slot (both words tagged with the step's lap; the host's stop, quit and
// the idle limit checked every 16th poll) and, with more than one block workgroup (share), hands
// the record on through the flags; the others wait for it there. false = leave.
__device__ __forceinline__ bool ps_record(const persist_ctl& pc, int64_t n, bool lead, bool share, bool ok,
                                          uint64_t* io, unsigned long long& t_seen)
{
    if (lead) {
        const int slot = int(n % kPsRing);
        const uint64_t tag = ps_tag(n);
        const unsigned long long t0 = wall_clock64();
        for (unsigned it = 0; ok; ++it) {
            const uint64_t r0 = __hip_atomic_load(&pc.mb->rec[slot].in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const uint64_t r1 = __hip_atomic_load(&pc.mb->rec[slot].out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((r0 & 15) == tag && (r1 & 15) == tag) {
                io[0] = r0 & ~uint64_t(15);
                io[1] = r1 & ~uint64_t(15);
                t_seen = wall_clock64();
                if (share) {
                    int64_t* r = pc.flags + kPsFlagIo + 2 * (n % kPsArr);
                    ps_st(r, int64_t(io[0]));
                    ps_st(r + 1, int64_t(io[1]));
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    ps_st(pc.flags + kPsFlagGo, n);
                }
                return true;
            }
            if ((it & 15) == 15 &&
                (__hip_atomic_load(&pc.mb->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) || ps_ld(pc.flags + 1) ||
                 (long long)(wall_clock64() - t0) > pc.idle_ticks)) {
                ps_st(pc.flags + 1, 1);
                return false;
            }
        }
        return false;
    }
    if (!ok || !ps_wait(pc, [&] { return ps_ld(pc.flags + kPsFlagGo) >= n; })) return false;
    ps_acquire();
    const int64_t* r = pc.flags + kPsFlagIo + 2 * (n % kPsArr);
    io[0] = uint64_t(ps_ld(r));
    io[1] = uint64_t(ps_ld(r + 1));
    return true;
}

// One bank of a sparse handle's filter (sparse_plan.hpp): the fixed-size tables, the compacted tiles
// (sized by the filter's kept tiles; null while none is kept) and the counts that came back from
// the device. The handle's current bank is its sp_* members; the spare one (a live update's) is sp2.
struct sparse_bank {
    uint32_t *bits = nullptr, *win = nullptr, *off = nullptr;
    int64_t* base = nullptr;
    cf* val = nullptr;
    int64_t tiles = 0, bins = 0, wtiles = 0;
};

}  // namespace neo_hip

struct neo_hip_upols {
    // the plan (upols_plan.hpp): splits, cache rows, strides, which paths are on, and in its level
    // schedule (levels_plan.hpp) the shape C, B, P and the FDL ring's rows
    neo_hip::upols_shape shape;
    neo_hip::level_sched& sched = shape.sched;
    int &C = sched.C, &B = sched.B, &P = sched.P, &ring = sched.ring;
    neo_hip_upols() = default;
    neo_hip_upols(const neo_hip_upols&) = delete;  // the references above
    neo_hip_upols& operator=(const neo_hip_upols&) = delete;
    int device = 0;
    hipStream_t stream = nullptr;
    neo_hip::cf* H = nullptr;
    neo_hip::cf* fdl = nullptr;
    neo_hip::cf* part = nullptr;
    float* prev = nullptr;
    int* arrivals = nullptr;  // per-channel split arrival counters (zero between steps)
    int wpos = 0;             // FDL write position (fdl_index.hpp:35-37), host-side
    neo_hip::cf* tw = nullptr;
    float* io = nullptr;       // device staging for host-pointer process()
    float* io_host = nullptr;  // pinned staging
    neo_hip::cf* part_b = nullptr;   // batched partial spectra [C][Sb][T][B]
    // streaming levels (upols_levels.hip; on: shape.ahead)
    int64_t lv_n = -1;              // blocks since the levels were primed (-1: prime at the next step)
    bool fdl_zero = false;          // FDL ring all zero, nothing stepped since (reset_state): every level
                                    // window the prime computes is zero, so priming is zeroing
    bool grouped = false;           // created by a convolver group (create_handle): no eager priming
    bool lv_ready = false;          // level buffers allocated
    neo_hip::cf* lv_slab[neo_hip::kLvToep] = {};  // Toeplitz level slabs [2][C][T][B]
    neo_hip::cf* fv_hf = nullptr;   // far segment spectra [C][nseg][256][B]
    neo_hip::cf* fv_xf = nullptr;   // far FDL row-pair spectra, ring of nseg slots [C][nseg][256][B]
    neo_hip::cf* fv_ff = nullptr;   // far field [2][C][128][B]
    neo_hip::cf* fv_tw = nullptr;   // 256-point twiddles
    neo_hip::cf* fv_acc = nullptr;  // far phase-1 partial sums [K][units][256][16] (K = far_group)
    bool fv_dirty = true;           // far segment spectra to recompute (filter changed)
    // step groups (sched.sg > 1): the level slices of G steps run as one launch on the handle's
    // background stream bg, one step group ahead (events ev_blk / ev_sl order the two; upols_levels.hip)
    int bg_pad = 0;  // dynamic LDS bytes of the slices launches (bg_pad_for): 1024 holds them to 2 workgroups per CU
    hipStream_t bg = nullptr;
    hipEvent_t ev_blk = nullptr, ev_sl[2] = {}, ev_join = nullptr;
    int paced = 0;                 // neo_hip_upols_set_paced: the group's background launch in G per-call pieces
                                   // (1) or in two pieces, at the group's calls 0 and G / 2 (2)
    bool pace_prev = false;        // a piece was issued before (its event ev_pc[(pace_seq - 1) & 1])
    int64_t pace_seq = 0;          // pieces issued since the levels primed
    hipEvent_t ev_pc[2] = {};
    bool bg_busy = false;  // slices enqueued on bg since the last join
    int64_t bg_launches = 0;
    float* tail = nullptr;  // batched OLA tails [C][T][B]
    // offline windows (k_off_mac, launch_offline; on: shape.off)
    neo_hip::cf* off_hf = nullptr;   // the filter's segment spectra [C][shape.off_nseg][256][B]
    bool off_dirty = true;           // off_hf to recompute (filter changed)
    neo_hip::cf* off_y = nullptr;    // a pass's output spectra [C][128 kOffMaxWP][B]
    float* off_tail = nullptr;       // OLA: a pass's tails [C][128 kOffMaxWP][B]
    // live filter updates (neo_hip_upols_update_filter; upols_fade.hip): from the first update on
    neo_hip::cf* H_alloc = nullptr;  // the allocation H and the FDL were made in (H may be the other bank by now)
    neo_hip::cf* H2 = nullptr;       // the spare bank [C][ring][B], the handle's own strides: bank B while a fade runs
    neo_hip::cf* part_f = nullptr;   // [C][fade_S][2][B] the fade step's slabs
    float* ovl2 = nullptr;           // overlap-add: bank B's tails [C][B]
    int fade_S = 1, fade_rows = 1;   // the fade step's splits (upols_fade_split)
    int fade_left = 0, fade_total = 0, fade_curve = 0;  // blocks left of the running fade (0: none)
    bool has_filter = false;         // a filter call succeeded (an update needs a filter to fade from)
    float* samples_dev = nullptr;   // process_samples host staging (device side)
    float* samples_host = nullptr;  // process_samples host staging (pinned)
    size_t samples_cap = 0;
    int timing = 0;          // 0: off; n: HIP events around every n-th launch group
    int64_t tick = 0;        // launch groups seen while timing
    bool ola = false;  // upola_convolver (overlap-add stage) instead of upols (overlap-save)
    bool v2 = false;   // upola_convolver_v2: sub-block input (implies ola)
    int in_pos = 0;    // v2: samples of the current block already consumed (_input_pos)
    float* window = nullptr;  // v2: real window [C][2B]
    neo_hip::cf* tmp = nullptr;        // v2: tail accumulator [C][B] packed (_tmp_accumulator)
    // sparse handle (neo_hip_upols_create_sparse, upols_sparse.hip; format: sparse_plan.hpp): no
    // dense filter (H stays null, the FDL is an allocation of its own), no levels or offline
    // windows; a block is one k_upols_sparse_step, or with batching on (off by default) T blocks
    // share one k_sparse_batch_mac pass over the kept tiles (upols_sparse_batch.hip)
    bool sparse = false;
    uint32_t* sp_bits = nullptr;   // kept-tile bitmaps [C][P][NW]
    uint32_t* sp_off = nullptr;    // row offsets [C][P + 1], tile units within the channel
    int64_t* sp_base = nullptr;    // [C + 2]: channel c's first tile, the total at [C]; kept columns at [C + 1]
    neo_hip::cf* sp_val = nullptr; // compacted tiles [kept tiles][16] (null until a filter is set, or none kept)
    int64_t sp_tiles = 0, sp_bins = 0;
    uint32_t* sp_win = nullptr;    // window bitmaps [C][P][NW]: the OR of rows [p, min(P, p + kMaxBatch)) of sp_bits
    int64_t sp_wtiles = 0;         // their popcount sum
    // live updates of a sparse handle (upols_sparse_fade.hip): the spare bank, bank B while a fade
    // runs and the retired filter after it. Its tables come with the first update and stay; its
    // tiles are allocated per update and go back to the pool at the next wait that covers the last
    // step that read them (the next update's wait for the counts, a resetting call's join, destroy).
    // part_f, ovl2 and the fade_* members above are shared with the dense handles' fades.
    neo_hip::sparse_bank sp2;
    struct ev_group {
        hipEvent_t e[4] = {};
        int n = 0;
        int part = 0;  // first part index its intervals add to (1: a step group's slice launch on bg)
    };
    std::deque<ev_group> events;   // pool, reused across timing windows (stable addresses while growing)
    size_t events_used = 0;
    double part_ms[4] = {};        // drained event time per part (see neo_hip_upols_timing_detail)
    int64_t part_n[4] = {};
    std::vector<float> group_ms;   // whole-group durations, in order (neo_hip_upols_step_times)
    // latency mode (neo_hip_upols_set_persistent): a persistent step kernel on ps_stream
    // (requested: sched.persist)
    bool ps_running = false;       // a persistent kernel was launched and not yet joined
    bool ps_valid = false;         // the level slabs follow the persistent schedule (relaunch without priming)
    hipStream_t ps_stream = nullptr;
    neo_hip::persist_mb* ps_mb = nullptr;      // mapped pinned mailbox (host address)
    neo_hip::persist_mb* ps_mb_dev = nullptr;  // its device address
    int64_t* ps_flags = nullptr;               // device: blk_done, quit, arrive, sl_done[]
    unsigned long long* ps_tl = nullptr;       // device: per ring slot {record seen, done} (wall clock, 100 MHz)
    int ps_nslices = 0;                        // slice workgroups of the persistent kernel
    int64_t ps_ld_in = 0, ps_ld_out = 0;       // channel strides of the running kernel
    int64_t ps_n0 = 0;                         // first step of the running kernel
    int64_t ps_launches = 0;                   // persistent launches so far (idle timeouts relaunch)
    int ps_wgs = 0;                            // workgroups of the running kernel (resident_admit)
    int64_t ps_fallbacks = 0;                  // calls run as normal steps: no room for the grid
    double ps_idle_ms = 50.0;                  // the kernel leaves after this long without a block
    // streams the step calls ran on since the last setup call (setup_join waits for these, not for
    // the device: another handle's resident latency-mode kernel must not stall a setup call); a
    // stream given to a step call must stay valid until the handle's next setup call or destroy
    neo_hip::stream_set used;
};


namespace neo_hip {

using upols_t = neo_hip_upols;

inline int note_stream(upols_t* h, hipStream_t s) { return h->used.note(s); }
// order a setup call (filter change, reset, mode switch, destroy) after every step of this handle:
// the streams its step calls ran on, its background stream, its own stream; device_input: also
// after work on the null stream (a device-resident filter or impulse produced there)
int setup_join(upols_t* h, bool device_input = false);

// The body is variadic on purpose. NEO_UPOLS_DISPATCH_OLA hands its BODY on to this macro, and a macro
// argument is expanded before it is handed on: a hipLaunchKernelGGL(...) in it has by then become
// kernel<<<grid, block, shmem, stream>>>(args), whose commas inside <<< >>> no parenthesis protects.
// A single named parameter would take them for argument separators.
#define NEO_UPOLS_DISPATCH(B_, ...) \
    switch (B_) {                   \
        case 16: { constexpr int BB = 16; __VA_ARGS__; break; }     \
        case 32: { constexpr int BB = 32; __VA_ARGS__; break; }     \
        case 64: { constexpr int BB = 64; __VA_ARGS__; break; }     \
        case 128: { constexpr int BB = 128; __VA_ARGS__; break; }   \
        case 256: { constexpr int BB = 256; __VA_ARGS__; break; }   \
        case 512: { constexpr int BB = 512; __VA_ARGS__; break; }   \
        case 1024: { constexpr int BB = 1024; __VA_ARGS__; break; } \
        case 2048: { constexpr int BB = 2048; __VA_ARGS__; break; } \
        case 4096: { constexpr int BB = 4096; __VA_ARGS__; break; } \
        default: return fail(NEO_HIP_EINVAL, "unsupported block size %d", B_); \
    }
// the same for a kernel with an overlap-add build: BODY also sees a constexpr bool OL (= OLA_)
#define NEO_UPOLS_DISPATCH_OLA(B_, OLA_, BODY) \
    {                                          \
        if (OLA_) {                            \
            constexpr bool OL = true;          \
            NEO_UPOLS_DISPATCH(B_, BODY)       \
        } else {                               \
            constexpr bool OL = false;         \
            NEO_UPOLS_DISPATCH(B_, BODY)       \
        }                                      \
    }

inline int64_t partitions_for(int64_t L, int B)
{
    // stft.hpp:21-25 with overlap 0: idiv(L - B, B) + 1 (= ceil(L/B) for L >= B);
    // the reference underflows for L < B, we clamp to one partition.
    if (L <= B) return 1;
    return (L - B + B - 1) / B + 1;
}

inline int batch_blocks(const upols_t* h) { return batch_blocks(h->shape); }
// the FDL write position T blocks on (fdl_index.hpp:35-37)
inline void advance(upols_t* h, int T) { h->wpos = (h->wpos + T) % h->ring; }
// device I/O the kernels' 16-byte accesses can take: both bases aligned, strides multiples of 4 floats
inline bool io_aligned(const float* in, const float* out, int64_t ld_in, int64_t ld_out)
{
    return !((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) && !((ld_in | ld_out) & 3);
}

// a handle with default options whose setup and host-I/O work runs on `stream` (a group's; not
// destroyed with the handle) instead of one of the device's shared streams (upols.hip)
int create_handle(int channels, int block, int partitions, int device, int method, hipStream_t stream,
                  neo_hip_upols** out);
// upols_sparse.hip: the sparse handle's buffers (bitmaps, offsets; the FDL and the step state are
// the creator's), its filter (filter and mask [C][P][B + 1] on the device -> bitmaps, offsets and
// compacted tiles; one 24-byte copy back, h->stream joined) and its block step's MAC launch
// (k_upols_sparse_step; launch_step_normal runs the frame around it)
int sparse_alloc(upols_t* h);
void sparse_free(upols_t* h);
int sparse_set_filter(upols_t* h, const cf* filter, const uint8_t* mask, hipStream_t s);
// live updates (upols_sparse.hip): the handle's current bank as a value and back; the spare bank's
// tables, the fade step's slabs and overlap-add's second tails at the first update (on s);
// sparse_fill: the one packing path, a filter into bank b on s (the bank's old tiles freed and the new
// ones allocated after the wait on s for the three counts); the end of a fade (banks swap by
// pointer, pc / pcb follow the new tiles); the spare bank's tiles back to the pool (the caller
// joined every step that read them); what fade_info reports
inline sparse_bank sparse_cur(const upols_t* h)
{
    return {h->sp_bits, h->sp_win, h->sp_off, h->sp_base, h->sp_val, h->sp_tiles, h->sp_bins, h->sp_wtiles};
}
inline void sparse_put(upols_t* h, const sparse_bank& b)
{
    h->sp_bits = b.bits, h->sp_win = b.win, h->sp_off = b.off, h->sp_base = b.base, h->sp_val = b.val;
    h->sp_tiles = b.tiles, h->sp_bins = b.bins, h->sp_wtiles = b.wtiles;
}
int sparse_fill(upols_t* h, sparse_bank& b, const cf* filter, const uint8_t* mask, hipStream_t s);
int sparse_fade_buffers(upols_t* h, hipStream_t s);
void sparse_fade_swap(upols_t* h);
void sparse_release_spare(upols_t* h);
int64_t sparse_spare_bytes(const upols_t* h);
// upols_sparse_fade.hip: the MAC of a sparse handle's fade step: banks a, b (kept tiles only) against
// the FDL at write position w into the slabs h->part_f [C][S][2][B]; split 0 and prime as
// launch_upols_fade_mac. The finish is launch_matrix_fade_finish with O = C.
int launch_sparse_fade_mac(const upols_t* h, const sparse_bank& a, const sparse_bank& b, const float* in, int64_t ld_in,
                           int S, int rows, int w, bool prime, hipStream_t s);
int launch_sparse_mac(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s);
// upols_sparse_batch.hip: the MAC of a batched pass of a sparse handle (launch_batch, upols_batch.hip):
// T blocks at write position h->wpos into the slabs part_b [C][Sb][T][B], over the kept tiles
int launch_sparse_batch_mac(const upols_t* h, int T, hipStream_t s);
// perceptual.hip: mask [C][P][B + 1] of the perceptual predicate (perceptual_plan.hpp) for a device
// filter, on s. *tmp (pooled) and the host weights [B + 1] stay alive until s is joined.
int perceptual_mask_device(const cf* filter, int C, int B, int P, const neo_hip_perceptual* pp, const float* weights,
                           uint8_t* mask, float** tmp, hipStream_t s);
// upols.hip: the unfused step's second launch (k_upols_finish: slabs summed in order, c2r)
int launch_finish(upols_t* h, float* out, int64_t ld_out, hipStream_t s);
// the same launch on plain arguments (upols_matrix.hip: one "channel" per output): slabs part [C][S][B],
// ovl [C][B] the overlap-add tails (not read by overlap-save)
int launch_finish_slabs(int C, int B, int S, bool ola, const cf* part, float* out, int64_t ld_out, float* ovl,
                        const cf* tw, hipStream_t s);
// upols_batch.hip: T whole blocks in one pass over the filter and the FDL
int launch_batch(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, int T, hipStream_t s);
// the launches around a batched MAC on plain arguments (upols_matrix.hip: a matrix handle's window
// transforms run per input, its finish per output). Window: blocks 0..T-1 of C inputs into FDL rows
// (w + j) mod ring of [C][ring][B]; prev [C][B] is read (overlap-save), not written. Finish: slabs
// part [C][S][T][B] summed in order, c2r. With `in` (a dense or sparse handle's pass) overlap-save
// saves block T - 1 of it as prev [C][B]; without (a matrix handle's: the previous block is per
// input, the finish per output) it reads no input and saves nothing. Overlap-add then chains tail
// [C][T][B] and ovl [C][B] into out.
int launch_batch_window(int C, int B, int T, bool ola, const float* in, int64_t ld_in, const float* prev, cf* fdl,
                        const cf* tw, int ring, int w, hipStream_t s);
int launch_batch_finish(int C, int B, int S, int T, bool ola, const cf* part, const float* in, int64_t ld_in, float* out,
                        int64_t ld_out, float* prev, float* tail, float* ovl, const cf* tw, hipStream_t s);
// upols_matrix_batch.hip: the MAC of a batched pass of a matrix handle: T blocks at write position w
// into the slabs part [O][Sb][T][B]; tab is the batch plan's run_off and runs (matrix_plan.hpp)
int launch_matrix_batch_mac(const cf* H, const cf* fdl, cf* part, const int* tab, int B, int P, int ring, int O, int Sb,
                            int T, int w, hipStream_t s);
// upols_levels.hip: k_lvf_filter, the segment spectra hf [C][nseg][256][B] (channel stride
// lvf_spec_stride(nseg, B): one row more than the data) of the filter rows H + c cstride + p pstride,
// p = 128 (s + seg0) + r, zero past P
int launch_lvf_filter(const cf* H, cf* hf, const cf* tw, int C, int B, int P, int nseg, int64_t cstride, int64_t pstride,
                      int seg0, hipStream_t s);
int64_t lvf_spec_stride(int nseg, int B);
// upols_matrix_offline.hip: the transforms of an offline pass of a matrix handle, wp windows of 128
// blocks at write position w. fwd: the npairs = nseg + wp - 1 pairs of ring rows of every input
// (matrix_offline_pair_row, matrix_plan.hpp) -> xf [I][npairs][256][B]. mac: per output its routes
// (tab: the handle's route table, matrix_route_table in matrix_plan.hpp, uploaded once with the
// filter) x segments against hf, the inverse transforms -> y [O][128 wp][B], one slab of
// launch_batch_finish.
int launch_matrix_off_fwd(const cf* fdl, cf* xf, const cf* twf, int I, int B, int ring, int npairs, int wp, int w,
                          hipStream_t s);
int launch_matrix_off_mac(const cf* xf, const cf* hf, cf* y, const cf* twf, const int* tab, int O, int B, int nseg,
                          int wp, int64_t hcs, hipStream_t s);
// upols_matrix_fade.hip: the fade step of a live filter update of a matrix handle. mac: both banks
// HA, HB [nroutes][P][B] against the FDL at write position w into the slabs part [O][S][2][B] (tab:
// the same route table as launch_matrix_off_mac's; grid O x S x matrix_fade_chunks).
// finish: per output both banks' slabs summed in order, two c2r, out = a + g (b - a) for the samples
// n0 .. n0 + B - 1 of a fade of `total` samples; overlap-add keeps a tail per bank (ovl_a, ovl_b
// [O][B]). prime (overlap-add): bank B's transform alone, its second half into ovl_b, no output.
int matrix_fade_chunks(int B);
int launch_matrix_fade_mac(const cf* HA, const cf* HB, const cf* fdl, cf* part, const int* tab, int B, int P, int ring,
                           int O, int S, int w, hipStream_t s);
int launch_matrix_fade_finish(const cf* part, float* out, int64_t ld_out, float* ovl_a, float* ovl_b, const cf* tw, int B,
                              int O, int S, bool ola, bool prime, int64_t n0, int64_t total, int curve, hipStream_t s);
// upols_fade.hip: the MAC of a dense handle's fade step: banks HA, HB (the handle's layout) against
// the FDL at write position w into the slabs h->part_f [C][S][2][B]; split 0 runs the window r2c of
// `in`, inserts row w and (overlap-save) saves the previous block, as the plain step does. prime
// (overlap-add, at the update call): no window and no insert, p = 0 from ring row w. The finish is
// launch_matrix_fade_finish with O = C.
int launch_upols_fade_mac(const upols_t* h, const cf* HA, const cf* HB, const float* in, int64_t ld_in, int S, int rows, int w,
                          bool prime, hipStream_t s);
// upols_matrix_levels.hip: window levels of a matrix handle. mac: the workgroups [wg0, wg1) of a
// level's grid O x S x chunks (a part; none: no launch) for the window of T blocks whose block 0 is
// ring row w, over the level's run table tab (matrix_level_table, matrix_plan.hpp), into that
// window's slabs part [O][S][T][B]. finish: per output the head's slabs head [O][Sh][B] in order, then
// per level l < n the S[l] rows row[l] + ((o S[l] + s) T[l]) B, s ascending, then the c2r tail.
struct matrix_lvl_rows {
    const cf* row[5];  // kMatrixMaxLevels
    int S[5], T[5];
    int n;
};
int launch_matrix_lvl_mac(const cf* H, const cf* fdl, cf* part, const int* tab, int B, int P, int ring, int O, int S, int T,
                          int w, int wg0, int wg1, hipStream_t s);
int launch_matrix_lvl_finish(int O, int B, bool ola, const cf* head, int Sh, const matrix_lvl_rows& lv, float* out,
                             int64_t ld_out, float* ovl, const cf* tw, hipStream_t s);
// Timing (neo_hip_upols_set_timing): the next event group of nev events if this launch
// group is a timed one (every h->timing-th), else nullptr; mark(g, i, s) records event i.
inline int timing_begin(upols_t* h, int nev, upols_t::ev_group** out)
{
    *out = nullptr;
    if (!h->timing || h->tick++ % h->timing != 0) return NEO_HIP_OK;
    if (h->events_used == h->events.size()) {
        upols_t::ev_group g;
        for (auto& e : g.e) NEO_HIP_CHECK(hipEventCreate(&e));
        h->events.push_back(g);
    }
    *out = &h->events[h->events_used++];
    (*out)->n = nev;
    (*out)->part = 0;
    return NEO_HIP_OK;
}
inline int timing_mark(upols_t::ev_group* g, int i, hipStream_t s)
{
    if (g) NEO_HIP_CHECK(hipEventRecord(g->e[i], s));
    return NEO_HIP_OK;
}

// upols_levels.hip: one streaming block step (level slabs + the newest partitions) and 1/T
// of every level's next window; buffers; filter-change hook (the plan: levels_plan.hpp)
// (snap: also copy each channel's input block, as read, to snap [C][B])
int launch_levels(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s,
                  float* snap = nullptr);
// the block role of streaming step n (FDL ring row w) again for channel c alone, with another
// input block (upols_group.hip: a speculatively stepped channel whose caller's block differed);
// the step's slabs and far field must not have been overwritten since
int launch_block_only(upols_t* h, int64_t n, int w, int c, const float* in, float* out, hipStream_t s);
int bg_pad_for(int C, int B);
// latency mode: whole blocks through the persistent kernel, synchronous (upols_levels.hip)
int persist_process(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t nblocks);
// latency mode of a handle without streaming levels: the plain step's persistent kernel on
// h->ps_stream (upols.hip), its control (mailbox, flags, first step) set up by the caller
// (no room for its grid beside the process's other persistent kernels: *launched false, nothing
// enqueued, persist_room)
int plain_persist_launch(upols_t* h, const persist_ctl& ctl, int64_t ld_in, int64_t ld_out, bool* launched);
// room on the device for a persistent grid of `grid` workgroups of kernel f (256 lanes): all of them
// resident at once beside the persistent kernels this process already runs there, within three
// quarters of the device's slots for f (occupancy x CUs); reserved in h->ps_wgs on success
bool persist_room(upols_t* h, const void* f, int grid);
// the normal (non-persistent) block step (launch_step without the latency-mode branch)
int launch_step_normal(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, hipStream_t s);
// stop the persistent kernel (if any) and leave the levels to re-prime on the next normal step
int persist_stop(upols_t* h);
// why a handle cannot run the latency mode (nullptr: it can)
const char* persist_ineligible(const upols_t* h);
// order everything enqueued on the background stream (step-group slices) before later work on s;
// every path that writes the FDL ring or the level buffers other than a streaming step calls it
int lvl_join(upols_t* h, hipStream_t s);
void lvl_free(upols_t* h);
void lvl_filter_changed(upols_t* h);
// offline windows: the segment spectra (if the filter changed) and k_off_mac for wp windows of
// 128 blocks at h->wpos into h->off_y (buffers allocated by the caller, launch_offline)
int launch_off_mac(upols_t* h, int wp, hipStream_t s);
size_t off_hf_bytes(const upols_t* h);  // the offline windows' segment spectra (padded channel stride)
// upols_batch.hip: wp windows of 128 blocks of every channel in one pass (window r2c of every
// block, k_off_mac, per-block finish), h->wpos advanced
int launch_offline(upols_t* h, const float* in, int64_t ld_in, float* out, int64_t ld_out, int wp, hipStream_t s);
// a setup call's last step (set_filter, set_impulse, reset; FDL just zeroed): the level buffers,
// the far segment spectra and window 0 of every level, on h->stream, so the next call is an
// ordinary streaming step (no-op without levels and for group handles)
int lvl_setup_prime(upols_t* h);
// upols_setup.hip: twiddles, uniform_partition and normalize_impulse on the device
int upload_tw(cf** d, int B);
int partition_device(const float* d_ir, int C, int64_t L, int B, bool packed, cf* out, const cf* tw, hipStream_t s,
                     int64_t cstride = 0, int64_t pstride = 0);
int normalize_device(float* d_ir, int C, int64_t L, hipStream_t s);
// filter [C][P][B+1] (reference layout, device) -> packed H rows of the handle (bank: another bank
// of the handle's layout instead, a live update's)
int pack_filter(upols_t* h, const cf* src, hipStream_t s, cf* bank = nullptr);

}  // namespace neo_hip
