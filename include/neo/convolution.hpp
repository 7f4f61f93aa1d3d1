// SPDX-License-Identifier: MIT
// neo/convolution.hpp — neo::convolution UPOLS API on MI355X (gfx950).
//
// Same names and semantics as the reference's src/neo/convolution/*:
//   fdl_index                 fdl_index.hpp:12-41 (host ring bookkeeping)
//   uniform_partition         uniform_partition.hpp:12-26  -> [C][P][B+1] complex<float> (complex<double> for a double view)
//   normalize_impulse         normalize_impulse.hpp:11-33  (bit-exact rounding on the GPU; double views in double)
//   upols_convolver           dense_convolver.hpp:19-20 + uniform_partitioned_convolver.hpp:13-65
//   split_upols_convolver     dense_convolver.hpp:38-42 (same math; one device layout)
//   upola_convolver(_v2)      dense_convolver.hpp:23-28 (overlap_add / overlap_add_convolver)
// plus the GPU-shaped entry the plugin and CLI loops map onto: upols_multichannel,
// C channels stepped by one launch pair per block ([C][B] in, [C][P][B+1] filter),
// and dense_convolve (extra/plugin/src/dsp/DenseConvolution.hpp:39-70). upols_multichannel64 and
// std::complex<double> instances of upols_convolver / upola_convolver / split_*: the same in double.
#pragma once

#include <neo/fft.hpp>
#include <neo/hip/detail.hpp>
#include <neo/perceptual.hpp>

#include <algorithm>
#include <complex>
#include <concepts>
#include <cstddef>
#include <memory>
#include <span>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <map>
#include <mutex>
#include <array>
#include <utility>
#include <vector>

namespace neo::convolution {

/// method.hpp:8-17
enum struct method
{
    automatic,
    direct,
    fft,
    ola,
    ols,
    upola,
    upols,
};

/// mode.hpp:12-29 (only `full` has an output size, like the reference)
enum struct mode
{
    full,
    valid,
    same,
};

template<mode Mode, std::integral Int>
[[nodiscard]] constexpr auto output_size(Int signal, Int patch) -> Int
{
    static_assert(Mode == mode::full, "the reference defines output_size for mode::full only");
    return static_cast<Int>(signal + patch - Int(1));
}

/// fdl_index.hpp:12-41 — insert(write_pos), then for segment s: multiply(s, (write_pos + P - s) % P)
template<typename IndexType = std::size_t>
struct fdl_index {
    using value_type = IndexType;

    fdl_index() noexcept = default;
    explicit fdl_index(IndexType num_segments) : _num_segments{num_segments} {}

    auto reset() -> void { _write_pos = 0; }

    template<std::invocable<IndexType> CopyCallback, std::invocable<IndexType, IndexType> MultiplyCallback>
    auto operator()(CopyCallback copy_callback, MultiplyCallback callback) -> void
    {
        copy_callback(_write_pos);
        for (IndexType segment{0}; segment < _num_segments; ++segment) {
            callback(segment, static_cast<IndexType>((_write_pos + _num_segments - segment) % _num_segments));
        }
        if (++_write_pos; _write_pos >= _num_segments) reset();
    }

private:
    IndexType _num_segments{0};
    IndexType _write_pos{0};
};

/// P = ceil(L / B) (stft.hpp:21-25, overlap 0)
[[nodiscard]] inline auto num_partitions(std::size_t length, std::size_t block) -> std::size_t
{
    std::int64_t p = 0;
    neo::hip::check(neo_hip_num_partitions(std::int64_t(length), int(block), &p));
    return std::size_t(p);
}

namespace detail {
/// Float = InMat::value_type of the reference's free functions: double for a view of double,
/// float for everything else (as before double views existed here)
template<typename V>
struct view_float {
    using type = float;
};
template<typename V>
    requires std::same_as<std::remove_cv_t<typename V::value_type>, double>
struct view_float<V> {
    using type = double;
};
template<typename V>
using view_float_t = typename view_float<V>::type;
}  // namespace detail

/// uniform_partition.hpp:12-26: impulse [C][L] -> [C][P][B+1] (computed on the GPU), in the view's
/// precision: a view of double gives complex<double>, computed in double
template<typename InMat>
    requires neo::hip::detail::matrix_like<InMat>
[[nodiscard]] auto uniform_partition(InMat impulse_response, std::size_t block_size)
    -> neo::hip::array<std::complex<detail::view_float_t<InMat>>, 3>
{
    using Float = detail::view_float_t<InMat>;
    auto const C = std::size_t(impulse_response.extent(0)), L = std::size_t(impulse_response.extent(1));
    std::vector<Float> ir(C * L);
    for (std::size_t c = 0; c < C; ++c)
        for (std::size_t i = 0; i < L; ++i) ir[c * L + i] = Float(neo::hip::detail::at(impulse_response, c, i));
    auto const P = num_partitions(L, block_size);
    neo::hip::array<std::complex<Float>, 3> out;
    out.buf.resize(C * P * (block_size + 1));
    out.ext[0] = C;
    out.ext[1] = P;
    out.ext[2] = block_size + 1;
    if constexpr (std::same_as<Float, double>)
        neo::hip::check(neo_hip_uniform_partition_f64(ir.data(), int(C), std::int64_t(L), int(block_size), out.data(), 0,
                                                      neo::hip::detail::default_device()));
    else
        neo::hip::check(neo_hip_uniform_partition(ir.data(), int(C), std::int64_t(L), int(block_size), out.data(), 0,
                                                  neo::hip::detail::default_device()));
    return out;
}

/// normalize_impulse.hpp:11-33 (rank 1: unit energy; rank 2: min factor over channels), in the
/// view's precision (a view of double: in double, written back as double)
template<typename Obj>
auto normalize_impulse(Obj obj) noexcept -> void
{
    using Float = detail::view_float_t<Obj>;
    std::size_t C = 1, L = 0;
    if constexpr (neo::hip::detail::matrix_like<Obj>) {
        C = std::size_t(obj.extent(0));
        L = std::size_t(obj.extent(1));
    } else {
        L = std::size_t(obj.extent(0));
    }
    if (C == 0 || L == 0) return;
    std::vector<Float> buf(C * L);
    for (std::size_t c = 0; c < C; ++c)
        for (std::size_t i = 0; i < L; ++i) {
            if constexpr (neo::hip::detail::matrix_like<Obj>) buf[c * L + i] = neo::hip::detail::at(obj, c, i);
            else buf[i] = neo::hip::detail::at(obj, i);
        }
    if constexpr (std::same_as<Float, double>)
        neo::hip::check_or_abort(neo_hip_normalize_impulse_f64(buf.data(), int(C), std::int64_t(L), 0,
                                                               neo::hip::detail::default_device()));
    else
        neo::hip::check_or_abort(neo_hip_normalize_impulse(buf.data(), int(C), std::int64_t(L), 0,
                                                           neo::hip::detail::default_device()));
    for (std::size_t c = 0; c < C; ++c)
        for (std::size_t i = 0; i < L; ++i) {
            if constexpr (neo::hip::detail::matrix_like<Obj>) neo::hip::detail::at(obj, c, i) = buf[c * L + i];
            else neo::hip::detail::at(obj, i) = buf[i];
        }
}

/// selects upola_convolver_v2 (overlap_add_convolver.hpp:20-136) in upols_multichannel
struct upola_v2_tag {};
inline constexpr upola_v2_tag upola_v2{};

/// selects a sparse handle (neo_hip_upols_create_sparse: sparse_upols_convolver /
/// sparse_upola_convolver, sparse_convolver.hpp:12-17) in upols_multichannel
struct sparse_tag {};
inline constexpr sparse_tag sparse{};

/// The plugin's sparsity rule (sparse_convolve, extra/plugin/src/dsp/DenseConvolution.cpp:110-170;
/// neo_hip_perceptual in neo_hip.h): keep a bin iff its level relative to its channel's strongest
/// bin plus its column's weight exceeds threshold_db. Argument errors throw std::invalid_argument
/// where it is used (the block size is known there): validate(block_size).
struct perceptual_sparsity {
    double sample_rate{48000.0};      ///< Hz, > 0
    float threshold_db{-40.0F};       ///< finite; the plugin passes -dynamicRange
    int low_bins_to_keep{0};          ///< 0 .. B: columns below it are always kept
    int weighting{1};                 ///< 1 = A-weighting, 0 = none

    [[nodiscard]] auto c_struct() const noexcept -> neo_hip_perceptual
    {
        return neo_hip_perceptual{sample_rate, threshold_db, low_bins_to_keep, weighting};
    }

    /// throws std::invalid_argument naming what is wrong for blocks of block_size
    auto validate(std::size_t block_size) const -> void
    {
        auto const p = c_struct();
        std::vector<float> w(std::min<std::size_t>(block_size, 4096) + 1);  // a larger block is refused
        if (neo_hip_perceptual_weights(block_size <= 4096 ? int(block_size) : -1, &p, w.data()) != NEO_HIP_OK)
            throw std::invalid_argument{std::string{"neo_hip: "} + neo_hip_last_error()};
    }
};

namespace detail {
struct upols_deleter {
    void operator()(neo_hip_upols* h) const noexcept { neo_hip_upols_destroy(h); }
};
using upols_ptr = std::unique_ptr<neo_hip_upols, upols_deleter>;
}  // namespace detail

/// The gain curve of a live filter update (matrix and dense convolvers): linear g = t, cosine
/// g = 0.5 - 0.5 cos(pi t), t = n / (fade_blocks B) (neo_hip_matrix_fade_gains).
enum class fade_curve : int { linear = 0, cosine = 1 };

/// What fade_info() of a convolver with live filter updates reports.
struct fade_desc {
    int remaining_blocks, fade_blocks;
    std::int64_t bank_bytes;  ///< the second filter bank, 0 until the first update
};

/// C independent uniformly-partitioned convolvers (UPOLS, or UPOLA with method::upola)
/// on one GPU, stepped together.
struct upols_multichannel {
    upols_multichannel(std::size_t channels, std::size_t block_size, std::size_t partitions,
                       int device = neo::hip::detail::default_device(), method m = method::upols)
        : _C{channels}, _B{block_size}, _P{partitions}
    {
        if (m != method::upols && m != method::upola)
            throw std::invalid_argument{"neo_hip: multichannel convolver supports method::upols and method::upola"};
        neo_hip_upols* h = nullptr;
        auto create = m == method::upols ? neo_hip_upols_create : neo_hip_upola_create;
        neo::hip::check(create(int(channels), int(block_size), int(partitions), device, &h));
        _h.reset(h);
    }

    /// C instances of upola_convolver_v2 (sub-block input through process())
    upols_multichannel(upola_v2_tag, std::size_t channels, std::size_t block_size, std::size_t partitions,
                       int device = neo::hip::detail::default_device())
        : _C{channels}, _B{block_size}, _P{partitions}
    {
        neo_hip_upols* h = nullptr;
        neo::hip::check(neo_hip_upola2_create(int(channels), int(block_size), int(partitions), device, &h));
        _h.reset(h);
    }

    /// C sparse convolvers (method::upols or method::upola): only the filter bins a mask keeps
    /// take part, kept as 128-byte tiles; filter_sparse() sets the filter (filter() and impulse()
    /// throw), and the latency mode, paced work and offline windows do not apply (they throw).
    /// One block per pass unless batch(true) turns the batched passes on.
    upols_multichannel(sparse_tag, std::size_t channels, std::size_t block_size, std::size_t partitions,
                       int device = neo::hip::detail::default_device(), method m = method::upols)
        : _C{channels}, _B{block_size}, _P{partitions}
    {
        if (m != method::upols && m != method::upola)
            throw std::invalid_argument{"neo_hip: sparse convolvers support method::upols and method::upola"};
        neo_hip_upols* h = nullptr;
        neo::hip::check(neo_hip_upols_create_sparse(int(channels), int(block_size), int(partitions), device,
                                                    m == method::upola ? 1 : 0, nullptr, &h));
        _h.reset(h);
    }

    /// filter [C][P][B+1] complex<float>, contiguous host memory; resets state
    auto filter(std::complex<float> const* partitions) -> void
    {
        neo::hip::check(neo_hip_upols_set_filter(_h.get(), partitions, 0));
    }
    /// sparse handles: filter [C][P][B+1] and mask [C][P][B+1] (nonzero = keep), contiguous host
    /// memory; resets state
    auto filter_sparse(std::complex<float> const* partitions, std::uint8_t const* mask) -> void
    {
        neo::hip::check(neo_hip_upols_set_filter_sparse(_h.get(), partitions, mask, 0));
    }
    /// sparse handles: filter [C][P][B+1] thinned by the plugin's rule, the mask made on the device
    auto filter_perceptual(std::complex<float> const* partitions, perceptual_sparsity const& sparsity) -> void
    {
        sparsity.validate(_B);
        auto const p = sparsity.c_struct();
        neo::hip::check(neo_hip_upols_set_filter_perceptual(_h.get(), partitions, &p, 0));
    }
    /// sparse handles: normalize_impulse (optional), uniform_partition, mask and tiles of
    /// ir [C][length], all on the GPU
    auto impulse_perceptual(float const* ir, std::size_t length, perceptual_sparsity const& sparsity,
                            bool normalize = true) -> void
    {
        sparsity.validate(_B);
        auto const p = sparsity.c_struct();
        neo::hip::check(neo_hip_upols_set_impulse_perceptual(_h.get(), ir, std::int64_t(length), normalize ? 1 : 0, &p, 0));
    }
    /// sparse handles: kept columns and kept 128-byte tiles of the current filter
    [[nodiscard]] auto sparse_kept() const -> std::pair<std::int64_t, std::int64_t>
    {
        std::int64_t bins = 0, tiles = 0;
        neo::hip::check(neo_hip_upols_sparse_info(_h.get(), &bins, &tiles, nullptr));
        return {bins, tiles};
    }
    /// normalize_impulse (optional) + uniform_partition of ir [C][length] on the GPU
    auto impulse(float const* ir, std::size_t length, bool normalize = true) -> void
    {
        neo::hip::check(neo_hip_upols_set_impulse(_h.get(), ir, std::int64_t(length), normalize ? 1 : 0, 0));
    }
    /// one block for every channel, in place, io [C][B] host memory (synchronous)
    auto operator()(float* io) noexcept -> void { neo::hip::check_or_abort(neo_hip_upols_process(_h.get(), io, 0, nullptr)); }
    /// one block, device pointers, channel c at in + c*ld_in (asynchronous on stream)
    auto process_device(float const* in, std::size_t ld_in, float* out, std::size_t ld_out, void* stream = nullptr) -> void
    {
        neo::hip::check(neo_hip_upols_process_device(_h.get(), in, std::int64_t(ld_in), out, std::int64_t(ld_out), stream));
    }
    /// num_samples per channel, in place, io [C][num_samples] host memory (synchronous);
    /// any count for upola_v2, whole blocks otherwise (overlap_add_convolver.hpp:80-134)
    auto process(float* io, std::size_t num_samples) noexcept -> void
    {
        auto const n = std::int64_t(num_samples);
        neo::hip::check_or_abort(neo_hip_upols_process_samples(_h.get(), io, n, io, n, n, 0, nullptr));
    }
    /// process() that throws std::runtime_error on a device failure instead of aborting
    auto process_checked(float* io, std::size_t num_samples) -> void
    {
        auto const n = std::int64_t(num_samples);
        neo::hip::check(neo_hip_upols_process_samples(_h.get(), io, n, io, n, n, 0, nullptr));
    }
    /// clears all state; a running fade (update_filter) completes: the new filter is the filter
    auto reset() -> void { neo::hip::check(neo_hip_upols_reset(_h.get())); }
    /// live update (neo_hip_upols_update_filter): crossfade to `partitions` ([C][P][B+1], host memory)
    /// over the next fade_blocks blocks and KEEP ALL STATE -- delay line, previous block, overlap
    /// tail; filter() remains the resetting call. Complete on return. Dense upols / upola handles
    /// outside the latency mode; throws otherwise, and while a fade still runs.
    auto update_filter(std::complex<float> const* partitions, int fade_blocks = 1, fade_curve curve = fade_curve::linear)
        -> void
    {
        neo::hip::check(neo_hip_upols_update_filter(_h.get(), partitions, 0, fade_blocks, int(curve), nullptr));
    }
    /// the same from ir [C][length] (host memory): normalize_impulse over its channels if `normalize`,
    /// then uniform_partition on the device into the second bank; keeps all state
    auto update_impulse(float const* ir, std::size_t length, bool normalize = true, int fade_blocks = 1,
                        fade_curve curve = fade_curve::linear) -> void
    {
        neo::hip::check(neo_hip_upols_update_impulse(_h.get(), ir, std::int64_t(length), normalize ? 1 : 0, 0, fade_blocks,
                                                     int(curve), nullptr));
    }
    /// sparse handles: live update (neo_hip_upols_update_filter_sparse) to `partitions` under `mask`
    /// ([C][P][B+1] each, host memory), keeping all state; filter_sparse() remains the resetting call.
    /// Complete on return; throws on a handle that is not sparse and while a fade still runs.
    auto update_filter_sparse(std::complex<float> const* partitions, std::uint8_t const* mask, int fade_blocks = 1,
                              fade_curve curve = fade_curve::linear) -> void
    {
        neo::hip::check(neo_hip_upols_update_filter_sparse(_h.get(), partitions, mask, 0, fade_blocks, int(curve), nullptr));
    }
    /// the same with the mask made on the device by the plugin's rule (the threshold knob)
    auto update_filter_perceptual(std::complex<float> const* partitions, perceptual_sparsity const& sparsity,
                                  int fade_blocks = 1, fade_curve curve = fade_curve::linear) -> void
    {
        sparsity.validate(_B);
        auto const p = sparsity.c_struct();
        neo::hip::check(neo_hip_upols_update_filter_perceptual(_h.get(), partitions, &p, 0, fade_blocks, int(curve), nullptr));
    }
    /// and from ir [C][length] (another impulse response while audio runs): normalize_impulse
    /// (optional), uniform_partition, mask and tiles on the GPU; keeps all state
    auto update_impulse_perceptual(float const* ir, std::size_t length, perceptual_sparsity const& sparsity,
                                   bool normalize = true, int fade_blocks = 1, fade_curve curve = fade_curve::linear) -> void
    {
        sparsity.validate(_B);
        auto const p = sparsity.c_struct();
        neo::hip::check(neo_hip_upols_update_impulse_perceptual(_h.get(), ir, std::int64_t(length), normalize ? 1 : 0, &p, 0,
                                                                fade_blocks, int(curve), nullptr));
    }
    [[nodiscard]] auto fade_info() const -> fade_desc
    {
        fade_desc d{};
        neo::hip::check(neo_hip_upols_fade_info(_h.get(), &d.remaining_blocks, &d.fade_blocks, &d.bank_bytes));
        return d;
    }
    /// latency mode (neo_hip_upols_set_persistent): one resident kernel steps every block; every
    /// call completes on return (shapes up to 16 channels, 256 partitions, B <= 512; throws otherwise)
    auto latency_mode(bool on, double idle_ms = 50.0) -> void
    {
        neo::hip::check(neo_hip_upols_set_persistent(_h.get(), on ? 1 : 0, idle_ms));
    }
    /// paced background work (neo_hip_upols_set_paced): an even cost per call with step groups
    auto paced(bool on) -> void { neo::hip::check(neo_hip_upols_set_paced(_h.get(), on ? 1 : 0)); }
    /// the same with the group's background launch in two pieces (two cross-stream waits per group)
    auto paced_two_pieces() -> void { neo::hip::check(neo_hip_upols_set_paced(_h.get(), 2)); }
    /// offline windows for batched calls of >= 128 blocks (on by default from 128 partitions;
    /// neo_hip_upols_set_offline): 128-block windows through partition-axis transforms
    auto offline(bool on) -> void { neo::hip::check(neo_hip_upols_set_offline(_h.get(), on ? 1 : 0)); }
    /// batched passes (neo_hip_upols_set_batch): process() runs T blocks per pass over the filter
    /// and the FDL. On by default on dense handles, off on sparse ones.
    auto batch(bool on) -> void { neo::hip::check(neo_hip_upols_set_batch(_h.get(), on ? 1 : 0)); }

    [[nodiscard]] auto channels() const noexcept { return _C; }
    [[nodiscard]] auto block_size() const noexcept { return _B; }
    [[nodiscard]] auto partitions() const noexcept { return _P; }

private:
    std::size_t _C, _B, _P;
    detail::upols_ptr _h;
};

namespace detail {
struct upols64_deleter {
    void operator()(neo_hip_upols64* h) const noexcept { neo_hip_upols64_destroy(h); }
};
using upols64_ptr = std::unique_ptr<neo_hip_upols64, upols64_deleter>;
}  // namespace detail

/// upols_multichannel over double / std::complex<double> (neo_hip_upols64): C independent
/// upols_convolver<complex<double>> (or upola with method::upola) on one GPU, stepped together, one
/// launch pair per block. Whole blocks only; no live updates, latency mode or offline windows.
/// batch(true) turns batched passes on for calls of many blocks.
struct upols_multichannel64 {
    /// split_workgroups: the workgroups the MAC launch aims for (0: automatic)
    upols_multichannel64(std::size_t channels, std::size_t block_size, std::size_t partitions,
                         int device = neo::hip::detail::default_device(), method m = method::upols,
                         int split_workgroups = 0)
        : _C{channels}, _B{block_size}, _P{partitions}
    {
        if (m != method::upols && m != method::upola)
            throw std::invalid_argument{"neo_hip: multichannel convolver supports method::upols and method::upola"};
        neo_hip_upols64* h = nullptr;
        neo::hip::check(neo_hip_upols64_create(int(channels), int(block_size), int(partitions), device,
                                               m == method::upola ? 1 : 0, split_workgroups, &h));
        _h.reset(h);
    }

    /// filter [C][P][B+1] complex<double>, contiguous host memory; resets state
    auto filter(std::complex<double> const* partitions) -> void
    {
        neo::hip::check(neo_hip_upols64_set_filter(_h.get(), partitions, 0));
    }
    /// normalize_impulse (optional) + uniform_partition of ir [C][length] on the GPU, in double
    auto impulse(double const* ir, std::size_t length, bool normalize = true) -> void
    {
        neo::hip::check(neo_hip_upols64_set_impulse(_h.get(), ir, std::int64_t(length), normalize ? 1 : 0, 0));
    }
    /// one block for every channel, in place, io [C][B] host memory (synchronous)
    auto operator()(double* io) noexcept -> void
    {
        auto const n = std::int64_t(_B);
        neo::hip::check_or_abort(neo_hip_upols64_process_samples(_h.get(), io, n, io, n, n, 0, nullptr));
    }
    /// one block, device pointers, channel c at in + c*ld_in (strides in doubles, even;
    /// asynchronous on stream)
    auto process_device(double const* in, std::size_t ld_in, double* out, std::size_t ld_out, void* stream = nullptr) -> void
    {
        neo::hip::check(neo_hip_upols64_process_samples(_h.get(), in, std::int64_t(ld_in), out, std::int64_t(ld_out),
                                                        std::int64_t(_B), 1, stream));
    }
    /// num_samples (whole blocks) per channel, in place, io [C][num_samples] host memory (synchronous)
    auto process(double* io, std::size_t num_samples) noexcept -> void
    {
        auto const n = std::int64_t(num_samples);
        neo::hip::check_or_abort(neo_hip_upols64_process_samples(_h.get(), io, n, io, n, n, 0, nullptr));
    }
    /// process() that throws std::runtime_error on a refusal or device failure instead of aborting
    auto process_checked(double* io, std::size_t num_samples) -> void
    {
        auto const n = std::int64_t(num_samples);
        neo::hip::check(neo_hip_upols64_process_samples(_h.get(), io, n, io, n, n, 0, nullptr));
    }
    auto reset() -> void { neo::hip::check(neo_hip_upols64_reset(_h.get())); }

    [[nodiscard]] auto channels() const noexcept { return _C; }
    [[nodiscard]] auto block_size() const noexcept { return _B; }
    [[nodiscard]] auto partitions() const noexcept { return _P; }
    /// splits per channel and partitions per split of the MAC launch
    [[nodiscard]] auto splits() const -> std::pair<int, int>
    {
        int s = 0, r = 0;
        neo::hip::check(neo_hip_upols64_info(_h.get(), &s, &r, nullptr));
        return {s, r};
    }

    /// what batch_info() reports
    struct batch_report {
        int blocks_per_pass;      ///< 1 while batching is off
        int splits;               ///< splits per channel of the pass's MAC
        std::int64_t extra_bytes; ///< device bytes that batching holds
    };
    /// batched passes on or off: a process call of q T + r blocks then runs q passes of T blocks
    /// and r plain steps. State stays as it is, so it may come between any two process calls.
    auto batch(bool enable) -> void { neo::hip::check(neo_hip_upols64_set_batch(_h.get(), enable ? 1 : 0)); }
    [[nodiscard]] auto batch_info() const -> batch_report
    {
        batch_report r{};
        neo::hip::check(neo_hip_upols64_batch_info(_h.get(), &r.blocks_per_pass, &r.splits, &r.extra_bytes));
        return r;
    }

    /// what offline_info() reports
    struct offline_report {
        int blocks_per_pass;        ///< 128; 0 while offline windows are off
        int segments;               ///< ceil(P / 128)
        std::int64_t spectra_bytes; ///< device bytes of the segment spectra
        std::int64_t extra_bytes;   ///< device bytes of the scratch, the windows' spectra and the tails
    };
    /// offline windows on or off (neo_hip_upols64_set_offline): a process call then runs a window
    /// pass for every 128 blocks left, then batched passes if batch(true), then plain steps. State
    /// stays as it is, so it may come between any two process calls.
    auto offline(bool enable) -> void { neo::hip::check(neo_hip_upols64_set_offline(_h.get(), enable ? 1 : 0)); }
    [[nodiscard]] auto offline_info() const -> offline_report
    {
        offline_report r{};
        neo::hip::check(neo_hip_upols64_offline_info(_h.get(), &r.blocks_per_pass, &r.segments, &r.spectra_bytes,
                                                     &r.extra_bytes));
        return r;
    }

private:
    std::size_t _C, _B, _P;
    detail::upols64_ptr _h;
};

namespace detail {
struct upols_multi_deleter {
    void operator()(neo_hip_upols_multi* m) const noexcept { neo_hip_upols_multi_destroy(m); }
};
}  // namespace detail

/// upols_multichannel over several devices of one node (neo_hip_upols_multi_*): channel
/// shard i = [C i / n, C (i + 1) / n) on devices[i] (a device may repeat), no collective
/// (channels are independent, DenseConvolution.hpp:35,50-67); every call runs the shards
/// concurrently. Results equal one upols_multichannel over all channels bit for bit.
struct upols_multidevice {
    upols_multidevice(std::size_t channels, std::size_t block_size, std::size_t partitions,
                      std::vector<int> const& devices, method m = method::upols)
        : _C{channels}, _B{block_size}, _P{partitions}
    {
        int const mi = m == method::upols ? 0 : m == method::upola ? 1 : -1;
        if (mi < 0) throw std::invalid_argument{"neo_hip: multidevice convolver supports method::upols and method::upola"};
        neo_hip_upols_multi* h = nullptr;
        neo::hip::check(neo_hip_upols_multi_create(int(channels), int(block_size), int(partitions), devices.data(),
                                                   int(devices.size()), mi, nullptr, &h));
        _h.reset(h);
    }

    /// filter [C][P][B+1] complex<float>, contiguous host memory; resets state
    auto filter(std::complex<float> const* partitions) -> void
    {
        neo::hip::check(neo_hip_upols_multi_set_filter(_h.get(), partitions));
    }
    /// normalize_impulse over all channels (optional) + uniform_partition of ir [C][length]
    auto impulse(float const* ir, std::size_t length, bool normalize = true) -> void
    {
        neo::hip::check(neo_hip_upols_multi_set_impulse(_h.get(), ir, std::int64_t(length), normalize ? 1 : 0));
    }
    /// num_samples (whole blocks) per channel, in place, io [C][num_samples] host memory
    auto process(float* io, std::size_t num_samples) -> void
    {
        auto const n = std::int64_t(num_samples);
        neo::hip::check(neo_hip_upols_multi_process_samples(_h.get(), io, n, io, n, n));
    }
    auto reset() -> void { neo::hip::check(neo_hip_upols_multi_reset(_h.get())); }
    /// upols_multichannel::update_filter on every shard, host memory, complete on return
    auto update_filter(std::complex<float> const* partitions, int fade_blocks = 1, fade_curve curve = fade_curve::linear)
        -> void
    {
        neo::hip::check(neo_hip_upols_multi_update_filter(_h.get(), partitions, fade_blocks, int(curve)));
    }
    /// the same from ir [C][length]; the normalisation factor is taken once over all channels
    auto update_impulse(float const* ir, std::size_t length, bool normalize = true, int fade_blocks = 1,
                        fade_curve curve = fade_curve::linear) -> void
    {
        neo::hip::check(neo_hip_upols_multi_update_impulse(_h.get(), ir, std::int64_t(length), normalize ? 1 : 0,
                                                           fade_blocks, int(curve)));
    }
    /// the shards' fades run in step: shard 0's counts, the shards' bank bytes summed
    [[nodiscard]] auto fade_info() const -> fade_desc
    {
        fade_desc d{};
        for (int i = 0, n = shards(); i < n; ++i) {
            neo_hip_upols* h = nullptr;
            neo::hip::check(neo_hip_upols_multi_shard(_h.get(), i, &h, nullptr, nullptr, nullptr));
            fade_desc s{};
            neo::hip::check(neo_hip_upols_fade_info(h, &s.remaining_blocks, &s.fade_blocks, &s.bank_bytes));
            if (i == 0) d = s;
            else d.bank_bytes += s.bank_bytes;
        }
        return d;
    }
    [[nodiscard]] auto shards() const -> int
    {
        int n = 0;
        neo::hip::check(neo_hip_upols_multi_shards(_h.get(), &n));
        return n;
    }

    [[nodiscard]] auto channels() const noexcept { return _C; }
    [[nodiscard]] auto block_size() const noexcept { return _B; }
    [[nodiscard]] auto partitions() const noexcept { return _P; }

private:
    std::size_t _C, _B, _P;
    std::unique_ptr<neo_hip_upols_multi, detail::upols_multi_deleter> _h;
};

/// Single-channel drop-in for upols_convolver<Complex> (uniform_partitioned_convolver.hpp:13-65)
/// and, with M = method::upola, upola_convolver: default-constructible; filter([P][B+1])
/// (re)initializes everything; operator()(block[B]) in place. Complex = std::complex<float> runs on
/// upols_multichannel, std::complex<double> on upols_multichannel64 (no latency mode there).
template<typename Complex, method M = method::upols>
struct hip_upols_convolver {
    static_assert(std::same_as<Complex, std::complex<float>> || std::same_as<Complex, std::complex<double>>);
    using value_type = Complex;
    using real_type = typename Complex::value_type;
    using accumulator_type = neo::hip::array<Complex, 1>;
    static constexpr bool is_double = std::same_as<real_type, double>;
    using impl_type = std::conditional_t<is_double, upols_multichannel64, upols_multichannel>;

    hip_upols_convolver() = default;

    template<typename InMat>
        requires neo::hip::detail::matrix_like<InMat>
    auto filter(InMat filter) -> void
    {
        auto const P = std::size_t(filter.extent(0)), bins = std::size_t(filter.extent(1));
        std::vector<Complex> h(P * bins);
        for (std::size_t p = 0; p < P; ++p)
            for (std::size_t k = 0; k < bins; ++k) h[p * bins + k] = Complex(neo::hip::detail::at(filter, p, k));
        if (!_impl || _impl->partitions() != P || _impl->block_size() != bins - 1) {
            _impl = std::make_unique<impl_type>(1, bins - 1, P, neo::hip::detail::default_device(), M);
            if constexpr (!is_double)
                if (_latency) _impl->latency_mode(true, _idle_ms);
        }
        _impl->filter(h.data());
        _block.resize(bins - 1);
    }

    /// latency mode for this instance (upols_multichannel::latency_mode), kept across filter()
    /// calls; applied at the next filter() when no filter was set yet. The double type has none: throws.
    auto latency_mode(bool on, double idle_ms = 50.0) -> void
    {
        if constexpr (is_double) {
            (void)on;
            (void)idle_ms;
            throw std::invalid_argument{"neo_hip: the latency mode is float32 only (std::complex<double> convolvers have none)"};
        } else {
            _latency = on;
            _idle_ms = idle_ms;
            if (_impl) _impl->latency_mode(on, idle_ms);
        }
    }

    template<typename Vec>
        requires neo::hip::detail::vector_like<Vec>
    auto operator()(Vec block) -> void
    {
        if (neo::hip::detail::contiguous(block)) {
            (*_impl)(block.data_handle());
            return;
        }
        neo::hip::detail::gather(block, _block.data());
        (*_impl)(_block.data());
        neo::hip::detail::scatter(_block.data(), block);
    }

private:
    std::unique_ptr<impl_type> _impl;
    std::vector<real_type> _block;
    bool _latency = false;
    double _idle_ms = 50.0;
};

/// The mask a sparsity predicate gives over a filter matrix [P][B+1]: mask[p (B+1) + k] =
/// sparsity(p, k, filter(p, k)), the call sparse_filter::filter makes per element
/// (sparse_filter.hpp:25-28, csr_matrix.hpp:32-34). Host only.
template<typename InMat, typename Sparsity>
    requires neo::hip::detail::matrix_like<InMat>
[[nodiscard]] auto sparsity_mask(InMat filter, Sparsity&& sparsity) -> std::vector<std::uint8_t>
{
    auto const P = std::size_t(filter.extent(0)), bins = std::size_t(filter.extent(1));
    std::vector<std::uint8_t> mask(P * bins);
    for (std::size_t p = 0; p < P; ++p)
        for (std::size_t k = 0; k < bins; ++k)
            mask[p * bins + k] = sparsity(p, k, neo::hip::detail::at(filter, p, k)) ? 1 : 0;
    return mask;
}

/// Single-channel drop-in for sparse_upols_convolver<complex<float>> and, with M = method::upola,
/// sparse_upola_convolver (sparse_convolver.hpp:12-17): filter([P][B+1], sparsity) with sparsity
/// callable as (row, col, value) -> bool; operator()(block[B]) in place. One channel on a sparse
/// handle of its own.
template<typename Complex, method M = method::upols>
struct hip_sparse_upols_convolver {
    static_assert(std::same_as<Complex, std::complex<float>>);
    using value_type = Complex;
    using accumulator_type = neo::hip::array<Complex, 1>;

    hip_sparse_upols_convolver() = default;

    template<typename InMat, typename Sparsity>
        requires(neo::hip::detail::matrix_like<InMat> && !std::same_as<std::remove_cvref_t<Sparsity>, perceptual_sparsity>)
    auto filter(InMat filter, Sparsity&& sparsity) -> void
    {
        auto const P = std::size_t(filter.extent(0)), bins = std::size_t(filter.extent(1));
        std::vector<Complex> h(P * bins);
        for (std::size_t p = 0; p < P; ++p)
            for (std::size_t k = 0; k < bins; ++k) h[p * bins + k] = Complex(neo::hip::detail::at(filter, p, k));
        auto const mask = sparsity_mask(filter, sparsity);
        if (!_impl || _impl->partitions() != P || _impl->block_size() != bins - 1)
            _impl = std::make_unique<upols_multichannel>(sparse, 1, bins - 1, P, neo::hip::detail::default_device(), M);
        _impl->filter_sparse(h.data(), mask.data());
        _block.resize(bins - 1);
    }

    /// the plugin's rule instead of a callable: the mask is made on the device from the filter
    template<typename InMat>
        requires neo::hip::detail::matrix_like<InMat>
    auto filter(InMat filter, perceptual_sparsity const& sparsity) -> void
    {
        auto const P = std::size_t(filter.extent(0)), bins = std::size_t(filter.extent(1));
        sparsity.validate(bins - 1);
        std::vector<Complex> h(P * bins);
        for (std::size_t p = 0; p < P; ++p)
            for (std::size_t k = 0; k < bins; ++k) h[p * bins + k] = Complex(neo::hip::detail::at(filter, p, k));
        if (!_impl || _impl->partitions() != P || _impl->block_size() != bins - 1)
            _impl = std::make_unique<upols_multichannel>(sparse, 1, bins - 1, P, neo::hip::detail::default_device(), M);
        _impl->filter_perceptual(h.data(), sparsity);
        _block.resize(bins - 1);
    }

    /// Live update: crossfade to `filter` under `sparsity` (a callable, as filter() takes it) over the
    /// next fade_blocks blocks, keeping all state (upols_multichannel::update_filter_sparse); filter()
    /// remains the resetting call. The shape must be the current filter's; throws before a filter()
    /// and while a fade still runs.
    template<typename InMat, typename Sparsity>
        requires(neo::hip::detail::matrix_like<InMat> && !std::same_as<std::remove_cvref_t<Sparsity>, perceptual_sparsity>)
    auto update_filter(InMat filter, Sparsity&& sparsity, int fade_blocks = 1, fade_curve curve = fade_curve::linear) -> void
    {
        auto const h = checked_copy(filter);
        auto const mask = sparsity_mask(filter, sparsity);
        _impl->update_filter_sparse(h.data(), mask.data(), fade_blocks, curve);
    }

    /// the same with the plugin's rule: the mask is made on the device from the filter
    template<typename InMat>
        requires neo::hip::detail::matrix_like<InMat>
    auto update_filter(InMat filter, perceptual_sparsity const& sparsity, int fade_blocks = 1,
                       fade_curve curve = fade_curve::linear) -> void
    {
        auto const h = checked_copy(filter);
        _impl->update_filter_perceptual(h.data(), sparsity, fade_blocks, curve);
    }

    [[nodiscard]] auto fade_info() const -> fade_desc { return _impl ? _impl->fade_info() : fade_desc{}; }

    template<typename Vec>
        requires neo::hip::detail::vector_like<Vec>
    auto operator()(Vec block) -> void
    {
        if (neo::hip::detail::contiguous(block)) {
            (*_impl)(block.data_handle());
            return;
        }
        neo::hip::detail::gather(block, _block.data());
        (*_impl)(_block.data());
        neo::hip::detail::scatter(_block.data(), block);
    }

private:
    // an update's filter as contiguous [P][B+1]: the shape of the filter the handle has
    template<typename InMat>
    auto checked_copy(InMat filter) const -> std::vector<Complex>
    {
        auto const P = std::size_t(filter.extent(0)), bins = std::size_t(filter.extent(1));
        if (!_impl) throw std::runtime_error("sparse convolver: update_filter before filter()");
        if (_impl->partitions() != P || _impl->block_size() != bins - 1)
            throw std::runtime_error("sparse convolver: update_filter takes a filter of the current filter's shape");
        std::vector<Complex> h(P * bins);
        for (std::size_t p = 0; p < P; ++p)
            for (std::size_t k = 0; k < bins; ++k) h[p * bins + k] = Complex(neo::hip::detail::at(filter, p, k));
        return h;
    }

    std::unique_ptr<upols_multichannel> _impl;
    std::vector<float> _block;
};

template<typename Complex>
using sparse_upols_convolver = hip_sparse_upols_convolver<Complex>;

template<typename Complex>
using sparse_upola_convolver = hip_sparse_upols_convolver<Complex, method::upola>;

/// Single-channel drop-in for upola_convolver_v2<complex<float>> (dense_convolver.hpp:28,
/// overlap_add_convolver.hpp:20-136): operator()(samples) takes any number of samples.
template<typename Complex>
struct hip_upola2_convolver {
    static_assert(std::same_as<Complex, std::complex<float>>);
    using value_type = Complex;
    using accumulator_type = neo::hip::array<Complex, 1>;

    hip_upola2_convolver() = default;

    template<typename InMat>
        requires neo::hip::detail::matrix_like<InMat>
    auto filter(InMat filter) -> void
    {
        auto const P = std::size_t(filter.extent(0)), bins = std::size_t(filter.extent(1));
        std::vector<Complex> h(P * bins);
        for (std::size_t p = 0; p < P; ++p)
            for (std::size_t k = 0; k < bins; ++k) h[p * bins + k] = Complex(neo::hip::detail::at(filter, p, k));
        if (!_impl || _impl->partitions() != P || _impl->block_size() != bins - 1)
            _impl = std::make_unique<upols_multichannel>(upola_v2, 1, bins - 1, P);
        _impl->filter(h.data());
    }

    template<typename Vec>
        requires neo::hip::detail::vector_like<Vec>
    auto operator()(Vec inout) -> void
    {
        auto const n = std::size_t(inout.extent(0));
        if (neo::hip::detail::contiguous(inout)) {
            _impl->process(inout.data_handle(), n);
            return;
        }
        _buf.resize(n);
        neo::hip::detail::gather(inout, _buf.data());
        _impl->process(_buf.data(), n);
        neo::hip::detail::scatter(_buf.data(), inout);
    }

private:
    std::unique_ptr<upols_multichannel> _impl;
    std::vector<float> _buf;
};

namespace detail {
struct matrix_deleter {
    void operator()(neo_hip_matrix* m) const noexcept { neo_hip_matrix_destroy(m); }
};
}  // namespace detail

/// A route of a matrix convolver: output `out` takes input `in` through a filter of its own.
struct matrix_route {
    int out;
    int in;
};

/// Matrix (multi-input, multi-output) convolver over libneo_hip's neo_hip_matrix_* (include/neo_hip.h):
/// output o = the sum over its routes (o, i) of what upols_convolver (M = method::upols) or
/// upola_convolver (M = method::upola) gives for (input i, that route's filter). The reference has
/// no such class; it is the routed form of its per-channel convolvers. One delay line per input,
/// one inverse transform per output. Construction and filter() throw std::runtime_error; the call
/// operator is noexcept like its neighbours.
template<method M>
struct hip_matrix_convolver {
    static_assert(M == method::upols || M == method::upola, "matrix convolvers: upols or upola");

    /// opts nullptr = all defaults (neo_hip_matrix_opts: fused, split_workgroups, out_tile)
    hip_matrix_convolver(std::size_t inputs, std::size_t outputs, std::size_t block_size, std::size_t partitions,
                         neo_hip_matrix_opts const* opts = nullptr, int device = neo::hip::detail::default_device())
        : _I{inputs}, _O{outputs}, _B{block_size}, _P{partitions}
    {
        neo_hip_matrix* m = nullptr;
        neo::hip::check(neo_hip_matrix_create(int(inputs), int(outputs), int(block_size), int(partitions), device,
                                              M == method::upola ? 1 : 0, opts, &m));
        _h.reset(m);
    }

    /// partitions [routes][P][B+1] in uniform_partition layout (host memory), one per route in the
    /// list's order; resets all state like filter() everywhere else
    auto filter(std::complex<float> const* partitions, std::vector<matrix_route> const& routes) -> void
    {
        std::vector<int> ro(routes.size()), ri(routes.size());
        for (std::size_t r = 0; r < routes.size(); ++r) ro[r] = routes[r].out, ri[r] = routes[r].in;
        neo::hip::check(neo_hip_matrix_set_filter(_h.get(), partitions, ro.data(), ri.data(), int(routes.size()), 0));
    }

    /// the dense matrix: partitions [O][I][P][B+1], every output fed by every input
    auto filter(std::complex<float> const* partitions) -> void
    {
        std::vector<matrix_route> all;
        for (std::size_t o = 0; o < _O; ++o)
            for (std::size_t i = 0; i < _I; ++i) all.push_back({int(o), int(i)});
        filter(partitions, all);
    }

    /// one block: in [I][B] -> out [O][B], host memory, complete on return; the two may be the same buffer
    auto operator()(float const* in, float* out) noexcept -> void
    {
        neo::hip::check_or_abort(
            neo_hip_matrix_process(_h.get(), in, std::int64_t(_B), out, std::int64_t(_B), 1, 0, nullptr));
    }

    /// num_blocks blocks: input i at in + i ld_in, output o at out + o ld_out (throws on bad strides)
    auto process(float const* in, std::size_t ld_in, float* out, std::size_t ld_out, std::size_t num_blocks,
                 bool device_memory = false, void* stream = nullptr) -> void
    {
        neo::hip::check(neo_hip_matrix_process(_h.get(), in, std::int64_t(ld_in), out, std::int64_t(ld_out),
                                               std::int64_t(num_blocks), device_memory ? 1 : 0, stream));
    }

    /// clears all state; a running fade (update_filter) completes: the new filter is the filter
    auto reset() -> void { neo::hip::check(neo_hip_matrix_reset(_h.get())); }

    /// live update (neo_hip_matrix_update_filter): crossfade to `partitions` ([routes][P][B+1], host
    /// memory, the route order of the last filter()) over the next fade_blocks blocks and KEEP ALL
    /// STATE -- delay lines, windows, overlap tails; filter() remains the resetting call. The route
    /// list does not change. Complete on return; throws while a fade still runs.
    auto update_filter(std::complex<float> const* partitions, int fade_blocks = 1, fade_curve curve = fade_curve::linear)
        -> void
    {
        neo::hip::check(neo_hip_matrix_update_filter(_h.get(), partitions, 0, fade_blocks, int(curve), nullptr));
    }

    /// the same from impulse responses ir [routes][length] (host memory): normalize_impulse over all
    /// routes' rows if `normalize`, then uniform_partition on the device; keeps all state
    auto update_impulse(float const* ir, std::size_t length, bool normalize = true, int fade_blocks = 1,
                        fade_curve curve = fade_curve::linear) -> void
    {
        neo::hip::check(neo_hip_matrix_update_impulse(_h.get(), ir, std::int64_t(length), normalize ? 1 : 0, 0, fade_blocks,
                                                      int(curve), nullptr));
    }

    using fade_desc = ::neo::convolution::fade_desc;  ///< (bank_bytes: 0 until the first update after a filter)
    [[nodiscard]] auto fade_info() const -> fade_desc
    {
        fade_desc d{};
        neo::hip::check(neo_hip_matrix_fade_info(_h.get(), &d.remaining_blocks, &d.fade_blocks, &d.bank_bytes));
        return d;
    }

    /// batched passes: process() runs up to 32 blocks of a call per pass over every route's filter
    /// (neo_hip_matrix_set_batch); the stream continues across the call. split_workgroups 0 = automatic
    auto batch(bool on, int split_workgroups = 0) -> void
    {
        neo::hip::check(neo_hip_matrix_set_batch(_h.get(), on ? 1 : 0, split_workgroups));
    }
    struct batch_desc {
        int blocks_per_pass, splits, ring_rows;
    };
    [[nodiscard]] auto batch_info() const -> batch_desc
    {
        batch_desc d{};
        neo::hip::check(neo_hip_matrix_batch_info(_h.get(), &d.blocks_per_pass, &d.splits, &d.ring_rows));
        return d;
    }

    /// offline windows: process() runs passes of 256 (windows_per_pass 1: 128) blocks while that many
    /// are left, by 256-point transforms along the block axis (neo_hip_matrix_set_offline: long
    /// filters, every block of a call known up front); the stream continues across the call
    auto offline(bool on, int windows_per_pass = 0) -> void
    {
        neo::hip::check(neo_hip_matrix_set_offline(_h.get(), on ? 1 : 0, windows_per_pass));
    }
    struct offline_desc {
        int blocks_per_pass, segments, ring_rows;
        std::int64_t spectra_bytes;
    };
    [[nodiscard]] auto offline_info() const -> offline_desc
    {
        offline_desc d{};
        neo::hip::check(neo_hip_matrix_offline_info(_h.get(), &d.blocks_per_pass, &d.segments, &d.ring_rows, &d.spectra_bytes));
        return d;
    }

    /// window levels: long filters one block per call (neo_hip_matrix_set_levels). A single step then
    /// reads only the head, partitions [0, 2 windows[0]), on every block and each level its band once per
    /// window of its length, one window ahead. windows empty = the default (8, 32); split_workgroups 0 =
    /// automatic. May be switched at any time between calls; throws on a bad window list
    auto levels(bool on, std::span<int const> windows = {}, int split_workgroups = 0) -> void
    {
        neo::hip::check(neo_hip_matrix_set_levels(_h.get(), on ? 1 : 0, windows.empty() ? nullptr : windows.data(),
                                                  int(windows.size()), split_workgroups));
    }
    [[nodiscard]] auto levels_info() const -> neo_hip_matrix_levels_desc
    {
        neo_hip_matrix_levels_desc d{};
        neo::hip::check(neo_hip_matrix_levels_info(_h.get(), &d));
        return d;
    }

    [[nodiscard]] auto info() const -> neo_hip_matrix_desc
    {
        neo_hip_matrix_desc d{};
        neo::hip::check(neo_hip_matrix_info(_h.get(), &d));
        return d;
    }
    [[nodiscard]] auto inputs() const noexcept { return _I; }
    [[nodiscard]] auto outputs() const noexcept { return _O; }
    [[nodiscard]] auto block_size() const noexcept { return _B; }
    [[nodiscard]] auto partitions() const noexcept { return _P; }

private:
    std::unique_ptr<neo_hip_matrix, detail::matrix_deleter> _h;
    std::size_t _I, _O, _B, _P;
};

using upols_matrix_convolver = hip_matrix_convolver<method::upols>;
using upola_matrix_convolver = hip_matrix_convolver<method::upola>;

namespace detail {
struct group_deleter {
    void operator()(neo_hip_upols_group* g) const noexcept { neo_hip_upols_group_destroy(g); }
};
}  // namespace detail

/// The convolvers of ONE owner (one plugin instance: DenseConvolution's
/// std::vector<upols_convolver>, DenseConvolution.hpp:35), grouped per shape
/// (neo_hip_upols_group_*): grouped_upols_convolver instances whose filter() runs inside a
/// scope() of this object join its group of their shape; instances outside any scope run alone.
/// register_buffer() names host memory the owner keeps allocated (its frame buffer) until
/// unregister_all(): only convolvers called on such buffers are stepped together.
class convolver_group {
public:
    convolver_group() = default;
    convolver_group(convolver_group const&) = delete;
    auto operator=(convolver_group const&) -> convolver_group& = delete;

    /// RAII: convolvers whose filter() runs on this thread while the scope lives join `g`
    class scope_guard {
    public:
        explicit scope_guard(convolver_group& g) noexcept : _prev{current()} { current() = &g; }
        ~scope_guard() { current() = _prev; }
        scope_guard(scope_guard const&) = delete;
        auto operator=(scope_guard const&) -> scope_guard& = delete;

    private:
        convolver_group* _prev;
    };
    [[nodiscard]] auto scope() -> scope_guard { return scope_guard{*this}; }

    /// what the owner promises about a registered frame buffer (neo_hip_upols_group_register_ex)
    enum class frame : int {
        plain = 0,                           ///< allocated until unregister_all(): exact comparison per member
        stable = NEO_HIP_GROUP_FRAME_STABLE,  ///< + written by nothing but the convolvers' calls during a frame
        in_place = NEO_HIP_GROUP_FRAME_STABLE | NEO_HIP_GROUP_FRAME_INPLACE,  ///< + read only through them, each
                                                                              ///< on the same block: outputs in place
    };
    /// [ptr, ptr + samples) stays allocated until unregister_all() (cheap to repeat per frame), with
    /// the owner's promise about it during a frame (the plugin's loop over a filled frame keeps
    /// frame::in_place; frame::stable skips the members' snapshot comparison)
    auto register_buffer(float const* ptr, std::size_t samples, frame promise = frame::plain) -> void
    {
        std::lock_guard<std::mutex> lk{_mu};
        auto const flags = int(promise);
        bool found = false;
        for (auto& r : _ranges)
            if (r.ptr == ptr && r.samples == samples) {
                r.flags = flags;
                found = true;
            }
        if (!found) _ranges.push_back({ptr, samples, flags});
        for (auto& [key, g] : _groups)
            neo::hip::check(neo_hip_upols_group_register_ex(g.get(), ptr, std::int64_t(samples * sizeof(float)), flags));
    }
    /// before the registered memory is freed or reallocated (e.g. at prepare())
    auto unregister_all() -> void
    {
        std::lock_guard<std::mutex> lk{_mu};
        _ranges.clear();
        for (auto& [key, g] : _groups) neo::hip::check(neo_hip_upols_group_unregister(g.get(), nullptr));
    }

    /// the group of one shape (created on first use, with the ranges registered so far)
    auto acquire(std::size_t block, std::size_t partitions, method m, int device) -> std::shared_ptr<neo_hip_upols_group>
    {
        std::lock_guard<std::mutex> lk{_mu};
        auto const key = std::array<std::size_t, 4>{block, partitions, std::size_t(m == method::upola), std::size_t(device)};
        if (auto it = _groups.find(key); it != _groups.end()) return it->second;
        auto g = make_group(block, partitions, m, device);
        for (auto const& r : _ranges)
            neo::hip::check(
                neo_hip_upols_group_register_ex(g.get(), r.ptr, std::int64_t(r.samples * sizeof(float)), r.flags));
        _groups.emplace(key, g);
        return g;
    }

    static auto make_group(std::size_t block, std::size_t partitions, method m, int device)
        -> std::shared_ptr<neo_hip_upols_group>
    {
        neo_hip_upols_group* raw = nullptr;
        neo::hip::check(
            neo_hip_upols_group_create(int(block), int(partitions), m == method::upola ? 1 : 0, device, &raw));
        return std::shared_ptr<neo_hip_upols_group>(raw, detail::group_deleter{});
    }

    /// the group scope active on this thread, or null
    static auto current() noexcept -> convolver_group*&
    {
        thread_local convolver_group* cur = nullptr;
        return cur;
    }

private:
    std::mutex _mu;
    std::map<std::array<std::size_t, 4>, std::shared_ptr<neo_hip_upols_group>> _groups;
    struct range {
        float const* ptr;
        std::size_t samples;
        int flags;
    };
    std::vector<range> _ranges;
};

/// Single-channel drop-in for upols_convolver<complex<float>> (uniform_partitioned_convolver.hpp:13-65)
/// that joins the convolver_group whose scope() is active when its filter() runs (else it runs
/// alone): in the plugin's frame pattern (DenseConvolution.cpp:62-74: every instance called once
/// per frame on a buffer of its own, inside the owner's registered frame buffer) a frame of all
/// instances is ONE launch instead of one launch and one wait per instance; each instance's
/// outputs are its own sequential convolver's in any pattern. upols_convolver / upola_convolver
/// are this type when NEO_HIP_CONVOLVER_GROUPS is defined (the split_* forms are not: the
/// plugin's Convolution.hpp:61 runs them on the host's own output buffer).
template<typename Complex, method M = method::upols>
struct grouped_upols_convolver {
    static_assert(std::same_as<Complex, std::complex<float>>);
    using value_type = Complex;
    using accumulator_type = neo::hip::array<Complex, 1>;

    grouped_upols_convolver() = default;
    grouped_upols_convolver(grouped_upols_convolver&& o) noexcept
        : _g{std::move(o._g)}, _owner{o._owner}, _id{std::exchange(o._id, -1)}, _B{o._B}, _P{o._P},
          _block{std::move(o._block)}
    {}
    auto operator=(grouped_upols_convolver&& o) noexcept -> grouped_upols_convolver&
    {
        if (this != &o) {
            leave();
            _g = std::move(o._g);
            _owner = o._owner;
            _id = std::exchange(o._id, -1);
            _B = o._B;
            _P = o._P;
            _block = std::move(o._block);
        }
        return *this;
    }
    ~grouped_upols_convolver() { leave(); }

    template<typename InMat>
        requires neo::hip::detail::matrix_like<InMat>
    auto filter(InMat filter) -> void
    {
        auto const P = std::size_t(filter.extent(0)), bins = std::size_t(filter.extent(1));
        std::vector<Complex> h(P * bins);
        for (std::size_t p = 0; p < P; ++p)
            for (std::size_t k = 0; k < bins; ++k) h[p * bins + k] = Complex(neo::hip::detail::at(filter, p, k));
        auto* owner = convolver_group::current();
        if (!_g || _P != P || _B != bins - 1 || owner != _owner) {
            leave();
            auto const dev = neo::hip::detail::default_device();
            _g = owner ? owner->acquire(bins - 1, P, M, dev) : convolver_group::make_group(bins - 1, P, M, dev);
            _owner = owner;
            neo::hip::check(neo_hip_upols_group_join(_g.get(), &_id));
            _B = bins - 1;
            _P = P;
            _block.resize(_B);
        }
        neo::hip::check(neo_hip_upols_group_set_filter(_g.get(), _id, h.data(), 0));
    }

    template<typename Vec>
        requires neo::hip::detail::vector_like<Vec>
    auto operator()(Vec block) -> void
    {
        if (neo::hip::detail::contiguous(block)) {
            neo::hip::check_or_abort(neo_hip_upols_group_process(_g.get(), _id, block.data_handle()));
            return;
        }
        neo::hip::detail::gather(block, _block.data());
        neo::hip::check_or_abort(neo_hip_upols_group_process(_g.get(), _id, _block.data()));
        neo::hip::detail::scatter(_block.data(), block);
    }

    /// the group this instance belongs to (diagnostics: neo_hip_upols_group_stats)
    [[nodiscard]] auto group() const noexcept -> neo_hip_upols_group* { return _g.get(); }

private:
    void leave() noexcept
    {
        if (_g && _id >= 0) (void)neo_hip_upols_group_leave(_g.get(), _id);
        _g.reset();
        _owner = nullptr;
        _id = -1;
    }

    std::shared_ptr<neo_hip_upols_group> _g;
    convolver_group* _owner = nullptr;
    int _id = -1;
    std::size_t _B = 0, _P = 0;
    std::vector<float> _block;
};

namespace detail {
struct overlap_deleter {
    void operator()(neo_hip_overlap* h) const noexcept { neo_hip_overlap_destroy(h); }
};

/// overlap_save / overlap_add (overlap_save.hpp:19-112, overlap_add.hpp:23-107) on the GPU:
/// ctor(block_size, filter_size), transform size 2^next_order(B + F - 1); operator()(block,
/// callback) runs the window update and rfft on the device, hands the callback the
/// transform_size() / 2 + 1 bins (a host view it may modify in place), then the irfft, 1/n and
/// the output block, in place.
template<typename Complex, int Kind>
struct hip_overlap {
    static_assert(std::same_as<Complex, std::complex<float>>);
    using value_type = Complex;
    using complex_type = Complex;
    using real_type = typename Complex::value_type;
    using size_type = std::size_t;

    hip_overlap(size_type block_size, size_type filter_size)
    {
        neo_hip_overlap* h = nullptr;
        neo::hip::check(neo_hip_overlap_create(Kind, 1, std::int64_t(block_size), std::int64_t(filter_size),
                                               neo::hip::detail::default_device(), &h));
        _h.reset(h);
        std::int64_t b = 0, f = 0, n = 0;
        neo::hip::check(neo_hip_overlap_info(h, &b, &f, &n));
        _block = size_type(b);
        _filter = size_type(f);
        _n = size_type(n);
        _bins.resize(_n / 2 + 1);
        _buf.resize(_block);
    }

    [[nodiscard]] auto block_size() const noexcept -> size_type { return _block; }
    [[nodiscard]] auto filter_size() const noexcept -> size_type { return _filter; }
    [[nodiscard]] auto transform_size() const noexcept -> size_type { return _n; }

    template<typename Vec, typename Callback>
        requires neo::hip::detail::vector_like<Vec>
    auto operator()(Vec block, Callback callback) -> void
    {
        float* io = _buf.data();
        bool const direct = neo::hip::detail::contiguous(block) && std::size_t(block.extent(0)) == _block;
        if (direct) io = block.data_handle();
        else neo::hip::detail::gather(block, _buf.data());
        neo::hip::check_or_abort(neo_hip_overlap_forward(_h.get(), io, std::int64_t(_block), _bins.data(), 0, nullptr));
        callback(neo::hip::make_view(_bins.data(), _bins.size()));
        neo::hip::check_or_abort(neo_hip_overlap_inverse(_h.get(), _bins.data(), io, std::int64_t(_block), 0, nullptr));
        if (!direct) neo::hip::detail::scatter(_buf.data(), block);
    }

private:
    std::unique_ptr<neo_hip_overlap, overlap_deleter> _h;
    size_type _block{}, _filter{}, _n{};
    std::vector<Complex> _bins;
    std::vector<float> _buf;
};
}  // namespace detail

template<typename Complex>
using overlap_save = detail::hip_overlap<Complex, 0>;

template<typename Complex>
using overlap_add = detail::hip_overlap<Complex, 1>;

#ifdef NEO_HIP_CONVOLVER_GROUPS
template<typename Complex>
using upols_convolver = grouped_upols_convolver<Complex>;

template<typename Complex>
using split_upols_convolver = hip_upols_convolver<Complex>;

/// dense_convolver.hpp:23-24, 32-35 (overlap-add stage, same FDL MAC)
template<typename Complex>
using upola_convolver = grouped_upols_convolver<Complex, method::upola>;

template<typename Complex>
using split_upola_convolver = hip_upols_convolver<Complex, method::upola>;
#else
template<typename Complex>
using upols_convolver = hip_upols_convolver<Complex>;

template<typename Complex>
using split_upols_convolver = hip_upols_convolver<Complex>;

/// dense_convolver.hpp:23-24, 32-35 (overlap-add stage, same FDL MAC)
template<typename Complex>
using upola_convolver = hip_upols_convolver<Complex, method::upola>;

template<typename Complex>
using split_upola_convolver = hip_upols_convolver<Complex, method::upola>;
#endif

/// dense_convolver.hpp:28
template<typename Complex>
using upola_convolver_v2 = hip_upola2_convolver<Complex>;

/// dense_convolve<upols_convolver> (DenseConvolution.hpp:39-70) over plain arrays:
/// signal [C][N], ir [C][L] -> out [C][N]; normalizes + partitions the IR, tail block zero-padded.
inline auto dense_convolve(float const* signal, std::size_t channels, std::size_t num_samples, float const* ir,
                           std::size_t ir_length, std::size_t block_size, float* out, method m = method::upols) -> void
{
    upols_multichannel conv{channels, block_size, num_partitions(ir_length, block_size),
                            neo::hip::detail::default_device(), m};
    conv.impulse(ir, ir_length, true);
    // whole signal in chunks of <= 2^26 samples: one upload, batched passes over the
    // filter and FDL, one download per chunk; the tail block is zero-padded
    std::size_t const nb = (num_samples + block_size - 1) / block_size;
    std::size_t chunk = std::max<std::size_t>(1, (std::size_t(1) << 26) / (channels * block_size));
    chunk = std::max<std::size_t>(256, chunk / 256 * 256);  // whole offline passes (two windows of 128 blocks)
    std::vector<float> buf;
    for (std::size_t t0 = 0; t0 < nb; t0 += chunk) {
        std::size_t const t1 = std::min(nb, t0 + chunk), lo = t0 * block_size,
                          hi = std::min(num_samples, t1 * block_size), n = (t1 - t0) * block_size;
        buf.assign(channels * n, 0.0F);
        for (std::size_t c = 0; c < channels; ++c)
            std::copy(signal + c * num_samples + lo, signal + c * num_samples + hi, buf.data() + c * n);
        conv.process(buf.data(), n);
        for (std::size_t c = 0; c < channels; ++c)
            std::copy(buf.data() + c * n, buf.data() + c * n + (hi - lo), out + c * num_samples + lo);
    }
}

/// the same in double (upols_multichannel64): signal, ir and out of double; offline: in offline
/// windows of 128 blocks (upols_multichannel64::offline), what is left in plain steps
inline auto dense_convolve(double const* signal, std::size_t channels, std::size_t num_samples, double const* ir,
                           std::size_t ir_length, std::size_t block_size, double* out, method m = method::upols,
                           bool offline = false) -> void
{
    upols_multichannel64 conv{channels, block_size, num_partitions(ir_length, block_size),
                              neo::hip::detail::default_device(), m};
    conv.impulse(ir, ir_length, true);
    if (offline) conv.offline(true);
    std::size_t const nb = (num_samples + block_size - 1) / block_size;
    std::size_t chunk = std::max<std::size_t>(1, (std::size_t(1) << 25) / (channels * block_size));
    if (offline) chunk = std::max<std::size_t>(128, chunk / 128 * 128);  // whole windows
    std::vector<double> buf;
    for (std::size_t t0 = 0; t0 < nb; t0 += chunk) {
        std::size_t const t1 = std::min(nb, t0 + chunk), lo = t0 * block_size,
                          hi = std::min(num_samples, t1 * block_size), n = (t1 - t0) * block_size;
        buf.assign(channels * n, 0.0);
        for (std::size_t c = 0; c < channels; ++c)
            std::copy(signal + c * num_samples + lo, signal + c * num_samples + hi, buf.data() + c * n);
        conv.process(buf.data(), n);
        for (std::size_t c = 0; c < channels; ++c)
            std::copy(buf.data() + c * n, buf.data() + c * n + (hi - lo), out + c * num_samples + lo);
    }
}

namespace detail {
// the loop of dense_convolve on a convolver whose filter is set: chunks of <= 2^26 samples, one
// upload, batched passes, one download per chunk; the tail block is zero-padded
inline auto convolve_chunks(upols_multichannel& conv, float const* signal, std::size_t channels,
                            std::size_t num_samples, std::size_t block_size, float* out) -> void
{
    std::size_t const nb = (num_samples + block_size - 1) / block_size;
    std::size_t chunk = std::max<std::size_t>(1, (std::size_t(1) << 26) / (channels * block_size));
    chunk = std::max<std::size_t>(256, chunk / 256 * 256);
    std::vector<float> buf;
    for (std::size_t t0 = 0; t0 < nb; t0 += chunk) {
        std::size_t const t1 = std::min(nb, t0 + chunk), lo = t0 * block_size,
                          hi = std::min(num_samples, t1 * block_size), n = (t1 - t0) * block_size;
        buf.assign(channels * n, 0.0F);
        for (std::size_t c = 0; c < channels; ++c)
            std::copy(signal + c * num_samples + lo, signal + c * num_samples + hi, buf.data() + c * n);
        conv.process_checked(buf.data(), n);
        for (std::size_t c = 0; c < channels; ++c)
            std::copy(buf.data() + c * n, buf.data() + c * n + (hi - lo), out + c * num_samples + lo);
    }
}
}  // namespace detail

/// The plugin's sparse_convolve loop (extra/plugin/src/dsp/DenseConvolution.cpp:124-186) over plain
/// arrays: signal [C][N], ir [C][L] -> out [C][N]; normalizes + partitions the IR, keeps the filter
/// bins of mask [C][P][B+1] (nonzero = keep; P = num_partitions(L, B)), tail block zero-padded.
/// Every block is known up front: the sparse handle runs batched passes.
inline auto sparse_convolve(float const* signal, std::size_t channels, std::size_t num_samples, float const* ir,
                            std::size_t ir_length, std::size_t block_size, std::uint8_t const* mask, float* out,
                            method m = method::upola) -> void
{
    auto const P = num_partitions(ir_length, block_size);
    int const device = neo::hip::detail::default_device();
    std::vector<float> h(ir, ir + channels * ir_length);
    neo::hip::check(neo_hip_normalize_impulse(h.data(), int(channels), std::int64_t(ir_length), 0, device));
    std::vector<std::complex<float>> parts(channels * P * (block_size + 1));
    neo::hip::check(neo_hip_uniform_partition(h.data(), int(channels), std::int64_t(ir_length), int(block_size),
                                              parts.data(), 0, device));
    upols_multichannel conv{sparse, channels, block_size, P, device, m};
    conv.filter_sparse(parts.data(), mask);
    conv.batch(true);
    detail::convolve_chunks(conv, signal, channels, num_samples, block_size, out);
}
/// the same with the plugin's own rule instead of a mask: the mask is made on the device
inline auto sparse_convolve(float const* signal, std::size_t channels, std::size_t num_samples, float const* ir,
                            std::size_t ir_length, std::size_t block_size, perceptual_sparsity const& sparsity,
                            float* out, method m = method::upola) -> void
{
    upols_multichannel conv{sparse, channels, block_size, num_partitions(ir_length, block_size),
                            neo::hip::detail::default_device(), m};
    conv.impulse_perceptual(ir, ir_length, sparsity, true);
    conv.batch(true);
    detail::convolve_chunks(conv, signal, channels, num_samples, block_size, out);
}

/// fft_convolve (fft_convolver.hpp:72-93): full linear convolution on the GPU, host arrays
/// (float or double, like the reference's Python overloads, main.cpp:255-258)
template<typename Float>
    requires(std::same_as<Float, float> || std::same_as<Float, double>)
inline auto fft_convolve(Float const* signal, std::size_t n, Float const* patch, std::size_t m) -> std::vector<Float>
{
    if (n == 0 || m == 0) return {};
    std::vector<Float> out(n + m - 1);
    auto const f = [] {
        if constexpr (std::same_as<Float, double>) return neo_hip_fft_convolve_f64;
        else return neo_hip_fft_convolve;
    }();
    neo::hip::check(f(signal, std::int64_t(n), patch, std::int64_t(m), out.data(), 0, neo::hip::detail::default_device()));
    return out;
}

/// direct_convolve (direct_convolve.hpp:58-68): same loop order and rounding as the reference
template<typename Float>
    requires(std::same_as<Float, float> || std::same_as<Float, double>)
inline auto direct_convolve(Float const* signal, std::size_t n, Float const* patch, std::size_t m)
    -> std::vector<Float>
{
    if (n == 0 || m == 0) return {};
    std::vector<Float> out(n + m - 1);
    auto const f = [] {
        if constexpr (std::same_as<Float, double>) return neo_hip_direct_convolve_f64;
        else return neo_hip_direct_convolve;
    }();
    neo::hip::check(f(signal, std::int64_t(n), patch, std::int64_t(m), out.data(), 0, neo::hip::detail::default_device()));
    return out;
}

}  // namespace neo::convolution
