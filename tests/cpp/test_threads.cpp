// test_threads.cpp — the thread contract of neo_hip.h ("Threads and streams") through the C++
// header API: eight std::threads, released together, each owning a neo::fft::fft_plan of order 10
// and a neo::convolution::upols_multichannel (2 channels, B = 64, 12 partitions), all eight also
// sharing ONE fft_plan of order 13 (the smallest multi-pass plan: one pair of staging buffers and
// one set of scratch buffers for every caller). Each thread brings its own objects up inside the
// thread, runs 100 rounds on its own host buffers and compares every result with the one computed
// serially before the threads started, by memcmp: distinct objects need no locking by the caller,
// a shared plan's calls are serialised by the library, and results are bit-identical to the same
// calls made one after the other. Only throwing entry points are used; a mismatch or an error
// prints a line and makes main return 1.
#include <neo/convolution.hpp>
#include <neo/fft.hpp>

#include "../../oracle/neo_oracle.h"

#include <atomic>
#include <complex>
#include <cstdio>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

using cf = std::complex<float>;
using plan_t = neo::fft::fft_plan<cf>;

namespace {

constexpr int kThreads = 8, kRounds = 100;
constexpr std::size_t C = 2, B = 64, P = 12, NB = 8;

struct job {
    std::vector<cf> x10, want10, x13, want13, parts;
    std::vector<float> sig, want_sig;
};

std::vector<cf> cnoise(std::uint64_t seed, std::size_t n)
{
    std::vector<cf> z(n);
    oracle_noise(seed, reinterpret_cast<float*>(z.data()), 2 * n);  // interleaved {re, im}
    return z;
}

std::mutex g_print;
std::atomic<int> g_bad{0};

void report(int t, int round, char const* what)
{
    std::lock_guard<std::mutex> lk(g_print);
    std::printf("thread %d, round %d: %s\n", t, round, what);
    ++g_bad;
}

template<class T>
bool same(std::vector<T> const& a, std::vector<T> const& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

void convolve(neo::convolution::upols_multichannel& conv, job const& j, std::vector<float>& io)
{
    io = j.sig;
    conv.reset();
    conv.process_checked(io.data(), NB * B);
}

}  // namespace

int main()
{
    int ndev = 0;
    if (neo_hip_device_count(&ndev) != NEO_HIP_OK || ndev < 1) {
        std::printf("no GPU: nothing to run\n");
        return 0;
    }
    try {
        // inputs and the serial results: fresh objects, one call after the other
        std::vector<job> jobs(kThreads);
        {
            plan_t serial13{neo::fft::from_order, 13};
            for (int t = 0; t < kThreads; ++t) {
                job& j = jobs[std::size_t(t)];
                j.x10 = cnoise(7000 + 10 * std::uint64_t(t), 1 << 10);
                j.x13 = cnoise(7001 + 10 * std::uint64_t(t), 1 << 13);
                j.want10.resize(j.x10.size());
                j.want13.resize(j.x13.size());
                plan_t p10{neo::fft::from_order, 10};
                p10.execute_host(j.x10.data(), j.want10.data(), neo::fft::direction::forward);
                serial13.execute_host(j.x13.data(), j.want13.data(), neo::fft::direction::forward);
                std::vector<float> ir(C * B * P);
                for (std::size_t c = 0; c < C; ++c) oracle_noise(7002 + 10 * std::uint64_t(t) + c, ir.data() + c * B * P, B * P);
                // the status-returning calls (the header's normalize_impulse aborts on a device failure)
                neo::hip::check(neo_hip_normalize_impulse(ir.data(), int(C), std::int64_t(B * P), 0, 0));
                j.parts.resize(C * P * (B + 1));  // B * P samples: exactly P partitions
                neo::hip::check(neo_hip_uniform_partition(ir.data(), int(C), std::int64_t(B * P), int(B), j.parts.data(), 0, 0));
                j.sig.resize(C * NB * B);
                oracle_noise(7005 + 10 * std::uint64_t(t), j.sig.data(), j.sig.size());
                neo::convolution::upols_multichannel conv{C, B, P};
                conv.filter(j.parts.data());
                convolve(conv, j, j.want_sig);
            }
        }
        // a forward transform of noise is not the noise: the comparisons below can fail
        if (same(jobs[0].want10, jobs[0].x10) || same(jobs[0].want13, jobs[1].want13) ||
            same(jobs[0].want_sig, jobs[0].sig)) {
            std::printf("the serial results do not tell the inputs apart\n");
            return 1;
        }

        plan_t shared13{neo::fft::from_order, 13};
        std::atomic<int> waiting{kThreads};
        auto body = [&](int t) {
            int round = -1;
            try {
                job const& j = jobs[std::size_t(t)];
                --waiting;
                while (waiting.load() > 0) std::this_thread::yield();  // the barrier
                plan_t p10{neo::fft::from_order, 10};                  // bring-up beside the others' calls
                neo::convolution::upols_multichannel conv{C, B, P};
                conv.filter(j.parts.data());
                std::vector<cf> y10(j.x10.size()), y13(j.x13.size());
                std::vector<float> io;
                for (round = 0; round < kRounds; ++round) {
                    p10.execute_host(j.x10.data(), y10.data(), neo::fft::direction::forward);
                    if (!same(y10, j.want10)) report(t, round, "own fft_plan (order 10) differs from the serial result");
                    shared13.execute_host(j.x13.data(), y13.data(), neo::fft::direction::forward);
                    if (!same(y13, j.want13)) report(t, round, "shared fft_plan (order 13) differs from the serial result");
                    convolve(conv, j, io);
                    if (!same(io, j.want_sig)) report(t, round, "own upols_multichannel differs from the serial result");
                    if (g_bad.load() > 16) return;  // enough lines
                }
            } catch (std::exception const& e) {
                report(t, round, e.what());
            }
        };
        std::vector<std::thread> threads;
        for (int t = 0; t < kThreads; ++t) threads.emplace_back(body, t);
        for (auto& th : threads) th.join();
    } catch (std::exception const& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    if (g_bad.load()) {
        std::printf("thread test FAILED: %d mismatches or errors\n", g_bad.load());
        return 1;
    }
    std::printf("thread test passed: %d threads x %d rounds\n", kThreads, kRounds);
    return 0;
}
