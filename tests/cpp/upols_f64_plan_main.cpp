// Stand-alone host program for neo-dsp_amd/csrc/upols_f64_plan.hpp (no GPU, no HIP header): the
// plan of every case read from standard input, one line each
//   plan channels block partitions method split_workgroups
//   io   block num_samples ld_in ld_out
// printed as one JSON object per line: the plan's fields ({"ok": 1} for an accepted io case), or
// {"refused": "<why>"}. The rules are checked by the caller (tests/test_upols_f64.py).
#include "../../neo-dsp_amd/csrc/upols_f64_plan.hpp"

#include <cstdio>
#include <cstring>

int main()
{
    char what[8];
    int cases = 0;
    while (std::scanf("%7s", what) == 1) {
        ++cases;
        if (!std::strcmp(what, "plan")) {
            int C, B, P, method, split;
            if (std::scanf("%d %d %d %d %d", &C, &B, &P, &method, &split) != 5) return 2;
            neo_hip::upols64_shape s;
            if (const char* why = neo_hip::make_upols64_shape(C, B, P, method, split, s)) {
                std::printf("{\"refused\": \"%s\"}\n", why);
                continue;
            }
            std::printf("{\"S\": %d, \"rows\": %d, \"ola\": %d, \"filter_bytes\": %lld, \"fdl_bytes\": %lld, \"prev_bytes\": %lld, "
                        "\"slab_bytes\": %lld, \"state_bytes\": %lld, \"step_bytes\": %lld}\n",
                        s.S, s.rows, int(s.ola), (long long)s.filter_bytes, (long long)s.fdl_bytes, (long long)s.prev_bytes,
                        (long long)s.slab_bytes, (long long)s.state_bytes, (long long)s.step_bytes);
        } else if (!std::strcmp(what, "io")) {
            int B;
            long long n, li, lo;
            if (std::scanf("%d %lld %lld %lld", &B, &n, &li, &lo) != 4) return 2;
            if (const char* why = neo_hip::upols64_io_refusal(B, n, li, lo)) std::printf("{\"refused\": \"%s\"}\n", why);
            else std::printf("{\"ok\": 1}\n");
        } else {
            return 2;
        }
    }
    std::fprintf(stderr, "%d cases\n", cases);
    return 0;
}
