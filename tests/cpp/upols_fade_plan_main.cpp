// Stand-alone host program for the fade split rule of neo-dsp_amd/csrc/upols_plan.hpp
// (upols_fade_split; no GPU, no HIP header): for every case read from standard input, one line each
//   channels block partitions fused(-1|0|1) split_workgroups
// the dense handle's plan and the fade step's, printed as one JSON object per line, or
// {"refused": "<why>"}. tests/test_upols_fade.py checks the rule; built with
// -fsanitize=address,undefined any bad read or overflow inside it ends the program.
#include "../../neo-dsp_amd/csrc/upols_plan.hpp"

#include <cstdio>

int main()
{
    int C, B, P, fused, wgs, cases = 0;
    while (std::scanf("%d %d %d %d %d", &C, &B, &P, &fused, &wgs) == 5) {
        const neo_hip_upols_opts opts{fused, wgs, 0, 0, -1, -1, 0, 0, 0, 0, 0};
        neo_hip::upols_shape s;
        ++cases;
        if (const char* why = neo_hip::make_upols_shape(C, B, P, &opts, neo_hip::upols_kind::dense, false, s)) {
            std::printf("{\"refused\": \"%s\"}\n", why);
            continue;
        }
        const neo_hip::upols_fade_plan f = neo_hip::upols_fade_split(s);
        std::printf("{\"S\": %d, \"rows\": %d, \"slab_bytes\": %lld, \"bank_bytes\": %lld, \"plain_S\": %d, \"plain_rows\": %d, "
                    "\"plain_fused\": %d, \"ring\": %d}\n",
                    f.S, f.rows, (long long)f.slab_bytes, (long long)f.bank_bytes, s.S, s.rows, int(s.fused), s.sched.ring);
    }
    std::fprintf(stderr, "%d cases\n", cases);
    return 0;
}
