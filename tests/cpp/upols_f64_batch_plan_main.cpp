// Stand-alone host program for the batched passes of neo-dsp_amd/csrc/upols_f64_plan.hpp (no GPU, no
// HIP header): every case read from standard input, one line each
//   batch  channels block partitions method split_workgroups blocks
//   window T P w p0      the source of every window row a split starting at p0 loads
//   commit T P w         the ring row every block of the pass commits (-1: none)
// printed as one JSON object per line: the plan's fields, {"refused": "<why>"}, or
//   window: {"first": [[scratch, row] for j = 0..T-1], "enter": [[scratch, row] for p = p0+1..P-1]}
//   commit: {"rows": [row for j = 0..T-1]}
// The rules are checked by the caller (tests/test_upols_f64_batch.py).
#include "../../neo-dsp_amd/csrc/upols_f64_plan.hpp"

#include <cstdio>
#include <cstring>

int main()
{
    char what[8];
    int cases = 0;
    while (std::scanf("%7s", what) == 1) {
        ++cases;
        if (!std::strcmp(what, "batch")) {
            int C, B, P, method, split, blocks;
            if (std::scanf("%d %d %d %d %d %d", &C, &B, &P, &method, &split, &blocks) != 6) return 2;
            neo_hip::upols64_shape s;
            neo_hip::upols64_batch_shape b;
            const char* why = neo_hip::make_upols64_shape(C, B, P, method, split, s);
            if (!why) why = neo_hip::make_upols64_batch_shape(s, blocks, split, b);
            if (why) {
                std::printf("{\"refused\": \"%s\"}\n", why);
                continue;
            }
            std::printf("{\"T\": %d, \"S\": %d, \"rows\": %d, \"scratch_bytes\": %lld, \"slab_bytes\": %lld, \"tail_bytes\": %lld, "
                        "\"extra_bytes\": %lld, \"pass_bytes\": %lld, \"filter_bytes\": %lld, \"fdl_bytes\": %lld, "
                        "\"state_bytes\": %lld}\n",
                        b.T, b.S, b.rows, (long long)b.scratch_bytes, (long long)b.slab_bytes, (long long)b.tail_bytes,
                        (long long)b.extra_bytes, (long long)b.pass_bytes, (long long)s.filter_bytes, (long long)s.fdl_bytes,
                        (long long)s.state_bytes);
        } else if (!std::strcmp(what, "window")) {
            int T, P, w, p0;
            if (std::scanf("%d %d %d %d", &T, &P, &w, &p0) != 4) return 2;
            std::printf("{\"first\": [");
            for (int j = 0; j < T; ++j) {
                const neo_hip::upols64_row_src r = neo_hip::upols64_window_src(j - p0, w, P);
                std::printf("%s[%d, %d]", j ? ", " : "", int(r.scratch), r.row);
            }
            std::printf("], \"enter\": [");
            for (int p = p0 + 1; p < P; ++p) {
                const neo_hip::upols64_row_src r = neo_hip::upols64_window_src(-p, w, P);
                std::printf("%s[%d, %d]", p > p0 + 1 ? ", " : "", int(r.scratch), r.row);
            }
            std::printf("]}\n");
        } else if (!std::strcmp(what, "commit")) {
            int T, P, w;
            if (std::scanf("%d %d %d", &T, &P, &w) != 3) return 2;
            std::printf("{\"rows\": [");
            for (int j = 0; j < T; ++j) std::printf("%s%d", j ? ", " : "", neo_hip::upols64_commit_row(j, T, P, w));
            std::printf("]}\n");
        } else {
            return 2;
        }
    }
    std::fprintf(stderr, "%d cases\n", cases);
    return 0;
}
