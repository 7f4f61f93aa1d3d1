// Stand-alone host program for the offline windows of neo-dsp_amd/csrc/upols_f64_plan.hpp (no GPU, no
// HIP header): every case read from standard input, one line each
//   offline channels block partitions method   the plan of the window passes of a shape
//   src P w       the source of every window row e = -128 (nseg + 1) .. 127 of a pass at w
//   commit P w    the ring row every block of a window pass commits (-1: none)
// printed as one JSON object per line: the plan's fields, {"refused": "<why>"}, or
//   src:    {"first": e of the first row, "rows": [[kind, row] ...]}   kind 0 scratch, 1 ring, 2 zero
//   commit: {"rows": [row for j = 0..127]}
// The rules are checked by the caller (tests/test_upols_f64_offline.py).
#include "../../neo-dsp_amd/csrc/upols_f64_plan.hpp"

#include <cstdio>
#include <cstring>

int main()
{
    char what[8];
    int cases = 0;
    while (std::scanf("%7s", what) == 1) {
        ++cases;
        if (!std::strcmp(what, "offline")) {
            int C, B, P, method;
            if (std::scanf("%d %d %d %d", &C, &B, &P, &method) != 4) return 2;
            neo_hip::upols64_shape s;
            if (const char* why = neo_hip::make_upols64_shape(C, B, P, method, 0, s)) {
                std::printf("{\"refused\": \"%s\"}\n", why);
                continue;
            }
            const neo_hip::upols64_offline_shape o = neo_hip::make_upols64_offline_shape(s);
            std::printf("{\"W\": %d, \"F\": %d, \"nseg\": %d, \"spectra_bytes\": %lld, \"scratch_bytes\": %lld, \"y_bytes\": %lld, "
                        "\"tail_bytes\": %lld, \"extra_bytes\": %lld, \"pass_bytes\": %lld, \"filter_bytes\": %lld, "
                        "\"fdl_bytes\": %lld}\n",
                        neo_hip::kOff64W, neo_hip::kOff64F, o.nseg, (long long)o.spectra_bytes, (long long)o.scratch_bytes,
                        (long long)o.y_bytes, (long long)o.tail_bytes, (long long)o.extra_bytes, (long long)o.pass_bytes,
                        (long long)s.filter_bytes, (long long)s.fdl_bytes);
        } else if (!std::strcmp(what, "src")) {
            int P, w;
            if (std::scanf("%d %d", &P, &w) != 2 || P < 1) return 2;
            const int nseg = (P + neo_hip::kOff64W - 1) / neo_hip::kOff64W, first = -neo_hip::kOff64W * (nseg + 1);
            std::printf("{\"first\": %d, \"rows\": [", first);
            for (int e = first; e < neo_hip::kOff64W; ++e) {
                const neo_hip::upols64_offline_row r = neo_hip::upols64_offline_src(e, w, P);
                std::printf("%s[%d, %d]", e > first ? ", " : "", r.kind, r.row);
            }
            std::printf("]}\n");
        } else if (!std::strcmp(what, "commit")) {
            int P, w;
            if (std::scanf("%d %d", &P, &w) != 2 || P < 1) return 2;
            std::printf("{\"rows\": [");
            for (int j = 0; j < neo_hip::kOff64W; ++j)
                std::printf("%s%d", j ? ", " : "", neo_hip::upols64_commit_row(j, neo_hip::kOff64W, P, w));
            std::printf("]}\n");
        } else {
            return 2;
        }
    }
    std::fprintf(stderr, "%d cases\n", cases);
    return 0;
}
