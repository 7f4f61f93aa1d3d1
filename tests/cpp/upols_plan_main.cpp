// Stand-alone host program for neo-dsp_amd/csrc/upols_plan.hpp (no GPU, no HIP header): the shape
// plan of every case read from standard input, one line each
//   kind(dense|v2|sparse) borrowed(0|1) channels block partitions nopts(0|11) [11 option ints]
// printed as one JSON object per line: the plan's fields, or {"refused": "<why>"}. The rules are
// checked by the caller (tests/test_upols_plan.py: a golden file recorded from the handles of the
// commit before this header existed, and structural facts); built with
// -fsanitize=address,undefined any bad read or overflow inside the rules ends the program.
#include "../../neo-dsp_amd/csrc/upols_plan.hpp"

#include <cstdio>
#include <cstring>

int main()
{
    char kind[16];
    int borrowed, C, B, P, nopts, cases = 0;
    while (std::scanf("%15s %d %d %d %d %d", kind, &borrowed, &C, &B, &P, &nopts) == 6) {
        int o[11] = {};
        if (nopts != 0 && nopts != 11) return 2;
        for (int i = 0; i < nopts; ++i)
            if (std::scanf("%d", &o[i]) != 1) return 2;
        const neo_hip_upols_opts opts{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10]};
        neo_hip::upols_kind k;
        if (!std::strcmp(kind, "dense")) k = neo_hip::upols_kind::dense;
        else if (!std::strcmp(kind, "v2")) k = neo_hip::upols_kind::v2;
        else if (!std::strcmp(kind, "sparse")) k = neo_hip::upols_kind::sparse;
        else return 2;
        neo_hip::upols_shape s;
        ++cases;
        if (const char* why = neo_hip::make_upols_shape(C, B, P, nopts ? &opts : nullptr, k, borrowed != 0, s)) {
            std::printf("{\"refused\": \"%s\"}\n", why);
            continue;
        }
        std::printf("{\"fused\": %d, \"S\": %d, \"rows\": %d, \"Sb\": %d, \"rows_b\": %d, \"bT\": %d, \"bNB\": %d, \"pc\": %d, "
                    "\"pcb\": %d, \"bufload\": %d, \"off\": %d, \"off_nseg\": %d, \"ahead\": %d, \"batch\": %d, \"ring\": %d, "
                    "\"cstride\": %lld, \"pstride\": %lld, \"batch_blocks\": %d, \"sg\": %d, \"levels\": %d, \"nseg\": %d, "
                    "\"stag\": %d, \"window\": %d}\n",
                    int(s.fused), s.S, s.rows, s.Sb, s.rows_b, s.bT, s.bNB, s.pc, s.pcb, int(s.bufload), int(s.off), s.off_nseg,
                    int(s.ahead), int(s.batch), s.sched.ring, (long long)s.cstride, (long long)s.pstride,
                    neo_hip::batch_blocks(s), s.sched.sg, s.sched.lv.n, s.sched.lv.nseg, s.sched.lv.stag,
                    s.sched.lv.nseg ? neo_hip::kFarT : s.sched.lv.n ? s.sched.lv.T[s.sched.lv.n - 1] : 1);
    }
    std::fprintf(stderr, "%d cases\n", cases);
    return 0;
}
