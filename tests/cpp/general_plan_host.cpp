// general_plan_host.cpp — TEST INFRASTRUCTURE: the host planning of the general kernels (teloscope_amd/csrc/general_plan_core.h:
// the region rule, the region tile planner, the whole-segment table entry) run by a program of its own under AddressSanitizer
// and UBSan, so that tests/test_general_plan_cpu.py can hold the code every driver calls to a plain restatement of the rules.
// Usage: general_plan_host < CASES.  One case per line, one line of numbers per case:
//   regions LEN TIPS TERMINAL_LIMIT                   ->  regions N : start,len ...
//   tiles IN_OFF SEG_START LEN SEG STEP HALO          ->  tiles N : in_off,seg_rel,k_p0,r_p0,n,avail,seg ...
//   entry IN_OFF LEN ABS_POS FIRST_TILE N_TILES SEG   ->  entry in_off,len,abs_pos,lo_rel,hi_rel,t0,t1,o0,o1,flags,seg
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../teloscope_amd/csrc/general_plan_core.h"

int main() {
    char kind[16];
    unsigned long long v[6];
    while (std::scanf("%15s", kind) == 1) {
        const int want = std::strcmp(kind, "regions") == 0 ? 3 : 6;
        for (int i = 0; i < want; ++i)
            if (std::scanf("%llu", &v[i]) != 1) { std::fprintf(stderr, "short case\n"); return 2; }
        if (std::strcmp(kind, "regions") == 0) {
            const tsplan::Regions R = tsplan::scanned_regions(v[0], v[1] != 0, (uint32_t)v[2]);
            std::printf("regions %u :", R.n);
            for (const tsplan::Span &s : R) std::printf(" %" PRIu64 ",%" PRIu64, s.start, s.len);
            std::printf("\n");
        } else if (std::strcmp(kind, "tiles") == 0) {
            std::vector<TsGeneralTile> tiles;                       // (grown tile by tile: a write past what was appended is a sanitizer error)
            tsplan::append_region_tiles(tiles, v[0], v[1], v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]);
            std::printf("tiles %zu :", tiles.size());
            for (const TsGeneralTile &T : tiles)
                std::printf(" %llu,%llu,%llu,%u,%u,%u,%u", T.in_off, T.seg_rel, T.k_p0, T.r_p0, T.n, T.avail, T.seg);
            std::printf("\n");
        } else if (std::strcmp(kind, "entry") == 0) {
            const TsShardSegIn S = tsplan::whole_segment_entry(v[0], v[1], v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]);
            std::printf("entry %llu,%llu,%llu,%llu,%llu,%u,%u,%u,%u,%u,%u\n", S.in_off, S.len, S.abs_pos, S.lo_rel, S.hi_rel, S.t0, S.t1, S.o0,
                        S.o1, S.flags, S.seg);
        } else {
            std::fprintf(stderr, "bad case: %s\n", kind);
            return 2;
        }
    }
    return 0;
}
