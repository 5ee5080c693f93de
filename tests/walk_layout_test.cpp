// walk_layout_test.cpp -- the record walk's chunk layout (vcfxg_walk_layout.h) on the host, a
// program of its own (tests/test_walk_layout_cpu.py builds it under ASan + UBSan and checks what
// it prints).  One case per input line:
//   make <lo> <hi> <C> <Cs> <K1> <waves> <xcd>          walk_layout_make (K1 = -1: every round full)
//   plan <lo> <hi> <C0> <S> <knob> <waves> <xcd>        walk_layout_plan (knob as VCFXG_WALK_LAYOUT)
// For each it prints "layout <kind> <C> <Cs> <K1> <grid> <nw> <base0..7>", then one line
// "<hardware block> <wave> <file-order walker> <cs> <ce> <size>" per walker of the grid, computed
// by walk_range exactly as the kernel does, then "end".
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "vcfxg_walk_layout.h"

using namespace vcfxg;

int main() {
    char line[512], what[16], knob[64];
    while (fgets(line, sizeof line, stdin)) {
        long long lo, hi, C, a, b;
        int waves, xcd, kind = 0;
        WalkLayout l;
        if (sscanf(line, "%15s", what) != 1) continue;
        if (!strcmp(what, "make")) {
            if (sscanf(line, "%*s %lld %lld %lld %lld %lld %d %d", &lo, &hi, &C, &a, &b, &waves, &xcd) != 7) return 2;
            l = walk_layout_make(lo, hi, C, a, b < 0 ? kWalkAllRounds : (uint32_t)b, waves, xcd != 0);
        } else if (!strcmp(what, "plan")) {
            if (sscanf(line, "%*s %lld %lld %lld %lld %63s %d %d", &lo, &hi, &C, &a, knob, &waves, &xcd) != 7) return 2;
            l = walk_layout_plan(lo, hi, C, a, parse_walk_layout(knob), waves, xcd != 0, &kind);
        } else {
            return 2;
        }
        printf("layout %d %" PRId64 " %" PRId64 " %lld %u %" PRId64, kind, l.C, l.Cs,
               l.K1 == kWalkAllRounds ? -1ll : (long long)l.K1, l.grid, l.nw);
        for (uint32_t x = 0; x < kWalkXcds; x++) printf(" %" PRId64, l.base[x]);
        printf("\n");
        for (uint32_t blk = 0; blk < l.grid; blk++)
            for (int wv = 0; wv < waves; wv++) {
                int64_t cs, ce, size;
                const int64_t wk = walk_range(l, blk, l.grid, wv, waves, hi, xcd != 0, cs, ce, size);
                printf("%u %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", blk, wv, wk, cs, ce, size);
            }
        printf("end\n");
    }
    return 0;
}
