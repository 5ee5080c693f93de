// decimal_bounds_test.cpp -- threshold_bounds (vcfxg_decimal.cpp) on doubles given by bit pattern.
//
// stdin: one 64-bit pattern per line, in hex.  stdout, one line per pattern:
//   <pattern> <kind> <lo> <hi> <lo_to_t> <hi_to_t>
// where a boundary is <sign>,<exp>,<inf>,<digits> ('-' for no digits).  A NaN prints its kind only.
// Built under ASan + UBSan (make build/san/decimal_bounds_asan); tests/test_decimal_bounds.py feeds it
// and compares every line with the midpoints of the double and its neighbours as exact fractions.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "vcfxg_decimal.h"

static void put(const vcfxg::DecHost &d) {
    printf(" %d,%d,%d,%s", d.sign, d.exp, d.inf, d.digits.empty() ? "-" : d.digits.c_str());
}

int main() {
    char line[64];
    while (fgets(line, sizeof line, stdin)) {
        uint64_t bits;
        if (sscanf(line, "%" SCNx64, &bits) != 1) continue;
        double t;
        memcpy(&t, &bits, sizeof t);
        vcfxg::ThresholdHost h;
        vcfxg::threshold_bounds(t, h);
        uint64_t back;
        memcpy(&back, &h.t, sizeof back);
        printf("%016" PRIx64 " %d", back, h.kind);
        if (h.kind == 0) {
            put(h.lo);
            put(h.hi);
            printf(" %d %d", h.lo_to_t, h.hi_to_t);
        }
        printf("\n");
    }
    return 0;
}
