// env_knobs_test.cpp -- the context's environment-knob reader (vcfxg_env.h) on the host, a program of
// its own (tests/test_env_knobs_cpu.py builds it under ASan + UBSan, sets the environment and checks
// what it prints).  One case per input line:
//   u64 <NAME> <default> <lo> <hi>      env_u64
//   i64 <NAME> <default> <lo> <hi>      env_i64
//   set <NAME>                          env_set
// For each it prints the value read.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "vcfxg_env.h"

using namespace vcfxg;

int main() {
    char line[512], what[8], name[128];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long d, lo, hi;
        long long sd, slo, shi;
        if (sscanf(line, "%7s %127s", what, name) != 2) continue;
        if (!strcmp(what, "u64")) {
            if (sscanf(line, "%*s %*s %llu %llu %llu", &d, &lo, &hi) != 3) return 2;
            printf("%" PRIu64 "\n", env_u64(name, d, lo, hi));
        } else if (!strcmp(what, "i64")) {
            if (sscanf(line, "%*s %*s %lld %lld %lld", &sd, &slo, &shi) != 3) return 2;
            printf("%" PRId64 "\n", env_i64(name, sd, slo, shi));
        } else if (!strcmp(what, "set")) {
            printf("%d\n", env_set(name) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
