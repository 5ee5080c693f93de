// The host-only code of VCFX_field_extractor (vcfx_amd/csrc/tools/fx_host.h) as a program of its own,
// built under ASan + UBSan (make build/san/host_fx_asan; tests/test_host_fx.py): the --fields split,
// every field form in both modes, the S<n> check, the names of a "#CHROM" line held in a heap block of
// exactly its size (a read past it is a sanitizer report), names with '\r', a 10,000-item list.  Prints
// the tables of one list in both modes ("T <mode> ..." lines, which the test compares with the Python
// restatement's) and "ok <checks>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "fx_host.h"

using namespace vcfxh;

static long checks = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        checks++;                                                 \
        if (!(x)) {                                               \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                              \
        }                                                         \
    } while (0)

static std::vector<std::string> split(const char *a) {
    std::unique_ptr<char[]> p(new char[strlen(a) + 1]);  // (exactly its size)
    strcpy(p.get(), a);
    std::vector<std::string> f;
    fx_split_fields(p.get(), f);
    return f;
}

static std::unordered_map<std::string, uint32_t> names_of(const std::string &line) {
    std::unique_ptr<char[]> p(line.empty() ? nullptr : new char[line.size()]);
    if (!line.empty()) memcpy(p.get(), line.data(), line.size());
    std::unordered_map<std::string, uint32_t> n;
    fx_names(p.get(), line.size(), n);
    return n;
}

// the list the Python test holds too
static const char kList[] =
    "CHROM,POS,ID,REF,ALT,QUAL,FILTER,INFO,DP,,chrom,A=B,NA1:GT,NA2:DP,dup:GT,S1:GT,S005:DP,S0:X,S2147483638:GT,"
    "absent:GT,NA1:,:GT,S1:,NA1:GT:x,last\r:GT,Sx:GT,s1:GT";
static const char kHeader[] = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA1\tNA2\tdup\t\tdup\tlast\r";

int main() {
    // the split: every -f appends, empty items are kept
    CHECK(split("") == std::vector<std::string>{""});
    CHECK((split(",") == std::vector<std::string>{"", ""}));
    CHECK((split("a,,b,") == std::vector<std::string>{"a", "", "b", ""}));
    {
        std::vector<std::string> f = split("CHROM,POS");
        fx_split_fields("DP", f);
        fx_split_fields("", f);
        CHECK((f == std::vector<std::string>{"CHROM", "POS", "DP", ""}));
        CHECK(fx_header_row(f) == "CHROM\tPOS\tDP\t\n");
    }
    // standard names are exact
    CHECK(fx_standard("CHROM") == 0 && fx_standard("INFO") == 7 && fx_standard("FORMAT") < 0 && fx_standard("chrom") < 0 &&
          fx_standard("") < 0 && fx_standard("CHROM ") < 0);
    // the sample part
    struct {
        const char *part;
        int form;
        int64_t idx;
    } const parts[] = {{"S1", 1, 1},   {"S0", 1, 0},         {"S007", 1, 7},   {"S2147483647", 1, 2147483647},
                       {"S2147483648", -1, 0}, {"S99999999999", -1, 0}, {"S99999999999999999999999", -1, 0}, {"S", -1, 0},
                       {"", 0, 0},     {"s1", 0, 0},         {"S1a", 0, 0},    {"S-1", 0, 0},
                       {"S+1", 0, 0},  {"S 1", 0, 0},        {"NA12878", 0, 0}, {"SS1", 0, 0}};
    for (const auto &p : parts) {
        int64_t idx = 0;
        CHECK(fx_sample_index(p.part, idx) == p.form);
        if (p.form == 1) CHECK(idx == p.idx);
    }
    // the check before any input is read
    CHECK(fx_first_bad_field(split(kList)) == -1);
    CHECK(fx_first_bad_field(split("CHROM,S:GT")) == 1);
    CHECK(fx_first_bad_field(split("S99999999999:GT,S:GT")) == 0);
    CHECK(fx_first_bad_field(split("S,S99999999999,DP")) == -1);  // (no colon: INFO keys)
    CHECK(fx_first_bad_field(split("S:")) == 0);
    CHECK(fx_first_bad_field(split("a,b,S2147483648:x:y")) == 2);
    CHECK(!fx_needs_names(split("CHROM,DP,S1:GT,S2504:DP"), false) && !fx_needs_names(split("S0:GT"), true));
    CHECK(fx_needs_names(split("S0:GT"), false) && fx_needs_names(split("CHROM,NA1:GT"), true) && fx_needs_names(split(":GT"), false));
    // the "#CHROM" line
    CHECK(fx_is_chrom("#CHROM", 6) && fx_is_chrom("#CHROMx\tq", 9) && !fx_is_chrom("#CHRO", 5) && !fx_is_chrom("#chrom\t", 7));
    {
        const auto n = names_of(kHeader);
        CHECK(n.size() == 5 && n.at("NA1") == 9 && n.at("NA2") == 10 && n.at("dup") == 13 && n.at("") == 12 && n.at("last\r") == 14);
        CHECK(names_of("#CHROM\tPOS").empty() && names_of("").empty());
        const auto t = names_of("#CHROM\t1\t2\t3\t4\t5\t6\t7\t8\tx\t");  // (a trailing tab: an empty last name)
        CHECK(t.size() == 2 && t.at("x") == 9 && t.at("") == 10);
    }
    // the tables of the list in both modes
    for (int stdin_mode = 0; stdin_mode < 2; stdin_mode++) {
        std::vector<vcfxg_fx_col> cols;
        std::string pool;
        const std::vector<std::string> f = split(kList);
        fx_build(f, names_of(kHeader), stdin_mode != 0, cols, pool);
        CHECK(cols.size() == f.size());
        for (const vcfxg_fx_col &c : cols) {
            printf("T %d %u %u %u %u %u %u %u\n", stdin_mode, c.kind, c.col, c.named, c.key_off, c.key_len, c.sub_off, c.sub_len);
            if (c.key_len != VCFXG_FX_NOKEY) CHECK((size_t)c.key_off + c.key_len <= pool.size());
            CHECK((size_t)c.sub_off + c.sub_len <= pool.size());
        }
        printf("P %d ", stdin_mode);
        for (unsigned char ch : pool) printf("%02x", ch);
        printf("\n");
        // without a "#CHROM" line every name is unresolved
        fx_build(f, {}, stdin_mode != 0, cols, pool);
        for (const vcfxg_fx_col &c : cols) CHECK(!c.named || c.col == 0);
    }
    // a 10,000-item list
    {
        std::string big;
        for (int i = 0; i < 10000; i++) big += (i ? "," : "") + std::string(i % 3 == 0 ? "S" + std::to_string(i + 1) + ":GT" : i % 3 == 1 ? "K" + std::to_string(i) : "POS");
        const std::vector<std::string> f = split(big.c_str());
        CHECK(f.size() == 10000 && fx_first_bad_field(f) == -1);
        std::vector<vcfxg_fx_col> cols;
        std::string pool;
        fx_build(f, {}, true, cols, pool);
        CHECK(cols.size() == 10000 && cols[9999].kind == VCFXG_FX_SAMPLE && cols[9999].col == 9 + 9999 && cols[1].kind == VCFXG_FX_INFO &&
              cols[2].kind == VCFXG_FX_STD && cols[2].col == 1);
        CHECK(pool.substr(cols[9999].key_off, cols[9999].key_len) == "S10000:GT" && pool.substr(cols[9999].sub_off, cols[9999].sub_len) == "GT");
        CHECK(fx_header_row(f).size() == big.size() + 1);
    }
    printf("ok %ld\n", checks);
    return 0;
}
