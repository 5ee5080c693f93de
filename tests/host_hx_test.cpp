// The host-only code of VCFX_haplotype_extractor (vcfx_amd/csrc/tools/hx_host.h) as a program of its
// own, built under ASan + UBSan (make build/san/host_hx_asan; tests/test_host_hx.py): std::stoi for -b,
// the header-line rule, the sample names, the GT spans and the texts the host formats, over lines held
// in heap blocks of exactly their size (a read past one is a sanitizer report).  Prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "hx_host.h"

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

struct Block {  // the bytes of s in a heap block of exactly their size
    std::unique_ptr<char[]> p;
    size_t n;
    explicit Block(const std::string &s) : p(s.empty() ? nullptr : new char[s.size()]), n(s.size()) {
        if (n) memcpy(p.get(), s.data(), n);
    }
};

struct Stoi {
    const char *text;
    int ok, value;
};

static std::string gts_of(const std::string &line, size_t ns) {
    Block b(line);
    std::vector<std::pair<uint32_t, uint32_t>> g;
    if (!hx_gts(b.p.get(), b.n, ns, g)) return "-";
    std::string o;
    for (auto &x : g) o += "[" + std::string(b.p.get() + x.first, x.second) + "]";
    return o;
}

int main() {
    const Stoi cases[] = {
        {"0", 1, 0},
        {"100000", 1, 100000},
        {"-1", 1, -1},
        {"+10", 1, 10},
        {" 7", 1, 7},
        {"\t\n\v\f\r 8", 1, 8},
        {"10x", 1, 10},
        {"010", 1, 10},
        {"2147483647", 1, 2147483647},
        {"-2147483648", 1, -2147483647 - 1},
        {"2147483648", 0, 0},
        {"-2147483649", 0, 0},
        {"99999999999999999999999999", 0, 0},
        {"", 0, 0},
        {"x", 0, 0},
        {"-", 0, 0},
        {"+-1", 0, 0},
        {"- 1", 0, 0},
    };
    for (const Stoi &c : cases) {
        int v = 12345;
        Block b(std::string(c.text) + std::string(1, '\0'));
        CHECK(hx_stoi(b.p.get(), v) == (c.ok != 0));
        CHECK(c.ok ? v == c.value : v == 12345);
    }
    // the header-line rule
    auto head = [](const std::string &s, bool in) {
        Block b(s);
        return hx_head_line(b.p.get(), b.n, in);
    };
    CHECK(head("", false) == kHxSkip && head("", true) == kHxSkip);
    CHECK(head("\r", false) == kHxSkip && head("\r", true) == kHxData);
    CHECK(head("#", false) == kHxSkip && head("##x", true) == kHxSkip && head("#CHRO", true) == kHxSkip);
    CHECK(head("#CHROM", false) == kHxChrom && head("#CHROMX\tA\r", true) == kHxChrom && head("#CHRO\r", true) == kHxSkip);
    CHECK(head("1\t2", false) == kHxData && head("x\r", true) == kHxData && head(" #CHROM", false) == kHxData);
    // the names
    auto names = [](const std::string &s) {
        Block b(s);
        std::vector<std::string> v;
        const bool ok = hx_names(b.p.get(), hx_strip(b.p.get(), b.n), v);
        std::string o = ok ? "+" : "-";
        for (auto &x : v) o += "[" + x + "]";
        return o;
    };
    const std::string nine = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
    CHECK(names(nine) == "-" && names("#CHROM") == "-" && names("") == "-");
    CHECK(names(nine + "\t") == "+[]" && names(nine + "\tA") == "+[A]" && names(nine + "\tA\tB\r") == "+[A][B]");
    CHECK(names(nine + "\tA\t") == "+[A][]" && names(nine + "\t\t\t") == "+[][][]");
    CHECK(hx_header_row({}) == "CHROM\tSTART\tEND\n" && hx_header_row({"A", "", "B"}) == "CHROM\tSTART\tEND\tA\t\tB\n");
    // the GT spans
    const std::string h = "1\t5\t.\tA\tC\t.\t.\t.\t";
    CHECK(gts_of(h + "GT\t0|1\t1|0", 2) == "[0|1][1|0]");
    CHECK(gts_of(h + "GT\t0|1\t1|0\tx", 2) == "[0|1][1|0]");
    CHECK(gts_of(h + "GT\t0|1", 2) == "-" && gts_of(h + "GT", 1) == "-" && gts_of("1\t5", 1) == "-");
    CHECK(gts_of(h + "AD:GT:DP\t5:0|1|1:3\t5:|:", 2) == "[0|1|1][|]");
    CHECK(gts_of(h + "AD:GT\t5:0|1\t5", 2) == "-" && gts_of(h + "AD:GT\t5:0|1\t5:", 2) == "[0|1][]");
    CHECK(gts_of(h + "AD:DP\t5:0|1", 1) == "-" && gts_of(h + "GTX:GT\t1:0|1", 1) == "[0|1]" && gts_of(h + "\t0|1", 1) == "-");
    CHECK(gts_of(h + "GT\t", 1) == "[]" && gts_of(h + "GT:GT\t0|1:1|1", 1) == "[0|1]");
    // the texts
    std::string w;
    {
        Block b("chrX\t77\t.");
        hx_warn_unphased(b.p.get(), b.n, 77, w);
        Block c("lonely");
        hx_warn_unphased(c.p.get(), c.n, 0, w);
        Block d("");
        hx_warn_unphased(d.p.get(), d.n, 2147483647, w);
    }
    CHECK(w == "Warning: Not all samples phased at chrX:77.\nWarning: Not all samples phased at lonely:0.\n"
               "Warning: Not all samples phased at :2147483647.\n");
    auto pair = [&](const std::string &a, const std::string &b, size_t ns, uint32_t flip) {
        Block x(a), y(b);
        std::vector<std::pair<uint32_t, uint32_t>> p, c;
        CHECK(hx_gts(x.p.get(), x.n, ns, p) && hx_gts(y.p.get(), y.n, ns, c));
        std::string o;
        hx_debug_pair(x.p.get(), p, y.p.get(), c, flip, o);
        return o;
    };
    CHECK(pair(h + "GT\t0|1\t|", h + "GT\t1|0\t0|1", 2, 0) ==
          "Checking phase consistency\nSample 0 last GT: 0|1 new GT: 1|0\nComparing alleles: 0|1 vs 1|0\n"
          "Phase flip detected in sample 0\n");
    CHECK(pair(h + "GT\t0|1\t|", h + "GT\t0|1\t0|1", 2, 2) ==
          "Checking phase consistency\nSample 0 last GT: 0|1 new GT: 0|1\nComparing alleles: 0|1 vs 0|1\n"
          "Sample 1 last GT: | new GT: 0|1\nAll phases consistent\n");
    CHECK(pair(h + "GT\t0|0|1\t1|1", h + "GT\t0|1\t1|0|0|1", 2, 1) ==
          "Checking phase consistency\nSample 0 last GT: 0|0|1 new GT: 0|1\nComparing alleles: 0|1 vs 0|1\n"
          "Sample 1 last GT: 1|1 new GT: 1|0|0|1\nComparing alleles: 1|1 vs 1|1\nPhase flip detected in sample 1\n");
    printf("ok %ld\n", checks);
    return 0;
}
