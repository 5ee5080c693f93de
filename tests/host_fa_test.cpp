// The host-only code of VCFX_fasta_converter (vcfx_amd/csrc/tools/fa_host.h) as a program of its
// own, built under ASan + UBSan (make build/san/host_fa_asan; tests/test_host_fa.py): the names of
// "#CHROM" lines held in heap blocks of exactly their size (a read past the line is a sanitizer
// report), and the text layout's row offsets against a byte-by-byte count.  Prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "fa_host.h"

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

// the line in a heap block of exactly its bytes
static std::vector<std::string> names_of(const std::string &line, std::vector<std::string> have = {}) {
    std::unique_ptr<char[]> p(new char[line.size() ? line.size() : 1]);
    memcpy(p.get(), line.data(), line.size());
    fa_names(p.get(), line.size(), have);
    return have;
}

static void name_lines() {
    const std::string head = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
    struct Case {
        const char *tail;
        std::vector<std::string> names;
    };
    const Case cases[] = {
        {"", {}},
        {"\t", {}},
        {"\tS1", {"S1"}},
        {"\tS1\t", {"S1"}},
        {"\tS1\tS2", {"S1", "S2"}},
        {"\tS1\t\tS3", {"S1", "", "S3"}},
        {"\t\t", {""}},
        {"\t\t\t", {"", ""}},
        {"\tS1\r", {"S1\r"}},
        {"\tS1\tS2\r", {"S1", "S2\r"}},
        {"\t\r", {"\r"}},
        {"\tname with spaces\t>odd", {"name with spaces", ">odd"}},
    };
    for (const Case &c : cases) CHECK(names_of(head + c.tail) == c.names);
    CHECK(names_of("#CHROM").empty());
    CHECK(names_of("").empty());
    CHECK(names_of("#CHROM\t\t\t\t\t\t\t\t\tX") == std::vector<std::string>{"X"});
    CHECK(names_of("a\tb\tc\td\te\tf\tg\th\ti\tj\tk") == (std::vector<std::string>{"j", "k"}));
    // a second line appends
    CHECK(names_of(head + "\tB", {"A"}) == (std::vector<std::string>{"A", "B"}));
}

static void layouts() {
    for (uint64_t cols : {0ull, 1ull, 59ull, 60ull, 61ull, 119ull, 120ull, 121ull, 240ull, 1000ull}) {
        uint64_t want = 0;  // a byte per base, a '\n' after every 60th and after the last
        for (uint64_t c = 0; c < cols; c++) want += 1 + ((c % VCFXG_FA_LINE == VCFXG_FA_LINE - 1 || c + 1 == cols) ? 1 : 0);
        CHECK(FaLayout::row_bytes(cols) == want);
    }
    FaLayout lay;
    lay.make(0, 10, {});
    CHECK(lay.bytes() == 0 && lay.row_off.size() == 1 && !lay.skip_of(0));
    lay.make(3, 61, {});
    CHECK(lay.row_off == (std::vector<uint64_t>{0, 63, 126, 189}) && !lay.any_skip && !lay.skip_of(3));
    lay.make(4, 61, {0, 0, 1, 61});  // the last sample was named after every column
    CHECK(lay.row_off == (std::vector<uint64_t>{0, 63, 126, 187, 187}) && lay.any_skip);
    CHECK(!lay.skip_of(2) && lay.skip_of(3) == lay.skip.data() && lay.skip_of(100) == lay.skip.data());
    lay.make(2, 5, {0, 9});  // (a skip past the columns is the columns)
    CHECK(lay.skip[1] == 5 && lay.bytes() == 6);
    lay.make(3, 120, {7});  // fewer entries than samples: the rest skip nothing
    CHECK(lay.skip == (std::vector<uint64_t>{7, 0, 0}) && lay.row_off[1] == 113 + 2 && lay.bytes() == 115 + 2 * 122);
}

int main() {
    name_lines();
    layouts();
    printf("ok %ld\n", checks);
    return 0;
}
