// The host-only code of VCFX_multiallelic_splitter (vcfx_amd/csrc/tools/ms_host.h) as a program of
// its own, built under ASan + UBSan (make build/san/host_ms_asan; tests/test_host_ms.py): the
// header-table parse on lines held in heap blocks of exactly their size (a read past the line is
// a sanitizer report), and the walk that interleaves copied lines with the device's rows, over a
// stand-in walk and a stand-in emitter.  Prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "ms_host.h"

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
static bool parse(const std::string &line, std::vector<MsDecl> &out) {
    std::unique_ptr<char[]> p(new char[line.size() ? line.size() : 1]);
    memcpy(p.get(), line.data(), line.size());
    return ms_parse_header_line(p.get(), line.size(), out);
}

static void header_lines() {
    struct Case {
        const char *line;
        bool ok;
        const char *id;
        int section, number;
    };
    const Case cases[] = {
        {"##INFO=<ID=AF,Number=A,Type=Float,Description=\"f\">", true, "AF", VCFXG_MS_INFO, VCFXG_MS_NUM_A},
        {"##FORMAT=<ID=AD,Number=R,Type=Integer>", true, "AD", VCFXG_MS_FORMAT, VCFXG_MS_NUM_R},
        {"##FORMAT=<ID=PL,Number=G>", true, "PL", VCFXG_MS_FORMAT, VCFXG_MS_NUM_G},
        {"##INFO=<ID=DP,Number=1>", true, "DP", VCFXG_MS_INFO, VCFXG_MS_NUM_OTHER},
        {"##INFO=<ID=X,Number=.>", true, "X", VCFXG_MS_INFO, VCFXG_MS_NUM_OTHER},
        {"##INFO=<ID=X,Number=a>", true, "X", VCFXG_MS_INFO, VCFXG_MS_NUM_OTHER},
        {"##INFO=<ID=X,Number=A >", true, "X", VCFXG_MS_INFO, VCFXG_MS_NUM_OTHER},
        {"##INFO=<ID=X,Number=AA>", true, "X", VCFXG_MS_INFO, VCFXG_MS_NUM_OTHER},
        {"##INFO=<Number=A,ID=K4,Type=Integer>", true, "K4", VCFXG_MS_INFO, VCFXG_MS_NUM_A},
        {"##INFO=<ID=,Number=A>", true, "", VCFXG_MS_INFO, VCFXG_MS_NUM_A},
        {"##INFO=<ID=KG,Number=A,ID=KH,Number=R>", true, "KG", VCFXG_MS_INFO, VCFXG_MS_NUM_A},
        {"##INFO=ID=Q>Number=G>", true, "Q", VCFXG_MS_INFO, VCFXG_MS_NUM_G},
        {"##INFO=<ID=K3,Type=Integer>", false, "", 0, 0},
        {"##INFO=<Number=A,Type=Integer>", false, "", 0, 0},
        {"##INFO=<ID=K5,Number=A", false, "", 0, 0},
        {"##INFO=<ID=K5", false, "", 0, 0},
        {"##INFO=<ID=", false, "", 0, 0},
        {"##INFO=<ID=A,Number=", false, "", 0, 0},
        {"##INFO=", false, "", 0, 0},
        {"##INFO", false, "", 0, 0},
        {"##FORMAT", false, "", 0, 0},
        {"##FORMAT=", false, "", 0, 0},
        {"##", false, "", 0, 0},
        {"#", false, "", 0, 0},
        {"", false, "", 0, 0},
        {"##INFO =<ID=KA,Number=A>", false, "", 0, 0},
        {"##info=<ID=KB,Number=A>", false, "", 0, 0},
        {"#INFO=<ID=KC,Number=A>", false, "", 0, 0},
        {"##contig=<ID=KI,Number=A>", false, "", 0, 0},
        {"##FORMAT=<ID=GT,Number=1,Type=String>\r", true, "GT", VCFXG_MS_FORMAT, VCFXG_MS_NUM_OTHER},
    };
    for (const Case &c : cases) {
        std::vector<MsDecl> d;
        CHECK(parse(c.line, d) == c.ok);
        CHECK(d.size() == (c.ok ? 1u : 0u));
        if (c.ok) CHECK(d[0].id == c.id && d[0].section == c.section && d[0].number == c.number);
    }
    // every prefix of a full line parses without reading past it
    const std::string full = "##FORMAT=<ID=LONG_ID_0123456789,Number=R,Type=Integer,Description=\"x\">";
    for (size_t n = 0; n <= full.size(); n++) {
        std::vector<MsDecl> d;
        CHECK(parse(full.substr(0, n), d) == (n >= full.find(",Type")+ 1));
    }
    // the table keeps header order; its entries point at the declarations' bytes
    std::vector<MsDecl> d;
    parse("##INFO=<ID=AD,Number=G>", d);
    parse("##FORMAT=<ID=AD,Number=R>", d);
    const std::vector<vcfxg_ms_entry> e = ms_entries(d);
    CHECK(e.size() == 2 && e[0].id_len == 2 && !memcmp(e[1].id, "AD", 2));
    CHECK(e[0].section == VCFXG_MS_INFO && e[0].number == VCFXG_MS_NUM_G && e[1].section == VCFXG_MS_FORMAT &&
          e[1].number == VCFXG_MS_NUM_R);
    CHECK(ms_entries(std::vector<MsDecl>()).empty());
}

// stand-ins for LineWalk and LineEmitter over a buffer of lines
struct Walk {
    const std::string buf;
    const std::vector<uint8_t> &st;
    size_t pos = 0, i = 0, a = 0, b = 0, fail_at;
    uint8_t v = 0;
    Walk(const std::string &s, const std::vector<uint8_t> &t, size_t f = ~(size_t)0) : buf(s), st(t), fail_at(f) {}
    bool next() {
        if (pos >= buf.size()) return false;
        const size_t nl = buf.find('\n', pos);
        a = pos;
        b = nl == std::string::npos ? buf.size() : nl;
        pos = b + 1;
        v = st[i++];
        return true;
    }
    size_t len() const { return b - a; }
    const char *bytes() { return i - 1 == fail_at ? nullptr : buf.data() + a; }
};
struct Emit {
    std::string out;
    void raw(const char *p, size_t n) { out.append(p, n); }
    void line(const char *ls, const char *le) {
        out.append(ls, le);
        out.push_back('\n');
    }
};

static void interleave() {
    const std::string text = "row1a\nrow1b\nrow4a\nrow4b\nrow4c\n";
    const uint64_t off[] = {0, 0, 12, 12, 12, 30, 30, 30};
    const std::vector<uint8_t> st = {VCFXG_MS_HEADER, VCFXG_MS_SPLIT, VCFXG_MS_EMPTY, VCFXG_MS_COPY,
                                     VCFXG_MS_SPLIT, VCFXG_MS_EMPTY, VCFXG_MS_COPY};
    for (int final_newline = 0; final_newline < 2; final_newline++) {
        const std::string in = std::string("#h\nsplit one\n\ncopied\nsplit four\n\nlast") + (final_newline ? "\n" : "");
        for (int stdin_mode = 0; stdin_mode < 2; stdin_mode++) {
            Walk w(in, st);
            Emit em;
            CHECK(ms_write_block(w, em, stdin_mode != 0, off, text.data()));
            const std::string e = stdin_mode ? "\n" : "";
            CHECK(em.out == "#h\nrow1a\nrow1b\n" + e + "copied\nrow4a\nrow4b\nrow4c\n" + e + "last\n");
        }
    }
    // a block of split lines only, of none, and an empty block
    {
        const std::vector<uint8_t> s2 = {VCFXG_MS_SPLIT, VCFXG_MS_SPLIT};
        const uint64_t o2[] = {0, 12, 30};
        Walk w("x\ny", s2);
        Emit em;
        CHECK(ms_write_block(w, em, false, o2, text.data()) && em.out == text);
        const std::vector<uint8_t> s3 = {VCFXG_MS_COPY, VCFXG_MS_HEADER};
        const uint64_t o3[] = {0, 0, 0};
        Walk w3("x\n#y", s3);
        Emit e3;
        CHECK(ms_write_block(w3, e3, true, o3, nullptr) && e3.out == "x\n#y\n");
        Walk w4("", s3);
        Emit e4;
        CHECK(ms_write_block(w4, e4, true, o3, nullptr) && e4.out.empty());
    }
    // a line whose bytes cannot be read ends the walk: nothing of it is written
    {
        const std::string in = "#h\nsplit one\n\ncopied\nsplit four\n\nlast\n";
        Walk w(in, st, 3);
        Emit em;
        CHECK(!ms_write_block(w, em, true, off, text.data()) && em.out == "#h\nrow1a\nrow1b\n\n");
    }
}

int main() {
    header_lines();
    interleave();
    printf("ok %ld\n", checks);
    return 0;
}
