// The host-only code of VCFX_diff_tool (vcfx_amd/csrc/tools/df_host.h) as a program of its own,
// built under ASan + UBSan (make build/san/host_df_asan; tests/test_host_df.py): the two files as
// the one text the device indexes, each file held in a heap block of exactly its size (a read past
// it is a sanitizer report), and the walk over a side's text blocks against a stand-in for
// vcfxg_diff_text that cuts the keys into blocks of a given size.  Prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "df_host.h"
#include "tools.h"

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

// the file in a heap block of exactly its bytes (an empty file: no block at all)
static std::unique_ptr<char[]> block(const std::string &s) {
    if (s.empty()) return nullptr;
    std::unique_ptr<char[]> p(new char[s.size()]);
    memcpy(p.get(), s.data(), s.size());
    return p;
}

static void joins() {
    struct Case {
        std::string a, b, text;
        uint64_t second;
        int chunks;
    };
    const std::string nul("x\0y\n", 4);
    const Case cases[] = {
        {"", "", "", 0, 1},
        {"", "b\n", "b\n", 0, 1},
        {"", "b", "b", 0, 1},
        {"a\n", "", "a\n", 2, 2},
        {"a", "", "a\n", 2, 3},
        {"a\n", "b\n", "a\nb\n", 2, 2},
        {"a", "b", "a\nb", 2, 3},
        {"a\r", "b", "a\r\nb", 3, 3},
        {"\n", "\n", "\n\n", 1, 2},
        {"\n\n", "x", "\n\nx", 2, 2},
        {"#h\n1\t5\t.\tA\tT", "#h\n1\t5\t.\tA\tT\n", "#h\n1\t5\t.\tA\tT\n#h\n1\t5\t.\tA\tT\n", 13, 3},
        {nul, nul, nul + nul, 4, 2},
        {std::string("\xff\n", 2), std::string("\x80", 1), std::string("\xff\n\x80", 3), 2, 2},
    };
    for (const Case &c : cases) {
        const auto pa = block(c.a), pb = block(c.b);
        DfJoin J;
        J.make(pa.get(), c.a.size(), pb.get(), c.b.size());
        CHECK(J.chunks == c.chunks);
        CHECK(J.second_start == c.second);
        CHECK(J.total == c.text.size());
        std::string got;
        for (int i = 0; i < J.chunks; i++) {
            CHECK((J.chunk[i].final_chunk != 0) == (i == J.chunks - 1));
            CHECK(J.chunk[i].n || i == J.chunks - 1);  // only the final chunk may be empty
            if (J.chunk[i].n) got.append(J.chunk[i].p, J.chunk[i].n);
        }
        CHECK(got == c.text);
        // file 2 begins a line: the text's first byte, or the byte after a '\n'
        CHECK(J.second_start == 0 || c.text[J.second_start - 1] == '\n');
        CHECK(got.substr(J.second_start) == c.b);
    }
    // a large file 1 without its last newline: three chunks, the middle one the one byte
    std::string big(1 << 20, 'k');
    const auto pa = block(big), pb = block("z");
    DfJoin J;
    J.make(pa.get(), big.size(), pb.get(), 1);
    CHECK(J.chunks == 3 && J.chunk[1].n == 1 && J.chunk[1].p[0] == '\n' && J.second_start == big.size() + 1);
}

// vcfxg_diff_text's contract: from key `first`, as many keys as fit `cap` bytes, one at least
struct Side {
    std::vector<std::string> keys;
    uint64_t cap;
    std::string written, text;
    int calls = 0;
    bool operator()(uint64_t first, uint64_t *taken, uint64_t *bytes) {
        calls++;
        text.clear();
        uint64_t k = 0;
        while (first + k < keys.size() && (k == 0 || text.size() + keys[first + k].size() + 1 <= cap)) {
            text += keys[first + k] + "\n";
            k++;
        }
        *taken = k;
        *bytes = text.size();
        return true;
    }
};

static void walks() {
    std::vector<std::string> keys;
    for (int i = 0; i < 300; i++) keys.push_back("1:" + std::to_string(i * 7) + ":A:" + std::string((size_t)(i % 40), 'T'));
    std::string all;
    for (auto &k : keys) all += k + "\n";
    for (uint64_t cap : {1ull, 8ull, 64ull, 100ull, 4096ull, 1ull << 30}) {
        Side s{keys, cap};
        const bool ok = write_text_blocks(keys.size(), [&](uint64_t f, uint64_t *t, uint64_t *b) { return s(f, t, b); },
                                     [&](uint64_t bytes) {
                                         CHECK(bytes == s.text.size());
                                         s.written += s.text;
                                         return true;
                                     });
        CHECK(ok);
        CHECK(s.written == all);
        CHECK(cap >= 64 || s.calls == (int)keys.size());
        CHECK(cap < (1ull << 30) || s.calls == 1);
    }
    // no key: no call at all
    int calls = 0;
    CHECK(write_text_blocks(0, [&](uint64_t, uint64_t *, uint64_t *) { return ++calls, true; }, [&](uint64_t) { return ++calls, true; }));
    CHECK(calls == 0);
    // a failed call, a failed write, a block of no key and a block past the end all stop the walk
    CHECK(!write_text_blocks(5, [&](uint64_t, uint64_t *, uint64_t *) { return false; }, [&](uint64_t) { return true; }));
    calls = 0;
    CHECK(!write_text_blocks(5, [&](uint64_t, uint64_t *t, uint64_t *) { return *t = 1, true; }, [&](uint64_t) { return ++calls < 3; }));
    CHECK(calls == 3);
    calls = 0;
    CHECK(!write_text_blocks(5, [&](uint64_t, uint64_t *t, uint64_t *) { return ++calls, *t = 0, true; }, [&](uint64_t) { return true; }));
    CHECK(calls == 1);
    CHECK(!write_text_blocks(5, [&](uint64_t f, uint64_t *t, uint64_t *) { return *t = f ? 4 : 2, true; }, [&](uint64_t) { return true; }));
    CHECK(write_text_blocks(5, [&](uint64_t f, uint64_t *t, uint64_t *) { return *t = f ? 3 : 2, true; }, [&](uint64_t) { return true; }));
}

int main() {
    joins();
    walks();
    printf("ok %ld\n", checks);
    return 0;
}
