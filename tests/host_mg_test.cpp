// The host-only code of VCFX_merger (vcfx_amd/csrc/tools/mg_host.h) as a program of its own, built
// under ASan + UBSan (make build/san/host_mg_asan; tests/test_host_mg.py): K files as the one text
// the device indexes, each file held in a heap block of exactly its size (a read past it is a
// sanitizer report), the split of -m values, and the walk over the text blocks against a stand-in
// for vcfxg_merge_text that cuts the lines into blocks of a given size.  Prints "ok <checks>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "mg_host.h"
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
        std::vector<std::string> files;
        std::string text;
        std::vector<uint64_t> start;
        int chunks;
    };
    const Case cases[] = {
        {{}, "", {0}, 1},
        {{""}, "", {0, 0}, 1},
        {{"", "", ""}, "", {0, 0, 0, 0}, 1},
        {{"a\n"}, "a\n", {0, 2}, 1},
        {{"a"}, "a\n", {0, 2}, 2},
        {{"a", "b", "c"}, "a\nb\nc\n", {0, 2, 4, 6}, 6},
        {{"a\n", "b", "c\n"}, "a\nb\nc\n", {0, 2, 4, 6}, 4},
        {{"", "b", ""}, "b\n", {0, 0, 2, 2}, 2},
        {{"a\n", "", "c"}, "a\nc\n", {0, 2, 2, 4}, 3},
        {{"a\r", "b"}, "a\r\nb\n", {0, 3, 5}, 4},
        {{"\n", "\n", "\n\n"}, "\n\n\n\n", {0, 1, 2, 4}, 3},
        {{"#h\n1\t5\t.", "#h\n1\t5\t.\n", "x"}, "#h\n1\t5\t.\n#h\n1\t5\t.\nx\n", {0, 9, 18, 20}, 5},
        {{"\xff\n", "\x80"}, "\xff\n\x80\n", {0, 2, 4}, 3},
    };
    for (const Case &c : cases) {
        std::vector<std::unique_ptr<char[]>> held;
        MgJoin J;
        for (const std::string &f : c.files) {
            held.push_back(block(f));
            J.add(held.back().get(), f.size());
        }
        J.finish();
        CHECK(J.files() == c.files.size());
        CHECK(J.start == c.start);
        CHECK(J.total == c.text.size());
        CHECK((int)J.chunk.size() == c.chunks);
        std::string text;
        for (size_t i = 0; i < J.chunk.size(); i++) {
            CHECK(J.chunk[i].final_chunk == (i + 1 == J.chunk.size() ? 1 : 0));
            if (J.chunk[i].n) text.append(J.chunk[i].p, J.chunk[i].n);
        }
        CHECK(text == c.text);
    }
    // a NUL is a byte like any other; many files
    const std::string nul("x\0y", 3);
    std::vector<std::unique_ptr<char[]>> held;
    MgJoin J;
    std::string want;
    for (int i = 0; i < 65; i++) {
        const std::string f = i % 3 == 0 ? std::string() : i % 3 == 1 ? nul : nul + "\n";
        held.push_back(block(f));
        J.add(held.back().get(), f.size());
        CHECK(J.start.back() == want.size());
        if (!f.empty()) want += nul + "\n";
    }
    J.finish();
    CHECK(J.files() == 65 && J.total == want.size() && J.start.back() == want.size());
    std::string text;
    for (const MgChunk &k : J.chunk)
        if (k.n) text.append(k.p, k.n);
    CHECK(text == want);
}

static void splits() {
    struct Split {
        std::string value;
        std::vector<std::string> names;
    };
    const Split splits[] = {
        {"", {""}},
        {"a", {"a"}},
        {"a,b", {"a", "b"}},
        {"a,,b", {"a", "", "b"}},
        {",", {"", ""}},
        {",,", {"", "", ""}},
        {"a,", {"a", ""}},
        {",a", {"", "a"}},
        {"dir/a.vcf,dir/b.vcf.gz,c", {"dir/a.vcf", "dir/b.vcf.gz", "c"}},
    };
    std::vector<std::string> all, want;
    for (const Split &s : splits) {
        std::vector<std::string> names;
        const std::unique_ptr<char[]> held = block(s.value);
        mg_split(std::string(held.get() ? held.get() : "", s.value.size()), names);
        CHECK(names == s.names);
        mg_split(s.value, all);  // two -m options add up
        want.insert(want.end(), s.names.begin(), s.names.end());
        CHECK(all == want);
    }
}

// the walk over blocks of at most `per` lines of `lines` output lines; a stand-in that fails, stalls
// or overruns ends it as a failure
static void walks() {
    for (uint64_t lines : {0ull, 1ull, 2ull, 7ull, 64ull, 100ull})
        for (uint64_t per : {1ull, 2ull, 7ull, 1000ull}) {
            uint64_t next = 0, calls = 0, written = 0;
            const bool ok = write_text_blocks(
                lines,
                [&](uint64_t first, uint64_t *taken, uint64_t *bytes) {
                    CHECK(first == next);
                    *taken = per < lines - first ? per : lines - first;
                    *bytes = 10 * *taken;
                    next += *taken;
                    calls++;
                    return true;
                },
                [&](uint64_t bytes) {
                    written += bytes;
                    return true;
                });
            CHECK(ok && next == lines && written == 10 * lines && calls == (lines + per - 1) / per);
        }
    CHECK(!write_text_blocks(3, [](uint64_t, uint64_t *, uint64_t *) { return false; }, [](uint64_t) { return true; }));
    CHECK(!write_text_blocks(3, [](uint64_t, uint64_t *t, uint64_t *) { *t = 0; return true; }, [](uint64_t) { return true; }));
    CHECK(!write_text_blocks(3, [](uint64_t, uint64_t *t, uint64_t *) { *t = 4; return true; }, [](uint64_t) { return true; }));
    CHECK(!write_text_blocks(3, [](uint64_t, uint64_t *t, uint64_t *) { *t = 1; return true; }, [](uint64_t) { return false; }));
    CHECK(write_text_blocks(0, [](uint64_t, uint64_t *, uint64_t *) { return false; }, [](uint64_t) { return false; }));
}

int main() {
    joins();
    splits();
    walks();
    printf("ok %ld\n", checks);
    return 0;
}
