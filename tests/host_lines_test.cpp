// host_lines_test.cpp -- the drop-ins' shared reader (vcfx_amd/csrc/host/emit.h: input_copy,
// LineSource, LineWalk, line_copy, Lines) without a device: built with the real hostio.cpp /
// gz.cpp and the host stand-in for the device library (tests/shard_tsan_stub.cpp, which keeps the
// loaded bytes and answers vcfxg_index / vcfxg_line_ends / vcfxg_fetch_lines / vcfxg_input_fetch
// over them), plain and under ASan + UBSan (`make sanitize`; tests/test_host_lines.py runs both
// with VCFX_WINDOW_BYTES = 16, 1024 and unset).
//
// Every input is given to the reader in its three forms, each part in a heap block of its exact
// size so that a read past a part is a sanitizer report:
//   host    host_n == n: all bytes on the host
//   view    bytes [h, n) at Input::tail (h at a line start, as a shard view's header part ends)
//   device  host_n = h < n and no tail: bytes [h, n) only in the stand-in's "device" buffer
// and every line, status and range the reader hands out is checked against a plain split of the
// bytes on '\n'.  Prints "ok <checks>" and exits 0, or the first difference and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <memory>
#include <string>
#include <vector>

#include "emit.h"
#include "hostio.h"

using namespace vcfxh;

extern "C" {
extern size_t vcfxg_stub_input_fetches;
extern uint64_t vcfxg_stub_max_block;
}

namespace {

size_t g_checks = 0;
std::string g_what;  // the input and form under test

#define CHECK(c)                                                                         \
    do {                                                                                 \
        g_checks++;                                                                      \
        if (!(c)) {                                                                      \
            fprintf(stderr, "%s: line %d: %s\n", g_what.c_str(), __LINE__, #c);          \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

// what a LineEmitter wrote: a memory file read back and emptied
struct Sink {
    int fd = memfd_create("host_lines", 0);
    std::string take() {
        const off_t n = lseek(fd, 0, SEEK_END);
        std::string s((size_t)n, '\0');
        if (n && pread(fd, &s[0], (size_t)n, 0) != n) exit(2);
        if (ftruncate(fd, 0) != 0 || lseek(fd, 0, SEEK_SET) != 0) exit(2);
        return s;
    }
};

enum Form { kHost, kView, kDevice };
const char *kFormName[] = {"host", "view", "device"};

struct Built {
    Input in;
    std::unique_ptr<char[]> head, tail;
    vcfxg_ctx *g = nullptr;
};

// B with its first h bytes as the host part, in the given form, loaded on the stand-in
void build(Built &x, const std::string &B, size_t h, Form f) {
    const size_t n = B.size();
    if (f == kHost) h = n;
    x.head.reset(new char[h]);
    memcpy(x.head.get(), B.data(), h);
    x.in.p = x.head.get();
    x.in.n = n;
    x.in.host_n = h;
    x.g = gpu(2);
    if (!x.g) exit(2);
    if (f == kView) {
        x.tail.reset(new char[n - h]);
        memcpy(x.tail.get(), B.data() + h, n - h);
        x.in.tail = x.tail.get();
    } else if (f == kDevice) {  // as read_fd(host_copy = false) leaves it: streamed, the last chunk open
        if (vcfxg_ingest_begin(x.g, n) != VCFXG_OK || vcfxg_ingest(x.g, B.data(), n, 0) != VCFXG_OK) exit(2);
        x.in.stream_ctx = x.g;
        x.in.streamed = n;
    }
}

struct Span {
    size_t a, b;  // a line: bytes [a, b), its '\n' at b when b < n
};
std::vector<Span> split(const std::string &B, size_t from) {
    std::vector<Span> v;
    for (size_t p = from; p < B.size();) {
        const size_t e = std::min(B.find('\n', p), B.size());
        v.push_back({p, e});
        p = e + 1;
    }
    return v;
}

void check_form(const std::string &B, size_t h, Form f, bool big) {
    g_what = g_what.substr(0, g_what.find(" /")) + " / " + kFormName[f] + " h=" + std::to_string(h);
    const size_t n = B.size();
    Built x;
    build(x, B, h, f);
    const Input &in = x.in;
    const std::vector<Span> all = split(B, 0);

    // Lines: every line of the input from byte 0 on (of a big input the first 2000: a line past
    // the host part costs a 64 KiB fetch)
    {
        Lines L(in, 2);
        size_t pos = 0, next = 0, k = 0;
        const char *ls, *le;
        while ((!big || k < 2000) && L.at(pos, ls, le, next)) {
            CHECK(k < all.size() && pos == all[k].a);
            CHECK((size_t)(le - ls) == all[k].b - all[k].a && memcmp(ls, B.data() + pos, (size_t)(le - ls)) == 0);
            CHECK(next == std::min(all[k].b + 1, n));
            pos = next;
            k++;
        }
        CHECK(!L.failed && (big || (k == all.size() && pos == n)));
        CHECK(L.device() && L.g == x.g);  // (loads the input: the device form's ingest completes here)
    }
    vcfxg_ctx *g = x.g;
    Sink sink;

    // ranges: input_copy, LineSource::put, and the last byte
    {
        std::vector<Span> rs = {{0, n}, {h / 2, h + (n - h) / 2}};
        if (!big) rs.insert(rs.end(), {{0, 0}, {n, n}, {h, n}, {0, h}});
        uint64_t r = 12345;
        for (int t = 0; t < 6 && n && !big; t++) {
            r = r * 6364136223846793005ull + 1442695040888963407ull;
            const size_t a = (size_t)((r >> 33) % (n + 1));
            r = r * 6364136223846793005ull + 1442695040888963407ull;
            const size_t b = a + (size_t)((r >> 33) % (n - a + 1));
            rs.push_back({a, b});
        }
        std::string got, want_all;
        LineEmitter em(in.p, in.host_n, sink.fd);
        LineSource src(in, g, em);
        for (const Span &s : rs) {
            got.assign(s.b - s.a, '?');
            CHECK(input_copy(in, g, s.a, s.b, &got[0]) == VCFXG_OK && got == B.substr(s.a, s.b - s.a));
            CHECK(src.put(s.a, s.b));
            want_all += B.substr(s.a, s.b - s.a);
        }
        em.finish();
        CHECK(src.ok && sink.take() == want_all);
        if (n) {
            char last = 0;
            CHECK(input_copy(in, g, n - 1, n, &last) == VCFXG_OK && last == B[n - 1]);
        }
    }

    // the walk, over an index from byte 0 and from the second line's start
    for (size_t ds : {(size_t)0, all.size() > 1 ? all[1].a : n}) {
        if (ds > in.host_n || (big && ds)) continue;  // (the tools index from within the host part)
        const std::vector<Span> want = split(B, ds);
        uint64_t nl = 0;
        CHECK(vcfxg_index(g, ds, &nl) == VCFXG_OK && nl == want.size());
        // line_copy: the first, a middle and the last line
        for (size_t l : {(size_t)0, want.size() / 2, want.size() - 1}) {
            if (l >= want.size()) continue;
            std::string line = "?";
            CHECK(line_copy(in, g, ds, l, line, 2) && line == B.substr(want[l].a, want[l].b - want[l].a));
        }
        // no bytes asked for: no line is fetched
        {
            LineEmitter em(in.p, in.host_n, sink.fd);
            const size_t f0 = vcfxg_stub_input_fetches;
            LineWalk w(in, g, em, ds, nl, 2, line_status(g, 2));
            size_t k = 0;
            while (w.next()) {
                CHECK(k < want.size() && w.a == want[k].a && w.b == want[k].b);
                CHECK(w.v == (want[k].b - want[k].a) % 4);
                k++;
            }
            CHECK(k == want.size() && w.finish() && vcfxg_stub_input_fetches == f0 && sink.take().empty());
        }
        // statuses and a second per-line array through the caller's callable; status 1 and 2: the
        // line and a '\n'; 3: its bytes as they are; 0: dropped, never fetched
        {
            std::string expect;
            for (const Span &s : want) {
                const size_t v = (s.b - s.a) % 4;
                if (v == 1 || v == 2) expect.append(B, s.a, s.b - s.a).push_back('\n');
                else if (v == 3) expect.append(B, s.a, std::min(s.b + 1, n) - s.a);
            }
            LineEmitter em(in.p, in.host_n, sink.fd);
            std::vector<int32_t> len;
            LineWalk w(in, g, em, ds, nl, 2, [&](uint64_t first, uint64_t count, uint8_t *st) {
                len.resize(count);
                return vcfxg_fetch_lines(g, first, count, len.data(), nullptr, st) == VCFXG_OK;
            });
            size_t k = 0;
            while (w.next()) {
                CHECK(k < want.size() && w.a == want[k].a && w.b == want[k].b && w.len() == w.b - w.a);
                CHECK(w.v == w.len() % 4 && (size_t)len[w.k] == w.len());
                k++;
                if (w.v == 0) continue;
                const char *p = w.bytes();
                CHECK(p && memcmp(p, B.data() + w.a, w.len()) == 0);
                CHECK(w.b == n || p[w.len()] == '\n');
                if (w.v == 3) em.bytes(p, p + w.len() + (w.b < n ? 1 : 0));
                else em.line(p, p + w.len());
            }
            CHECK(k == want.size() && w.finish());
            CHECK(sink.take() == expect);
        }
        CHECK(vcfxg_stub_max_block <= LineWalk::kBlock);
    }
    close(sink.fd);
}

// one input in every form and at several splits
void check(const char *name, const std::string &B, bool big = false) {
    g_what = name;
    const size_t n = B.size();
    const std::vector<Span> all = split(B, 0);
    check_form(B, n, kHost, big);
    // device: a split anywhere (lines straddle it); view: at line starts
    std::vector<size_t> dev = {n / 2}, view;
    if (!big) {
        dev.push_back(0);
        view = {0, n};
        if (n) dev.push_back(n - 1);
    }
    if (n > 1) dev.push_back(1);
    if (all.size() > 1) {
        view.push_back(all[all.size() / 2].a);
        dev.push_back(all[all.size() / 2].a);
        if (!big) {
            view.push_back(all[1].a);
            view.push_back(all.back().a);
            dev.push_back(all.back().a);
            if (all.back().a < n) dev.push_back(all.back().a + 1);
        }
    }
    for (size_t h : view) check_form(B, h, kView, big);
    for (size_t h : dev)
        if (h < n) check_form(B, h, kDevice, big);
}

std::string rep(const char *s, size_t k) {
    std::string r;
    r.reserve(strlen(s) * k);
    for (size_t i = 0; i < k; i++) r += s;
    return r;
}

}  // namespace

int main() {
    check("empty", "");
    check("a", "a");
    check("newline", "\n");
    check("newlines", "\n\n\n\n\n");
    check("crlf", "#h\r\nab\r\n\r\ncde\r\nf\r\n");
    check("no final newline", "#h\n1\tx\n22\ty\nlast line without a newline");
    check("mixed", "##a\n#CHROM\tS1\n\n1\t5\t.\n\n\n2\t77\tid\tA\tC\n3\n");
    // the edge of Lines' 64 KiB fetch
    check("64KiB lines", "h\n" + std::string(65535, 'p') + "\n" + std::string(65536, 'q') + "\n" + std::string(65537, 'r') +
                             "\nz\n");
    // the window: a line longer than it, and lines that end just before, at and after its end
    const size_t W = window_bytes();
    if (W <= (1u << 20)) {
        std::string b = "hd\n";
        for (size_t len : {W - 2, W - 1, W, W + 1, 3 * W + 1, W - 1, (size_t)1, W - 3, W})
            b += std::string(len, 'w') + "\n";
        check("window edges", b);
        check("window edges, open end", b + std::string(W - 1, 'e'));
    }
    // the walk's block edge
    for (size_t lines : {(size_t)(1u << 20) - 1, (size_t)1u << 20, (size_t)(1u << 20) + 1})
        check(("x lines " + std::to_string(lines)).c_str(), rep("x\n", lines), true);
    gpu_join();
    printf("ok %zu\n", g_checks);
    return 0;
}
