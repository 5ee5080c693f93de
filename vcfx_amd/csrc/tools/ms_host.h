// ms_host.h -- the host side of VCFX_multiallelic_splitter that needs no device: the header table
// (parseHeaderLine, VCFX_multiallelic_splitter.cpp:226-245; parseNumberEq :61-76) and the walk that
// interleaves the lines the host copies with the rows the device wrote.  Header only, so the
// stand-alone check (tests/host_ms_test.cpp) compiles exactly what the tool runs.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "vcfx_gpu.h"

namespace vcfxh {

struct MsDecl {
    std::string id;
    uint8_t section, number;
};

// [p, p + n) found in [s, s + len): its offset, or -1
inline long ms_find(const char *s, size_t len, const char *p, size_t n) {
    for (size_t i = 0; i + n <= len; i++)
        if (!memcmp(s + i, p, n)) return (long)i;
    return -1;
}

// A "##INFO=" / "##FORMAT=" line [ls, ls + len): ID = the text after the first "ID=" up to ',' or
// '>', Number = the text after the first "Number=" up to ',' or '>'; a line that lacks either, or
// either's end, declares nothing.  Appends the declaration (the caller's table is in header order:
// the last entry of an ID wins).
inline bool ms_parse_header_line(const char *ls, size_t len, std::vector<MsDecl> &out) {
    uint8_t section;
    if (len >= 7 && !memcmp(ls, "##INFO=", 7)) section = VCFXG_MS_INFO;
    else if (len >= 9 && !memcmp(ls, "##FORMAT=", 9)) section = VCFXG_MS_FORMAT;
    else return false;
    auto value = [&](const char *tag, size_t tn, std::string &v) {
        const long i = ms_find(ls, len, tag, tn);
        if (i < 0) return false;
        const char *p = ls + i + tn, *end = ls + len, *e = p;
        while (e < end && *e != ',' && *e != '>') e++;
        if (e == end) return false;
        v.assign(p, e);
        return true;
    };
    std::string id, num;
    if (!value("ID=", 3, id) || !value("Number=", 7, num)) return false;
    const uint8_t number = num == "A"   ? VCFXG_MS_NUM_A
                           : num == "R" ? VCFXG_MS_NUM_R
                           : num == "G" ? VCFXG_MS_NUM_G
                                        : VCFXG_MS_NUM_OTHER;
    out.push_back(MsDecl{id, section, number});
    return true;
}

inline std::vector<vcfxg_ms_entry> ms_entries(const std::vector<MsDecl> &d) {
    std::vector<vcfxg_ms_entry> e(d.size());
    for (size_t i = 0; i < d.size(); i++) e[i] = vcfxg_ms_entry{d[i].id.data(), (uint32_t)d[i].id.size(), d[i].section, d[i].number};
    return e;
}

// The lines of one device block in order (Walk: LineWalk's next() / v / bytes() / len()), line k
// of the block with the rows text[off[k], off[k + 1]): header and copied lines leave as ranges of
// the input (a last line without '\n' gets one), a split line's rows from the device text, an
// empty line as "\n" in stdin mode and not at all in file mode.  False when a line's bytes could
// not be read.
template <typename Walk, typename Emitter>
bool ms_write_block(Walk &w, Emitter &em, bool stdin_mode, const uint64_t *off, const char *text) {
    for (size_t k = 0; w.next(); k++) {
        if (w.v == VCFXG_MS_EMPTY) {
            if (stdin_mode) em.raw("\n", 1);
        } else if (w.v == VCFXG_MS_SPLIT) {
            em.raw(text + off[k], (size_t)(off[k + 1] - off[k]));
        } else {
            const char *a = w.bytes();
            if (!a) return false;
            em.line(a, a + w.len());
        }
    }
    return true;
}

}  // namespace vcfxh
