// hx_host.h -- the host side of VCFX_haplotype_extractor that needs no device: the sample names of the
// "#CHROM" line (parseHeader, VCFX_haplotype_extractor.cpp:268-285), std::stoi for -b (:862), what a
// header line is in each mode (:605-630, :738-754), and the texts the host formats from the lines it
// holds: the header row, the "not phased" warning and the -c -d stream (phaseIsConsistent :303-349),
// which the device's block decisions and first-flip index drive.  Plain C++: tests/host_hx_test.cpp
// builds it under ASan + UBSan without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace vcfxh {

// the line [s, s + n) without one trailing '\r'
inline size_t hx_strip(const char *s, size_t n) { return n && s[n - 1] == '\r' ? n - 1 : n; }

enum HxHead { kHxSkip, kHxChrom, kHxData };
// a raw line before the data part: skipped (empty; in file mode also '\r' alone; a '#' line), a
// "#CHROM" line, or the first data line (on stdin a line of '\r' alone is one: the test for empty
// comes before the strip, :739-744)
inline HxHead hx_head_line(const char *s, size_t n, bool stdin_mode) {
    if (!n) return kHxSkip;
    const size_t m = hx_strip(s, n);
    if (!m) return stdin_mode ? kHxData : kHxSkip;
    if (s[0] != '#') return kHxData;
    return m >= 6 && !memcmp(s, "#CHROM", 6) ? kHxChrom : kHxSkip;
}

// fields 10 onward of the (stripped) line; false when it has nine fields or fewer.  Every tab ends a
// field, and a line that ends in a tab has an empty last field (splitTabsView :217-232)
inline bool hx_names(const char *s, size_t n, std::vector<std::string> &names) {
    names.clear();
    size_t p = 0, col = 0;
    for (;;) {
        size_t e = p;
        while (e < n && s[e] != '\t') e++;
        if (col >= 9) names.emplace_back(s + p, e - p);
        col++;
        if (e >= n) break;
        p = e + 1;
    }
    return col > 9;
}

// std::stoi(text): white space, a sign, digits (what follows them is ignored); false where it throws
inline bool hx_stoi(const char *t, int &out) {
    while (*t == ' ' || (*t >= '\t' && *t <= '\r')) t++;
    bool neg = false;
    if (*t == '+' || *t == '-') neg = *t++ == '-';
    if (*t < '0' || *t > '9') return false;
    int64_t v = 0;
    for (; *t >= '0' && *t <= '9'; t++) {
        v = v * 10 + (*t - '0');
        if (v > 2147483648ll) return false;
    }
    v = neg ? -v : v;
    if (v > 2147483647ll || v < -2147483648ll) return false;
    out = (int)v;
    return true;
}

inline std::string hx_header_row(const std::vector<std::string> &names) {
    std::string r = "CHROM\tSTART\tEND";
    for (const std::string &s : names) {
        r += '\t';
        r += s;
    }
    r += '\n';
    return r;
}

// "Warning: Not all samples phased at CHROM:POS." for the (stripped) line
inline void hx_warn_unphased(const char *s, size_t n, int64_t pos, std::string &out) {
    size_t e = 0;
    while (e < n && s[e] != '\t') e++;
    out += "Warning: Not all samples phased at ";
    out.append(s, e);
    out += ':';
    out += std::to_string(pos);
    out += ".\n";
}

// the GT sub-fields of a member's (stripped) line as (offset, length) pairs, for the debug stream only
// (findGTIndex :174-193, extractNthField :196-214); false when the line is no member's
inline bool hx_gts(const char *s, size_t n, size_t ns, std::vector<std::pair<uint32_t, uint32_t>> &out) {
    out.clear();
    std::vector<size_t> tabs;
    for (size_t p = 0; p < n && tabs.size() < 9 + ns; p++)
        if (s[p] == '\t') tabs.push_back(p);
    if (tabs.size() < 8 + ns) return false;
    int gi = -1, idx = 0;
    for (size_t a = tabs[7] + 1, p = a;; p++) {
        if (p == tabs[8] || s[p] == ':') {
            if (p - a == 2 && s[a] == 'G' && s[a + 1] == 'T') {
                gi = idx;
                break;
            }
            idx++;
            a = p + 1;
        }
        if (p == tabs[8]) break;
    }
    if (gi < 0) return false;
    for (size_t k = 0; k < ns; k++) {
        size_t p = tabs[8 + k] + 1;
        const size_t e = 9 + k < tabs.size() ? tabs[9 + k] : n;
        int f = 0;
        while (f < gi && p < e) {
            if (s[p] == ':') f++;
            p++;
        }
        if (f < gi) return false;
        size_t q = p;
        while (q < e && s[q] != ':') q++;
        out.emplace_back((uint32_t)p, (uint32_t)(q - p));
    }
    return true;
}

// the -c -d stream of one pair that passed the CHROM and distance test: the previous member's line and
// GTs, the new member's, and the device's answer (flip = the first flipping sample, ns: none)
inline void hx_debug_pair(const char *prev, const std::vector<std::pair<uint32_t, uint32_t>> &pg, const char *cur,
                          const std::vector<std::pair<uint32_t, uint32_t>> &cg, uint32_t flip, std::string &out) {
    out += "Checking phase consistency\n";
    const size_t ns = cg.size() < pg.size() ? cg.size() : pg.size();
    for (size_t s = 0; s < ns; s++) {
        out += "Sample " + std::to_string(s) + " last GT: ";
        out.append(prev + pg[s].first, pg[s].second);
        out += " new GT: ";
        out.append(cur + cg[s].first, cg[s].second);
        out += '\n';
        if (pg[s].second >= 3 && cg[s].second >= 3) {
            out += "Comparing alleles: ";
            out += prev[pg[s].first];
            out += '|';
            out += prev[pg[s].first + pg[s].second - 1];
            out += " vs ";
            out += cur[cg[s].first];
            out += '|';
            out += cur[cg[s].first + cg[s].second - 1];
            out += '\n';
        }
        if (s == flip) {
            out += "Phase flip detected in sample " + std::to_string(s) + "\n";
            return;
        }
    }
    out += "All phases consistent\n";
}

}  // namespace vcfxh
