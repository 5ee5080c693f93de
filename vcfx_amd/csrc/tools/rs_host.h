// rs_host.h -- the host side of VCFX_region_subsampler that needs no device: the BED loader
// (loadRegions, VCFX_region_subsampler.cpp:344-381) as the flat arrays vcfxg_regions_load takes, and
// a sort_and_merge of its own (sortAndMergeIntervals :383-404), the host check of the device's merged
// table in tests/host_rs_test.cpp.  Header-only; no device call.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

namespace vcfxh {

// What the reference keeps of a BED text: the distinct names in first-appearance order (of the names
// that keep an interval) as one byte blob plus n_chrom + 1 offsets, per interval its name id, 1-based
// start and end, and the warning text of the rejected lines in line order.
struct RsBed {
    std::string names;
    std::vector<uint64_t> name_off{0};
    std::vector<uint32_t> chrom_id;
    std::vector<int32_t> start1, end;
    std::string warnings;
    uint32_t n_chrom() const { return (uint32_t)(name_off.size() - 1); }

    static bool space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }
    // `stream >> int` at p: white space, one sign, decimal digits up to the first other byte; false
    // without a digit or with a value outside int
    static bool extract_int(const char *&p, const char *e, int &v) {
        while (p < e && space((unsigned char)*p)) p++;
        bool neg = false;
        if (p < e && (*p == '-' || *p == '+')) neg = *p++ == '-';
        const char *d = p;
        int64_t x = 0;
        bool over = false;
        for (; p < e && *p >= '0' && *p <= '9'; p++) {
            if (x > (int64_t)1 << 32) over = true;
            else x = x * 10 + (*p - '0');
        }
        if (p == d) return false;
        if (neg) x = -x;
        if (over || x > INT32_MAX || x < INT32_MIN) return false;
        v = (int)x;
        return true;
    }

    // one line (without its '\n'), number `lineno` from 1
    void line(const char *s, const char *e, uint64_t lineno, std::unordered_map<std::string, uint32_t> &ids) {
        if (s == e || *s == '#') return;
        const char *p = s;
        while (p < e && space((unsigned char)*p)) p++;
        const char *c0 = p;
        while (p < e && !space((unsigned char)*p)) p++;
        const char *c1 = p;
        int a = 0, b = 0;
        if (c0 == c1 || !extract_int(p, e, a) || !extract_int(p, e, b)) {
            warnings += "Warning: skipping invalid bed line " + std::to_string(lineno) + ": ";
            warnings.append(s, (size_t)(e - s));
            warnings += "\n";
            return;
        }
        if (a < 0) a = 0;
        const int64_t st = (int64_t)a + 1;  // 1-based
        if ((int64_t)b < st) return;        // an empty or negative interval: dropped silently
        const std::string name(c0, (size_t)(c1 - c0));
        auto it = ids.find(name);
        if (it == ids.end()) {
            it = ids.emplace(name, n_chrom()).first;
            names += name;
            name_off.push_back(names.size());
        }
        chrom_id.push_back(it->second);
        start1.push_back((int32_t)st);
        end.push_back(b);
    }

    // the whole text: lines end at '\n' only, bytes after the last one are a line
    void parse(const char *p, size_t n) {
        std::unordered_map<std::string, uint32_t> ids;
        uint64_t lineno = 0;
        size_t pos = 0;
        while (pos < n) {
            const char *nl = (const char *)memchr(p + pos, '\n', n - pos);
            const size_t le = nl ? (size_t)(nl - p) : n;
            line(p + pos, p + le, ++lineno, ids);
            pos = le + 1;
        }
    }
};

struct RsRow {
    uint32_t id;
    int32_t start, end;
    bool operator==(const RsRow &o) const { return id == o.id && start == o.start && end == o.end; }
};

// the merged intervals in (name id, start) order: per name sorted by start, joined while
// start <= last end + 1
inline std::vector<RsRow> sort_and_merge(const RsBed &B) {
    std::vector<RsRow> v(B.chrom_id.size());
    for (size_t i = 0; i < v.size(); i++) v[i] = RsRow{B.chrom_id[i], B.start1[i], B.end[i]};
    std::stable_sort(v.begin(), v.end(), [](const RsRow &a, const RsRow &b) { return a.id != b.id ? a.id < b.id : a.start < b.start; });
    std::vector<RsRow> out;
    for (const RsRow &r : v) {
        if (!out.empty() && out.back().id == r.id && (int64_t)r.start <= (int64_t)out.back().end + 1) {
            if (r.end > out.back().end) out.back().end = r.end;
        } else {
            out.push_back(r);
        }
    }
    return out;
}

}  // namespace vcfxh
