// fx_host.h -- the host side of VCFX_field_extractor that needs no device: the --fields list
// (main, VCFX_field_extractor.cpp:733-742), what each field is in each mode (parseFieldSpec :282-314
// for a file, parseLineExtract :582-647 for stdin), the check of the S<n> fields that std::stoi would
// reject, the names of the first "#CHROM" line (:366-385, :674-680) and the table the device reads
// (vcfxg_fx_col, include/vcfx_gpu.h).  Plain C++: tests/host_fx_test.cpp builds it under ASan + UBSan
// without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "vcfx_gpu.h"

namespace vcfxh {

// one -f value appended to the list: split at commas, the empty items kept ("" is one empty field)
inline void fx_split_fields(const char *arg, std::vector<std::string> &fields) {
    const char *p = arg;
    for (;;) {
        const char *e = strchr(p, ',');
        if (!e) break;
        fields.emplace_back(p, (size_t)(e - p));
        p = e + 1;
    }
    fields.emplace_back(p);
}

// the header row: the field strings joined by tabs
inline std::string fx_header_row(const std::vector<std::string> &fields) {
    std::string r;
    for (size_t i = 0; i < fields.size(); i++) {
        if (i) r += '\t';
        r += fields[i];
    }
    r += '\n';
    return r;
}

inline int fx_standard(const std::string &f) {
    static const char *const kStd[8] = {"CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"};
    for (int i = 0; i < 8; i++)
        if (f == kStd[i]) return i;
    return -1;
}

// the sample part of "sample:subfield": 0 = a name, 1 = 'S' and digits with idx = std::stoi of them,
// -1 = 'S' and digits that std::stoi rejects ('S' alone, a value outside int)
inline int fx_sample_index(const std::string &part, int64_t &idx) {
    if (part.empty() || part[0] != 'S') return 0;
    for (size_t i = 1; i < part.size(); i++)
        if (part[i] < '0' || part[i] > '9') return 0;
    if (part.size() == 1) return -1;
    int64_t v = 0;
    for (size_t i = 1; i < part.size(); i++) {
        v = v * 10 + (part[i] - '0');
        if (v > 2147483647ll) return -1;
    }
    idx = v;
    return 1;
}

// the first field the reference would abort on, or -1 (checked before any input is read)
inline int fx_first_bad_field(const std::vector<std::string> &fields) {
    for (size_t i = 0; i < fields.size(); i++) {
        const std::string &f = fields[i];
        const size_t colon = f.find(':');
        int64_t idx;
        if (fx_standard(f) < 0 && colon != std::string::npos && fx_sample_index(f.substr(0, colon), idx) < 0) return (int)i;
    }
    return -1;
}

// is the (stripped) line the "#CHROM" line
inline bool fx_is_chrom(const char *s, size_t n) { return n >= 6 && !memcmp(s, "#CHROM", 6); }

// name -> column of the "#CHROM" line's fields 10 onward: of two equal names the later column wins; a
// line that ends in a tab has an empty last name.  The caller strips the '\r' in file mode only.
inline void fx_names(const char *s, size_t n, std::unordered_map<std::string, uint32_t> &names) {
    names.clear();
    size_t p = 0;
    uint32_t col = 0;
    for (;;) {
        size_t e = p;
        while (e < n && s[e] != '\t') e++;
        if (col >= 9) names[std::string(s + p, e - p)] = col;
        col++;
        if (e >= n) break;
        p = e + 1;
    }
}

inline bool fx_needs_names(const std::vector<std::string> &fields, bool stdin_mode) {
    for (const std::string &f : fields) {
        const size_t colon = f.find(':');
        if (fx_standard(f) >= 0 || colon == std::string::npos) continue;
        int64_t idx = 0;
        const int form = fx_sample_index(f.substr(0, colon), idx);
        if (form == 0 || (form == 1 && idx == 0 && !stdin_mode)) return true;  // (file mode: S0 is the name "")
    }
    return false;
}

// The table: one vcfxg_fx_col per field, keys and sub-fields in the pool.  names: the "#CHROM" line's
// (empty without one: every name is unresolved).  Fields that fx_first_bad_field rejects must not come
// here.
inline void fx_build(const std::vector<std::string> &fields, const std::unordered_map<std::string, uint32_t> &names,
                     bool stdin_mode, std::vector<vcfxg_fx_col> &cols, std::string &pool) {
    cols.clear();
    pool.clear();
    cols.reserve(fields.size());
    auto add = [&](const std::string &s) {
        const uint32_t o = (uint32_t)pool.size();
        pool += s;
        return o;
    };
    for (const std::string &f : fields) {
        vcfxg_fx_col c;
        memset(&c, 0, sizeof c);
        c.key_len = VCFXG_FX_NOKEY;
        const int std_col = fx_standard(f);
        const size_t colon = f.find(':');
        if (std_col >= 0) {
            c.kind = VCFXG_FX_STD;
            c.col = (uint32_t)std_col;
        } else if (colon == std::string::npos) {
            c.kind = VCFXG_FX_INFO;
            c.key_off = add(f);
            c.key_len = (uint32_t)f.size();
        } else {
            c.kind = VCFXG_FX_SAMPLE;
            const std::string part = f.substr(0, colon), sub = f.substr(colon + 1);
            int64_t idx = 0;
            const int form = fx_sample_index(part, idx);
            bool by_name = form == 0;
            std::string name = part;
            if (form == 1) {
                if (idx > 2147483638ll) c.col = 0;  // (outside the domain: the reference's int sum overflows)
                else if (idx > 0) c.col = (uint32_t)(9 + (idx - 1));
                else if (!stdin_mode) by_name = true, name.clear();  // (file mode: index 0 falls to the name "")
                // (stdin mode: index 0 is column 8, below the samples: nothing)
            }
            if (by_name) {
                const auto it = names.find(name);
                c.named = 1;
                if (it != names.end()) c.col = it->second;
            }
            c.sub_off = add(sub);
            c.sub_len = (uint32_t)sub.size();
            if (stdin_mode) {  // (the map of INFO is asked for the whole field first)
                c.key_off = add(f);
                c.key_len = (uint32_t)f.size();
            }
        }
        cols.push_back(c);
    }
}

}  // namespace vcfxh
