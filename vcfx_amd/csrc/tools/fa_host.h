// fa_host.h -- the host side of VCFX_fasta_converter that needs no device: the sample names of a
// "#CHROM" line (VCFX_fasta_converter.cpp:314-324, :448-455), the layout of the text the device
// writes (each sample's row of sequence lines, 60 bases a line), and the runs of lines that are
// parsed against one set of names.  Plain C++ over include/vcfx_gpu.h's constants: tests/
// host_fa_test.cpp builds it under ASan + UBSan without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "vcfx_gpu.h"

namespace vcfxh {

// fields 10 onward of the line [s, s + n) appended to names: every tab ends a field, and a line
// that ends in a tab has no empty field after it (the loops stop at the line's end); a '\r' before
// the '\n' belongs to the last name
inline void fa_names(const char *s, size_t n, std::vector<std::string> &names) {
    size_t p = 0, col = 0;
    while (p < n) {
        size_t e = p;
        while (e < n && s[e] != '\t') e++;
        if (col >= 9) names.emplace_back(s + p, e - p);
        p = e + 1;
        col++;
    }
}

// lines [l0, l1) of the index are parsed against the first n_samples names
struct FaRun {
    uint64_t l0, l1;
    uint32_t n_samples;
};

// The text: sample s holds columns [skip[s], total) -- skip[s] = the columns before the "#CHROM"
// line that named it (missing entries: 0) -- as lines of VCFXG_FA_LINE bases, each with its '\n'.
// row_off[s] = the row's first byte, row_off[samples] = the text's size.
struct FaLayout {
    std::vector<uint64_t> row_off, skip;
    bool any_skip = false;
    static uint64_t row_bytes(uint64_t cols) { return cols + (cols + VCFXG_FA_LINE - 1) / VCFXG_FA_LINE; }
    void make(size_t samples, uint64_t total, const std::vector<uint64_t> &skipped) {
        skip.assign(samples, 0);
        row_off.assign(samples + 1, 0);
        any_skip = false;
        for (size_t s = 0; s < samples; s++) {
            if (s < skipped.size()) skip[s] = skipped[s] < total ? skipped[s] : total;
            any_skip = any_skip || skip[s] != 0;
            row_off[s + 1] = row_off[s] + row_bytes(total - skip[s]);
        }
    }
    uint64_t bytes() const { return row_off.empty() ? 0 : row_off.back(); }
    // skip for a run of n samples: null when none of them skips a column (the aligned tiles)
    const uint64_t *skip_of(uint32_t n) const {
        for (uint32_t s = 0; s < n && s < skip.size(); s++)
            if (skip[s]) return skip.data();
        return nullptr;
    }
};

}  // namespace vcfxh
