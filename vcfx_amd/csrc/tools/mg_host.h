// mg_host.h -- the host side of VCFX_merger that needs no device: how the opened files become the
// one text the device indexes (every file in list order, each followed by one '\n' when it is not
// empty and lacks a final one), where each file begins in it, and the split of a -m value.  Plain
// C++: tests/host_mg_test.cpp builds it under ASan + UBSan without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace vcfxh {

// a piece of the joined text, in order (vcfxg_ingest's arguments)
struct MgChunk {
    const char *p;
    size_t n;
    int final_chunk;
};

struct MgJoin {
    std::vector<MgChunk> chunk;
    std::vector<uint64_t> start;  // after finish(): files + 1 offsets, the last one `total`
    uint64_t total = 0;
    size_t files() const { return start.empty() ? 0 : start.size() - 1; }
    // the next file = [p, p + n) (n = 0: p is not read)
    void add(const char *p, size_t n) {
        static const char nl = '\n';
        start.push_back(total);
        if (!n) return;
        chunk.push_back({p, n, 0});
        total += n;
        if (p[n - 1] != '\n') {
            chunk.push_back({&nl, 1, 0});
            total += 1;
        }
    }
    // the last chunk is marked final (an empty join is one empty final chunk)
    void finish() {
        start.push_back(total);
        if (chunk.empty()) chunk.push_back({nullptr, 0, 1});
        chunk.back().final_chunk = 1;
    }
};

// a -m value split at every comma, every piece appended, empty ones too (run :109-118)
inline void mg_split(const std::string &value, std::vector<std::string> &names) {
    size_t a = 0;
    for (;;) {
        const size_t b = value.find(',', a);
        if (b == std::string::npos) break;
        names.emplace_back(value, a, b - a);
        a = b + 1;
    }
    names.emplace_back(value, a);
}

}  // namespace vcfxh
