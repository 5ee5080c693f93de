// df_host.h -- the host side of VCFX_diff_tool that needs no device: how the two files become the
// one text the device indexes (file 1, one '\n' when file 1 is not empty and lacks a final one, file
// 2).  Plain C++: tests/host_df_test.cpp builds it under
// ASan + UBSan without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vcfxh {

// a piece of the joined text, in order (vcfxg_ingest's arguments)
struct DfChunk {
    const char *p;
    size_t n;
    int final_chunk;
};

struct DfJoin {
    DfChunk chunk[3];
    int chunks = 0;
    uint64_t second_start = 0, total = 0;  // where file 2 begins; all bytes
    // file 1 = [p1, p1 + n1), file 2 = [p2, p2 + n2); the last chunk is marked final (an empty
    // join is one empty final chunk)
    void make(const char *p1, size_t n1, const char *p2, size_t n2) {
        static const char nl = '\n';
        chunks = 0;
        if (n1) chunk[chunks++] = {p1, n1, 0};
        if (n1 && p1[n1 - 1] != '\n') chunk[chunks++] = {&nl, 1, 0};
        second_start = 0;
        for (int i = 0; i < chunks; i++) second_start += chunk[i].n;
        chunk[chunks++] = {n2 ? p2 : nullptr, n2, 1};
        total = second_start + n2;
    }
};

}  // namespace vcfxh
