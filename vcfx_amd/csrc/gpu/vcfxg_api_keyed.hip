// vcfxg_api_keyed.hip -- the host stages the keyed line tools share (VCFX_duplicate_remover,
// VCFX_sorter, VCFX_diff_tool, VCFX_merger; declared in vcfxg_ctx.h): the stable radix sort of
// (key part, line) pairs pass after pass, the placement of the output lines, a block of their text,
// and the fetches of the statuses and the order.
#include <hipcub/hipcub.hpp>

#include "vcfxg_ctx.h"

namespace vcfxg {

int bit_width(uint64_t x) {
    int b = 0;
    while (x) {
        b++;
        x >>= 1;
    }
    return b;
}

int sort_begin(vcfxg_ctx *c, SortScratch &S, uint64_t n) {
    int r = ensure(c, S.k0, 8 * n);
    if (!r) r = ensure(c, S.k1, 8 * n);
    if (!r) r = ensure(c, S.v0, 4 * n);
    if (!r) r = ensure(c, S.v1, 4 * n);
    if (r) return r;
    S.ka = P<uint64_t>(S.k0), S.kb = P<uint64_t>(S.k1);
    S.va = P<uint32_t>(S.v0), S.vb = P<uint32_t>(S.v1);
    S.t_sort = 0;
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(nullptr, S.t_sort, S.ka, S.kb, S.va, S.vb, (int)n, 0, 64, c->stream));
    return ensure(c, S.tmp, S.t_sort);
}

int sort_pass(vcfxg_ctx *c, SortScratch &S, uint64_t n, int end_bit) {
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(S.tmp.p, S.t_sort, S.ka, S.kb, S.va, S.vb, (int)n, 0, end_bit, c->stream));
    std::swap(S.ka, S.kb);
    std::swap(S.va, S.vb);
    return VCFXG_OK;
}

int place_begin(vcfxg_ctx *c, TextOrder &T, uint64_t n) {
    T.n = n;
    T.off_host.clear();
    int r = ensure(c, T.len, 8 * (n + 1));
    if (!r) r = ensure(c, T.off, 8 * (n + 1));
    if (!r) r = ensure(c, T.src, 8 * (n + 1));
    return r;
}

int place_lines(vcfxg_ctx *c, TextOrder &T, const uint64_t *line_end, int64_t data_start, const uint32_t *order, uint64_t n) {
    int r = place_begin(c, T, n);
    if (r) return r;
    HIPCHK(c, launch_line_len(data_start, line_end, n, order, P<uint64_t>(T.len), P<uint64_t>(T.src), c->stream));
    return exclusive_scan(c, P<uint64_t>(T.len), P<uint64_t>(T.off), (size_t)n + 1);
}

int text_block(vcfxg_ctx *c, TextOrder &T, const char *src_text, uint64_t first, uint64_t hi, uint64_t block,
               const char *region, uint64_t *taken, uint64_t *bytes) {
    c->text_bytes = 0;
    if (first == hi) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (T.off_host.size() != T.n + 1) {
        T.off_host.resize(T.n + 1);
        HIPCHK(c, hipMemcpyAsync(T.off_host.data(), T.off.p, 8 * (T.n + 1), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const uint64_t *off = T.off_host.data();
    uint64_t k = (uint64_t)(std::upper_bound(off + first + 1, off + hi + 1, off[first] + block) - (off + first + 1));
    if (!k) k = 1;
    const uint64_t n = off[first + k] - off[first];
    int r = ensure(c, c->text, n + 32);
    if (r) return r;
    prof_begin(c, region);
    HIPCHK(c, launch_text_gather(src_text, P<uint64_t>(T.off), P<uint64_t>(T.src), first, k, n, c->srt_nt, P<char>(c->text),
                                 c->stream));
    prof_end(c, region);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = n;
    if (taken) *taken = k;
    if (bytes) *bytes = n;
    return VCFXG_OK;
}

int fetch_status(vcfxg_ctx *c, StatusOwner owner, const Done &done, uint64_t first, uint64_t count, uint8_t *status) {
    if (!status && count) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, done) || c->status_owner != owner) return VCFXG_E_STATE;
    if (first > c->n_lines || count > c->n_lines - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(status, P<uint8_t>(c->status) + first, count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int fetch_order(vcfxg_ctx *c, const Done &done, const uint32_t *order, uint64_t n, uint64_t first, uint64_t count, uint32_t *lines) {
    if (!lines && count) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, done)) return VCFXG_E_STATE;
    if (first > n || count > n - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(lines, order + first, 4 * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

}  // namespace vcfxg
