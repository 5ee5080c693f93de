// vcfxg_api_dd.hip -- VCFX_duplicate_remover (the C ABI of include/vcfx_gpu.h)
#include <hipcub/hipcub.hpp>

#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(vcfxg::kDdEmpty == VCFXG_DD_EMPTY && vcfxg::kDdKept == VCFXG_DD_KEPT && vcfxg::kDdDup == VCFXG_DD_DUP &&
                  vcfxg::kDdShort == VCFXG_DD_SHORT && vcfxg::kDdHeader == VCFXG_DD_HEADER &&
                  vcfxg::kDdWindow == VCFXG_DD_WINDOW,
              "dedup line statuses");

extern "C" {

// The key pass over every indexed line, the data lines' (hash, line) pairs compacted in line
// order (a scan; ONE host synchronisation for their number, which sizes the sort), hipcub's stable
// radix sort, the run heads and their max scan, the verify pass, the status counts (the second
// synchronisation).
int vcfxg_dedup(vcfxg_ctx *c, int mode, const vcfxg_dd_params *p, vcfxg_summary *out) {
    if (!c || !p || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN) || p->hash_bits > 63) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    const uint64_t L = c->n_lines;
    if (L >= (1ull << 31)) return VCFXG_E_ARG;  // (the scans and the sort count their items in an int)
    HIPCHK(c, hipSetDevice(c->device));
    claim_status(c, StatusOwner::dedup);
    c->dd_done = {};
    std::memset(c->dd_counts, 0, sizeof c->dd_counts);
    if (out) std::memset(out, 0, sizeof *out);
    if (!L) {
        mark_done(c, c->dd_done);
        return VCFXG_OK;
    }
    int r = status_buffer(c, L, StatusOwner::dedup);
    if (!r) r = ensure(c, c->counters, 64);
    if (!r) r = ensure(c, c->dd_isdata, 4 * (L + 1));
    if (!r) r = ensure(c, c->dd_ord, 8 * (L + 1));
    if (!r) r = ensure(c, c->dd_tabs, 40 * L);
    if (!r) r = ensure(c, c->dd_pos, 4 * L);
    if (!r) r = ensure(c, c->dd_hash, 8 * L);
    if (!r) r = ensure(c, c->dd_queue, 4 * L);
    if (r) return r;
    const char *buf = P<char>(c->input);
    const int stdin_mode = mode == VCFXG_MODE_STDIN ? 1 : 0;
    const uint64_t *le = P<uint64_t>(c->line_end);
    unsigned long long *counters = P<unsigned long long>(c->counters);
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint32_t>(c->dd_isdata) + L, 0, 4, c->stream));
    prof_begin(c, "dd_key");
    HIPCHK(c, vcfxg::launch_dd_key(buf, (int64_t)c->data_start, (int64_t)c->n, le, L, stdin_mode, P<uint8_t>(c->status),
                                   P<uint32_t>(c->dd_isdata), P<uint64_t>(c->dd_tabs), P<int32_t>(c->dd_pos),
                                   P<uint64_t>(c->dd_hash), P<uint32_t>(c->dd_queue), counters, c->stream));
    prof_end(c, "dd_key");
    prof_begin(c, "dd_sort");
    r = exclusive_scan(c, P<uint32_t>(c->dd_isdata), P<uint64_t>(c->dd_ord), (size_t)L + 1);
    if (r) return r;
    static thread_local uint64_t nd_host;
    HIPCHK(c, hipMemcpyAsync(&nd_host, P<uint64_t>(c->dd_ord) + L, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nd = nd_host;
    if (nd) {
        SortScratch &S = c->dd_sort;
        r = sort_begin(c, S, nd);
        if (!r) r = ensure(c, c->dd_hp, 4 * nd);
        if (!r) r = ensure(c, c->dd_head, 4 * nd);
        if (!r) r = ensure(c, c->dd_left, nd);
        if (r) return r;
        uint32_t *hp = P<uint32_t>(c->dd_hp), *head = P<uint32_t>(c->dd_head);
        size_t t_scan = 0;
        HIPCHK(c, hipcub::DeviceScan::InclusiveScan(nullptr, t_scan, hp, head, hipcub::Max(), (int)nd, c->stream));
        r = ensure(c, S.tmp, std::max(S.t_sort, t_scan));
        if (r) return r;
        HIPCHK(c, vcfxg::launch_dd_gather(L, P<uint32_t>(c->dd_isdata), P<uint64_t>(c->dd_ord), P<uint64_t>(c->dd_hash),
                                          p->hash_bits, S.ka, S.va, c->stream));
        r = sort_pass(c, S, nd, p->hash_bits ? (int)p->hash_bits : 64);
        if (r) return r;
        prof_end(c, "dd_sort");
        prof_begin(c, "dd_verify");
        HIPCHK(c, vcfxg::launch_dd_heads(nd, S.ka, hp, c->stream));
        HIPCHK(c, hipcub::DeviceScan::InclusiveScan(S.tmp.p, t_scan, hp, head, hipcub::Max(), (int)nd, c->stream));
        HIPCHK(c, hipMemsetAsync(c->dd_left.p, 0, nd, c->stream));
        HIPCHK(c, vcfxg::launch_dd_verify(buf, (int64_t)c->data_start, le, stdin_mode, P<uint64_t>(c->dd_tabs),
                                          P<int32_t>(c->dd_pos), nd, S.ka, S.va, head, P<uint8_t>(c->status),
                                          P<uint8_t>(c->dd_left), counters, c->stream));
        prof_end(c, "dd_verify");
    } else {
        prof_end(c, "dd_sort");
    }
    HIPCHK(c, vcfxg::launch_dd_count(L, P<uint8_t>(c->status), counters, c->stream));
    static thread_local uint64_t cnt[8];
    HIPCHK(c, hipMemcpyAsync(cnt, c->counters.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (int i = 0; i < 6; i++) c->dd_counts[i] = cnt[i];
    mark_done(c, c->dd_done);
    if (out) {
        out->n_lines = L;
        out->rows = cnt[VCFXG_DD_KEPT];
        out->data_lines = cnt[VCFXG_DD_KEPT] + cnt[VCFXG_DD_DUP];
        out->warn_lines = cnt[VCFXG_DD_SHORT];
        out->general_records = cnt[5];
    }
    return VCFXG_OK;
}

int vcfxg_dedup_status(vcfxg_ctx *c, uint64_t first, uint64_t count, uint8_t *status) {
    return c ? fetch_status(c, StatusOwner::dedup, c->dd_done, first, count, status) : VCFXG_E_ARG;
}

int vcfxg_dedup_counts(const vcfxg_ctx *c, uint64_t counts[6]) {
    if (!c || !counts) return VCFXG_E_ARG;
    std::memcpy(counts, c->dd_counts, sizeof c->dd_counts);
    return VCFXG_OK;
}

}  // extern "C"
