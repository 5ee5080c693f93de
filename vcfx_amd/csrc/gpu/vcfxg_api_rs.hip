// vcfxg_api_rs.hip -- VCFX_region_subsampler (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(vcfxg::kRsEmpty == VCFXG_RS_EMPTY && vcfxg::kRsHeader == VCFXG_RS_HEADER && vcfxg::kRsIn == VCFXG_RS_IN &&
                  vcfxg::kRsOut == VCFXG_RS_OUT && vcfxg::kRsEarly == VCFXG_RS_EARLY && vcfxg::kRsShort == VCFXG_RS_SHORT &&
                  vcfxg::kRsBadPos == VCFXG_RS_BADPOS && vcfxg::kRsWindow == VCFXG_RS_WINDOW,
              "region line statuses");

extern "C" {

// The names and the intervals uploaded, the dictionary filled, the intervals sorted by (name id,
// start), the reach scanned along them, the names' ranges and the merged rows placed; ONE host
// synchronisation at the end, for the number of merged rows.
int vcfxg_regions_load(vcfxg_ctx *c, const char *names, const uint64_t *name_off, uint32_t n_chrom, const uint32_t *chrom_id,
                       const int32_t *start1, const int32_t *end, uint64_t n, const vcfxg_rs_params *p) {
    if (!c || !p || p->hash_bits > 63 || n >= (1ull << 31) || n_chrom >= (1u << 31)) return VCFXG_E_ARG;
    if ((n_chrom && (!names || !name_off)) || (n && (!chrom_id || !start1 || !end || !n_chrom))) return VCFXG_E_ARG;
    for (uint32_t i = 0; i < n_chrom; i++)
        if (name_off[i + 1] < name_off[i]) return VCFXG_E_ARG;
    for (uint64_t j = 0; j < n; j++)
        if (chrom_id[j] >= n_chrom || start1[j] < 1 || end[j] < start1[j]) return VCFXG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    c->rs_loaded = false;
    c->rs_done = {};  // (statuses of an earlier filter belong to the table they were made with)
    const uint64_t name_bytes = n_chrom ? name_off[n_chrom] : 0;
    uint32_t slots = 4;
    while (slots < 2u * n_chrom) slots <<= 1;
    int r = ensure(c, c->rs_names, name_bytes + 16);
    if (!r) r = ensure(c, c->rs_noff, 8 * ((size_t)n_chrom + 1));
    if (!r) r = ensure(c, c->rs_dict, 4 * (size_t)slots);
    if (!r) r = ensure(c, c->rs_first, 4 * ((size_t)n_chrom + 1));
    if (!r) r = ensure(c, c->rs_last, 4 * ((size_t)n_chrom + 1));
    if (!r) r = ensure(c, c->rs_tab, sizeof(RsTableArgs));
    if (!r) r = ensure(c, c->rs_in, 12 * (n + 1));
    if (!r) r = ensure(c, c->rs_sid, 4 * (n + 1));
    if (!r) r = ensure(c, c->rs_start, 4 * (n + 1));
    if (!r) r = ensure(c, c->rs_reach, 4 * (n + 1));
    if (!r) r = ensure(c, c->rs_key, 8 * (n + 1));
    if (!r) r = ensure(c, c->rs_tile, 8 * (rs_scan_tiles(n) + 1));
    if (!r) r = ensure(c, c->rs_open, 4 * (n + 1));
    if (!r) r = ensure(c, c->rs_ord, 8 * (n + 1));
    if (!r) r = ensure(c, c->rs_mid, 4 * (n + 1));
    if (!r) r = ensure(c, c->rs_mstart, 4 * (n + 1));
    if (!r) r = ensure(c, c->rs_mend, 4 * (n + 1));
    if (r) return r;
    // (the copies are synchronous with respect to the caller's pageable memory once the call returns:
    // it ends in a stream synchronisation)
    static const uint64_t zero_off = 0;
    HIPCHK(c, hipMemcpyAsync(c->rs_noff.p, n_chrom ? name_off : &zero_off, 8 * ((size_t)n_chrom + 1), hipMemcpyHostToDevice,
                             c->stream));
    if (name_bytes) HIPCHK(c, hipMemcpyAsync(c->rs_names.p, names, name_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->rs_dict.p, 0, 4 * (size_t)slots, c->stream));
    HIPCHK(c, hipMemsetAsync(c->rs_first.p, 0, 4 * ((size_t)n_chrom + 1), c->stream));
    HIPCHK(c, hipMemsetAsync(c->rs_last.p, 0, 4 * ((size_t)n_chrom + 1), c->stream));
    uint32_t *in_id = P<uint32_t>(c->rs_in);
    int32_t *in_start = P<int32_t>(c->rs_in) + n, *in_end = P<int32_t>(c->rs_in) + 2 * n;
    if (n) {
        HIPCHK(c, hipMemcpyAsync(in_id, chrom_id, 4 * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(in_start, start1, 4 * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(in_end, end, 4 * n, hipMemcpyHostToDevice, c->stream));
    }
    static thread_local RsTableArgs tab;
    tab = RsTableArgs{P<char>(c->rs_names),    P<uint64_t>(c->rs_noff), P<uint32_t>(c->rs_dict),
                      P<uint32_t>(c->rs_first), P<uint32_t>(c->rs_last), P<int32_t>(c->rs_start),
                      P<int32_t>(c->rs_reach),  slots - 1u,              rs_hash_mask(p->hash_bits)};
    HIPCHK(c, hipMemcpyAsync(c->rs_tab.p, &tab, sizeof tab, hipMemcpyHostToDevice, c->stream));
    prof_begin(c, "rs_build");
    HIPCHK(c, vcfxg::launch_rs_dict(n_chrom, P<char>(c->rs_names), P<uint64_t>(c->rs_noff), p->hash_bits, slots - 1u,
                                    P<uint32_t>(c->rs_dict), c->stream));
    uint64_t nm = 0;
    if (n) {
        SortScratch &S = c->rs_sort;
        r = sort_begin(c, S, n);
        if (r) return r;
        HIPCHK(c, vcfxg::launch_rs_keys(n, in_id, in_start, S.ka, S.va, c->stream));
        r = sort_pass(c, S, n, 32 + std::max(1, bit_width(n_chrom - 1u)));
        if (r) return r;
        uint32_t *open = P<uint32_t>(c->rs_open);
        HIPCHK(c, hipMemsetAsync(open + n, 0, 4, c->stream));
        HIPCHK(c, vcfxg::launch_rs_table(n, S.ka, S.va, in_end, P<uint32_t>(c->rs_sid), P<int32_t>(c->rs_start),
                                         P<uint64_t>(c->rs_key), P<uint64_t>(c->rs_tile), P<int32_t>(c->rs_reach),
                                         P<uint32_t>(c->rs_first), P<uint32_t>(c->rs_last), open, c->stream));
        r = exclusive_scan(c, open, P<uint64_t>(c->rs_ord), (size_t)n + 1);
        if (r) return r;
        HIPCHK(c, vcfxg::launch_rs_rows(n, P<uint32_t>(c->rs_sid), P<int32_t>(c->rs_start), P<int32_t>(c->rs_reach), open,
                                        P<uint64_t>(c->rs_ord), P<uint32_t>(c->rs_mid), P<int32_t>(c->rs_mstart),
                                        P<int32_t>(c->rs_mend), c->stream));
        prof_end(c, "rs_build");
        static thread_local uint64_t nm_host;
        HIPCHK(c, hipMemcpyAsync(&nm_host, P<uint64_t>(c->rs_ord) + n, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        nm = nm_host;
    } else {
        prof_end(c, "rs_build");
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    prof_collect(c);
    c->rs_n = n;
    c->rs_nm = nm;
    c->rs_nchrom = n_chrom;
    c->rs_loaded = true;
    return VCFXG_OK;
}

int vcfxg_regions_merged(vcfxg_ctx *c, uint32_t *chrom_id, int32_t *start1, int32_t *end, uint64_t cap, uint64_t *n) {
    if (!c || !n) return VCFXG_E_ARG;
    if (!c->rs_loaded) return VCFXG_E_STATE;
    *n = c->rs_nm;
    if (c->rs_nm > cap) return VCFXG_OK;  // (the caller repeats the call with room for all)
    if (!c->rs_nm) return VCFXG_OK;
    if (!chrom_id || !start1 || !end) return VCFXG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(chrom_id, c->rs_mid.p, 4 * c->rs_nm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(start1, c->rs_mstart.p, 4 * c->rs_nm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(end, c->rs_mend.p, 4 * c->rs_nm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

// The class pass over every indexed line and the status counts: ONE host synchronisation.
int vcfxg_region_filter(vcfxg_ctx *c, int mode, vcfxg_summary *out) {
    if (!c || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (!c->indexed || !c->rs_loaded) return VCFXG_E_STATE;
    DENSE(c);
    const uint64_t L = c->n_lines;
    if (L >= (1ull << 31)) return VCFXG_E_ARG;  // (the wave list holds line numbers in 32 bits)
    HIPCHK(c, hipSetDevice(c->device));
    claim_status(c, StatusOwner::region);
    c->rs_done = {};
    std::memset(c->rs_counts, 0, sizeof c->rs_counts);
    if (out) std::memset(out, 0, sizeof *out);
    if (!L) {
        mark_done(c, c->rs_done);
        return VCFXG_OK;
    }
    int r = status_buffer(c, L, StatusOwner::region);
    if (!r) r = ensure(c, c->counters, 128);
    if (!r) r = ensure(c, c->rs_queue, 4 * L);
    if (r) return r;
    unsigned long long *counters = P<unsigned long long>(c->counters);
    static thread_local uint64_t init[9];
    std::memset(init, 0, sizeof init);
    init[8] = L;
    HIPCHK(c, hipMemcpyAsync(counters, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    prof_begin(c, "rs_class");
    HIPCHK(c, vcfxg::launch_rs_class(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end), L,
                                     mode == VCFXG_MODE_STDIN ? 1 : 0, P<RsTableArgs>(c->rs_tab), P<uint8_t>(c->status), P<uint32_t>(c->rs_queue),
                                     counters, c->stream));
    prof_end(c, "rs_class");
    static thread_local uint64_t cnt[8];
    HIPCHK(c, hipMemcpyAsync(cnt, counters, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (int i = 0; i < 8; i++) c->rs_counts[i] = cnt[i];
    mark_done(c, c->rs_done);
    if (out) {
        out->n_lines = L;
        out->rows = cnt[VCFXG_RS_IN];
        out->data_lines = cnt[VCFXG_RS_IN] + cnt[VCFXG_RS_OUT] + cnt[VCFXG_RS_EARLY] + cnt[VCFXG_RS_SHORT] + cnt[VCFXG_RS_BADPOS];
        out->warn_lines = cnt[VCFXG_RS_EARLY] + cnt[VCFXG_RS_SHORT] + cnt[VCFXG_RS_BADPOS];
        out->general_records = cnt[7];
    }
    return VCFXG_OK;
}

int vcfxg_region_status(vcfxg_ctx *c, uint64_t first, uint64_t count, uint8_t *status) {
    return c ? fetch_status(c, StatusOwner::region, c->rs_done, first, count, status) : VCFXG_E_ARG;
}

int vcfxg_region_counts(const vcfxg_ctx *c, uint64_t counts[8]) {
    if (!c || !counts) return VCFXG_E_ARG;
    std::memcpy(counts, c->rs_counts, sizeof c->rs_counts);
    return VCFXG_OK;
}

}  // extern "C"
