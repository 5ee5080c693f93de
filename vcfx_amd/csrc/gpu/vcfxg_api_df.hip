// vcfxg_api_df.hip -- VCFX_diff_tool (the C ABI of include/vcfx_gpu.h)
#include <hipcub/hipcub.hpp>

#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(vcfxg::kDfEmpty == VCFXG_DF_EMPTY && vcfxg::kDfCommon == VCFXG_DF_COMMON && vcfxg::kDfUnique == VCFXG_DF_UNIQUE &&
                  vcfxg::kDfSkipped == VCFXG_DF_SKIPPED && vcfxg::kDfHeader == VCFXG_DF_HEADER &&
                  vcfxg::kDfRepeat == VCFXG_DF_REPEAT && vcfxg::kDfWindow == VCFXG_DF_WINDOW,
              "diff line statuses");

extern "C" {

// The cut line and the key pass over every indexed line, the scans of the data flags and the key
// lengths (the FIRST host synchronisation: the data lines, of file 1 and in all, and the key text's
// bytes size what follows), the key text.  Default mode: hipcub's stable radix sort of (hash, line),
// the run heads and their max scan, the classes, the statuses.  Sorted mode: the ordered check (a
// synchronisation for its flag), then the bounds kernel or the serial walk, launch after launch of
// at most df_walk_steps steps: a step moves a pointer, so ceil(data lines / steps) launches end it,
// with no host read between them.  Then the unique lines' flags and their scan (a synchronisation
// for the counts), their lengths and the scan that places them in the output.
int vcfxg_diff(vcfxg_ctx *c, const vcfxg_df_params *p, vcfxg_summary *out) {
    if (!c || !p || p->hash_bits > 63) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    if (c->data_start != 0 || p->second_start > c->n) return VCFXG_E_ARG;
    DENSE(c);
    const uint64_t L = c->n_lines;
    if (L >= (1ull << 31)) return VCFXG_E_ARG;  // (the scans and the sort count their items in an int)
    HIPCHK(c, hipSetDevice(c->device));
    claim_status(c, StatusOwner::diff);
    c->df_done = {};
    c->df_nu1 = 0;
    c->df_out.n = 0;
    c->df_out.off_host.clear();
    std::memset(c->df_counts, 0, sizeof c->df_counts);
    const int sorted = p->assume_sorted ? 1 : 0, natural = sorted && p->natural ? 1 : 0;
    c->df_counts[6] = sorted ? VCFXG_DF_PATH_BOUNDS : VCFXG_DF_PATH_HASH;
    if (out) std::memset(out, 0, sizeof *out);
    if (!L) {
        mark_done(c, c->df_done);
        return VCFXG_OK;
    }
    int r = status_buffer(c, L, StatusOwner::diff);
    if (!r) r = ensure(c, c->counters, 128);
    if (!r) r = ensure(c, c->df_isdata, 4 * (L + 1));
    if (!r) r = ensure(c, c->df_ord, 8 * (L + 1));
    if (!r) r = ensure(c, c->df_klen, 8 * (L + 1));
    if (!r) r = ensure(c, c->df_koff, 8 * (L + 1));
    if (!r) r = ensure(c, c->df_tabs, 40 * L);
    if (!r) r = ensure(c, c->df_ntok, 4 * L);
    if (!r) r = ensure(c, c->df_posv, 8 * L);
    if (!r) r = ensure(c, c->df_natv, 8 * L);
    if (!r) r = ensure(c, c->df_nsuf, 8 * L);
    if (!r) r = ensure(c, c->df_hash, 8 * L);
    if (!r) r = ensure(c, c->df_queue, 4 * L);
    if (!r) r = ensure(c, c->df_uflag, 4 * (L + 1));
    if (!r) r = ensure(c, c->df_uord, 8 * (L + 1));
    if (!r) r = ensure(c, c->df_state, 16);
    if (!r) r = ensure(c, c->df_sum, 64);
    if (r) return r;
    unsigned long long *counters = P<unsigned long long>(c->counters);
    const DfLines D{P<char>(c->input),      (int64_t)c->data_start,  P<uint64_t>(c->line_end), L,
                    P<uint8_t>(c->status),  P<uint32_t>(c->df_isdata), P<uint32_t>(c->df_ntok),  P<uint64_t>(c->df_tabs),
                    P<uint64_t>(c->df_klen), P<uint64_t>(c->df_nsuf),  P<int64_t>(c->df_posv),   P<int64_t>(c->df_natv)};
    uint64_t *ord = P<uint64_t>(c->df_ord), *koff = P<uint64_t>(c->df_koff);
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 128, c->stream));
    HIPCHK(c, hipMemsetAsync(D.isdata + L, 0, 4, c->stream));
    HIPCHK(c, hipMemsetAsync(D.klen + L, 0, 8, c->stream));
    prof_begin(c, "df_key");
    HIPCHK(c, vcfxg::launch_df_cut(D.line_end, D.data_start, L, p->second_start, counters, c->stream));
    HIPCHK(c, vcfxg::launch_df_key(D, natural, P<uint32_t>(c->df_queue), counters, c->stream));
    prof_end(c, "df_key");
    prof_begin(c, "df_text");
    r = exclusive_scan(c, D.isdata, ord, (size_t)L + 1);
    if (!r) r = exclusive_scan(c, D.klen, koff, (size_t)L + 1);
    if (r) return r;
    static thread_local uint64_t head[4];
    HIPCHK(c, hipMemcpyAsync(&head[0], ord + L, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&head[1], koff + L, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&head[2], counters + 7, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nd = head[0], kbytes = head[1], cut = head[2];
    if (cut > L) return VCFXG_E_HIP;
    HIPCHK(c, hipMemcpyAsync(&head[3], ord + cut, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t n1 = head[3];
    if (nd) {
        // (the gather reads whole aligned 16 B pairs around a key)
        r = ensure(c, c->df_ktext, kbytes + 64);
        if (!r) r = ensure(c, c->df_line, 4 * nd);
        if (r) return r;
        uint32_t *line = P<uint32_t>(c->df_line);
        HIPCHK(c, vcfxg::launch_df_text(D, ord, koff, P<char>(c->df_ktext), P<uint64_t>(c->df_hash), line,
                                        P<uint32_t>(c->df_queue), counters, c->stream));
        prof_end(c, "df_text");
        if (!sorted) {
            prof_begin(c, "df_sort");
            SortScratch &S = c->df_sort;
            r = sort_begin(c, S, nd);
            if (!r) r = ensure(c, c->df_hp, 4 * nd);
            if (!r) r = ensure(c, c->df_head, 4 * nd);
            if (!r) r = ensure(c, c->df_rep, 4 * nd);
            if (!r) r = ensure(c, c->df_first2, 4 * nd);
            if (!r) r = ensure(c, c->df_left, nd);
            if (r) return r;
            uint32_t *hp = P<uint32_t>(c->df_hp), *hd = P<uint32_t>(c->df_head);
            size_t t_scan = 0;
            HIPCHK(c, hipcub::DeviceScan::InclusiveScan(nullptr, t_scan, hp, hd, hipcub::Max(), (int)nd, c->stream));
            r = ensure(c, S.tmp, std::max(S.t_sort, t_scan));
            if (r) return r;
            HIPCHK(c, vcfxg::launch_df_pairs(nd, line, P<uint64_t>(c->df_hash), p->hash_bits, S.ka, S.va, c->stream));
            r = sort_pass(c, S, nd, p->hash_bits ? (int)p->hash_bits : 64);
            if (r) return r;
            prof_end(c, "df_sort");
            prof_begin(c, "df_classes");
            HIPCHK(c, vcfxg::launch_dd_heads(nd, S.ka, hp, c->stream));
            HIPCHK(c, hipcub::DeviceScan::InclusiveScan(S.tmp.p, t_scan, hp, hd, hipcub::Max(), (int)nd, c->stream));
            HIPCHK(c, hipMemsetAsync(c->df_left.p, 0, nd, c->stream));
            HIPCHK(c, vcfxg::launch_df_classes(P<char>(c->df_ktext), koff, D.klen, nd, S.ka, S.va, hd, P<uint32_t>(c->df_rep),
                                               P<uint32_t>(c->df_first2), P<uint8_t>(c->df_left), D.status, counters,
                                               c->stream));
            prof_end(c, "df_classes");
        } else {
            prof_begin(c, "df_ordered");
            HIPCHK(c, vcfxg::launch_df_ordered(D, natural, line, n1, nd, counters, c->stream));
            prof_end(c, "df_ordered");
            static thread_local uint64_t unordered;
            HIPCHK(c, hipMemcpyAsync(&unordered, counters + 8, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (!unordered) {
                prof_begin(c, "df_bounds");
                HIPCHK(c, vcfxg::launch_df_bounds(D, natural, line, n1, nd, c->stream));
                prof_end(c, "df_bounds");
            } else {
                c->df_counts[6] = VCFXG_DF_PATH_WALK;
                uint64_t *state = P<uint64_t>(c->df_state);
                HIPCHK(c, hipMemsetAsync(state, 0, 16, c->stream));
                const uint64_t steps = c->df_walk_steps, launches = std::max<uint64_t>((nd + steps - 1) / steps, 1);
                prof_begin(c, "df_walk");
                for (uint64_t k = 0; k < launches; k++)
                    HIPCHK(c, vcfxg::launch_df_walk(D, natural, line, n1, nd, steps, state, c->stream));
                HIPCHK(c, vcfxg::launch_df_drain(line, n1, nd, state, D.status, c->stream));
                prof_end(c, "df_walk");
            }
        }
    } else {
        prof_end(c, "df_text");
    }
    prof_begin(c, "df_place");
    uint32_t *uflag = P<uint32_t>(c->df_uflag);
    uint64_t *uord = P<uint64_t>(c->df_uord);
    HIPCHK(c, vcfxg::launch_df_flag(L, D.status, uflag, c->stream));
    r = exclusive_scan(c, uflag, uord, (size_t)L + 1);
    if (r) return r;
    HIPCHK(c, vcfxg::launch_df_sum(L, ord, uord, counters, P<uint64_t>(c->df_sum), c->stream));
    static thread_local uint64_t sum[8];
    HIPCHK(c, hipMemcpyAsync(sum, c->df_sum.p, sizeof sum, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nu = sum[0] + sum[1];
    TextOrder &T = c->df_out;
    r = place_begin(c, T, nu);
    if (r) return r;
    HIPCHK(c, vcfxg::launch_df_place(L, uflag, uord, koff, D.klen, P<uint64_t>(T.len), P<uint64_t>(T.src), c->stream));
    r = exclusive_scan(c, P<uint64_t>(T.len), P<uint64_t>(T.off), (size_t)nu + 1);
    if (r) return r;
    prof_end(c, "df_place");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (int i = 0; i < 8; i++)
        if (i != 6) c->df_counts[i] = sum[i];
    c->df_nu1 = sum[0];
    mark_done(c, c->df_done);
    if (out) {
        out->n_lines = L;
        out->rows = nu;
        out->data_lines = nd;
        out->warn_lines = sum[4];
        out->general_records = sum[5];
    }
    return VCFXG_OK;
}

int vcfxg_diff_status(vcfxg_ctx *c, uint64_t first, uint64_t count, uint8_t *status) {
    return c ? fetch_status(c, StatusOwner::diff, c->df_done, first, count, status) : VCFXG_E_ARG;
}

int vcfxg_diff_counts(const vcfxg_ctx *c, uint64_t counts[8]) {
    if (!c || !counts) return VCFXG_E_ARG;
    std::memcpy(counts, c->df_counts, sizeof c->df_counts);
    return VCFXG_OK;
}

// Keys [first_out, first_out + k) of one side's output: as many as fit df_block bytes, one at least,
// gathered into the text from the key text.
int vcfxg_diff_text(vcfxg_ctx *c, int side, uint64_t first_out, uint64_t *taken, uint64_t *bytes) {
    if (!c || (side != 0 && side != 1)) return VCFXG_E_ARG;
    if (taken) *taken = 0;
    if (bytes) *bytes = 0;
    if (!c->indexed || !is_done(c, c->df_done)) return VCFXG_E_STATE;
    const uint64_t lo = side ? c->df_nu1 : 0, hi = side ? c->df_out.n : c->df_nu1;
    if (first_out > hi - lo) return VCFXG_E_ARG;
    return text_block(c, c->df_out, P<char>(c->df_ktext), lo + first_out, hi, c->df_block, "df_gather", taken, bytes);
}

}  // extern "C"
