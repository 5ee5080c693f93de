// vcfxg_api_mg.hip -- VCFX_merger (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(vcfxg::kMgEmpty == VCFXG_MG_EMPTY && vcfxg::kMgKept == VCFXG_MG_KEPT && vcfxg::kMgBad == VCFXG_MG_BAD &&
                  vcfxg::kMgHeader == VCFXG_MG_HEADER && vcfxg::kMgDropped == VCFXG_MG_DROPPED &&
                  vcfxg::kMgWindow == VCFXG_MG_WINDOW,
              "merger line statuses");

extern "C" {

// The files' first lines, the key pass and the class pass over every indexed line, the written
// lines compacted in line order (a scan; ONE host synchronisation for their number, the counts and
// the longest key string, which size the sort).  -s: the ordered check (a synchronisation for its
// flag).  Sort path: hipcub's stable radix sort, least significant part first (POS, the key
// string's length, its words from the last to the first; natural: then num and the prefix), each
// part gathered through the order so far; every bit range starts at 0 (sort_string_words).  Walk
// path: launch after launch of at most mg_walk_steps steps: a step writes a line, so ceil(kept
// lines / steps) launches end it, with no host read between them.  Then the output lines' lengths
// and their scan.
int vcfxg_merge(vcfxg_ctx *c, const vcfxg_mg_params *p, vcfxg_summary *out) {
    if (!c || !p || !p->file_start || !p->n_files) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    const uint32_t K = p->n_files;
    if (c->data_start != 0 || p->file_start[0] != 0 || p->file_start[K] != c->n) return VCFXG_E_ARG;
    for (uint32_t f = 0; f < K; f++)
        if (p->file_start[f] > p->file_start[f + 1]) return VCFXG_E_ARG;
    DENSE(c);
    const uint64_t L = c->n_lines;
    if (L >= (1ull << 31)) return VCFXG_E_ARG;  // (the scans and the sort count their items in an int)
    HIPCHK(c, hipSetDevice(c->device));
    claim_status(c, StatusOwner::merge);
    c->mg_done = {};
    c->mg_out.n = 0;
    c->mg_out.off_host.clear();
    c->mg_files = K;
    std::memset(c->mg_counts, 0, sizeof c->mg_counts);
    const int sorted = p->assume_sorted ? 1 : 0, natural = p->natural ? 1 : 0;
    c->mg_counts[6] = VCFXG_MG_PATH_SORT;
    c->mg_counts[7] = K;
    if (out) std::memset(out, 0, sizeof *out);
    const uint64_t K1 = (uint64_t)K + 1;
    int r = status_buffer(c, L, StatusOwner::merge);
    if (!r) r = ensure(c, c->counters, 128);
    if (!r) r = ensure(c, c->mg_fmeta, 8 * 7 * K1);
    if (!r) r = ensure(c, c->mg_file, 4 * (L + 1));
    if (!r) r = ensure(c, c->mg_pn, 4 * (L + 1));
    if (!r) r = ensure(c, c->mg_pos, 8 * (L + 1));
    if (!r) r = ensure(c, c->mg_w0, 8 * (L + 1));
    if (!r) r = ensure(c, c->mg_ks, 8 * (L + 1));
    if (!r) r = ensure(c, c->mg_kl, 8 * (L + 1));
    if (!r) r = ensure(c, c->mg_num, 8 * (L + 1));
    if (!r) r = ensure(c, c->mg_queue, 4 * (L + 1));
    if (!r) r = ensure(c, c->mg_written, 4 * (L + 1));
    if (!r) r = ensure(c, c->mg_ord, 8 * (L + 1));
    if (!r) r = ensure(c, c->mg_state, 64);
    if (r) return r;
    uint64_t *fm = P<uint64_t>(c->mg_fmeta);
    unsigned long long *counters = P<unsigned long long>(c->counters);
    const MgLines M{P<char>(c->input),    P<uint64_t>(c->line_end), L,
                    K,                    sorted,                   natural,
                    P<uint8_t>(c->status), P<uint32_t>(c->mg_file),  P<uint32_t>(c->mg_pn),
                    P<uint64_t>(c->mg_w0), P<uint64_t>(c->mg_ks),    P<uint64_t>(c->mg_kl),
                    P<uint64_t>(c->mg_num), P<int64_t>(c->mg_pos),   fm,
                    fm + K1,              fm + 2 * K1,              fm + 3 * K1,
                    fm + 4 * K1,          fm + 5 * K1,              fm + 6 * K1};
    uint32_t *written = P<uint32_t>(c->mg_written);
    uint64_t *ord = P<uint64_t>(c->mg_ord);
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 128, c->stream));
    HIPCHK(c, hipMemcpyAsync(fm, p->file_start, 8 * K1, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's array is read by now)
    prof_begin(c, "mg_key");
    HIPCHK(c, vcfxg::launch_mg_cut(M, c->stream));
    if (!L) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        prof_end(c, "mg_key");
        prof_collect(c);
        mark_done(c, c->mg_done);
        return VCFXG_OK;
    }
    HIPCHK(c, hipMemsetAsync(written + L, 0, 4, c->stream));
    HIPCHK(c, vcfxg::launch_mg_key(M, P<uint32_t>(c->mg_queue), counters, c->stream));
    HIPCHK(c, vcfxg::launch_mg_class(M, written, counters, c->stream));
    prof_end(c, "mg_key");
    prof_begin(c, "mg_order");
    r = exclusive_scan(c, written, ord, (size_t)L + 1);
    if (r) return r;
    static thread_local uint64_t head[10];
    HIPCHK(c, hipMemcpyAsync(&head[0], ord + L, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&head[1], c->counters.p, 72, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nw = head[0], kept = head[1 + VCFXG_MG_KEPT], longest = head[1 + 6];
    for (int i = 0; i < 6; i++) c->mg_counts[i] = head[1 + i];
    c->mg_counts[7] = head[1 + 7];
    if (nw) {
        SortScratch &S = c->mg_sort;
        r = sort_begin(c, S, nw);
        if (r) return r;
        HIPCHK(c, vcfxg::launch_mg_scatter(L, written, ord, S.va, c->stream));
        bool walk = false;
        if (sorted) {
            HIPCHK(c, vcfxg::launch_mg_ordered(M, nw, S.va, counters, c->stream));
            static thread_local uint64_t unordered;
            HIPCHK(c, hipMemcpyAsync(&unordered, counters + 8, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            walk = unordered != 0;
        }
        if (!walk) {
            auto fill = [&](int part, uint64_t w, uint32_t shift) -> int {
                HIPCHK(c, vcfxg::launch_mg_part(M, nw, part, w, shift, S.va, S.ka, c->stream));
                return VCFXG_OK;
            };
            auto pass = [&](int part, int end_bit) -> int {
                const int rf = fill(part, 0, 0);
                return rf ? rf : sort_pass(c, S, nw, end_bit);
            };
            r = pass(kMgPartPos, 64);
            if (!r) r = pass(kMgPartLen, bit_width(longest + 1));
            if (!r) r = sort_string_words(c, S, nw, longest, [&](uint64_t w, uint32_t shift) { return fill(kMgPartWord, w, shift); });
            if (natural) {
                if (!r) r = pass(kMgPartNum, 64);
                if (!r) r = pass(kMgPartPrefix, 27);
            }
            if (r) return r;
        } else {
            c->mg_counts[6] = VCFXG_MG_PATH_WALK;
            uint64_t *state = P<uint64_t>(c->mg_state);
            HIPCHK(c, hipMemsetAsync(state, 0, 64, c->stream));
            HIPCHK(c, vcfxg::launch_mg_walk_init(M, ord, S.va, S.vb, counters, state, c->stream));
            const uint64_t steps = c->mg_walk_steps, launches = std::max<uint64_t>((kept + steps - 1) / steps, 1);
            for (uint64_t k = 0; k < launches; k++) HIPCHK(c, vcfxg::launch_mg_walk(M, S.va, S.vb, steps, state, c->stream));
            std::swap(S.va, S.vb);
        }
        prof_end(c, "mg_order");
        prof_begin(c, "mg_place");
        r = place_lines(c, c->mg_out, M.line_end, 0, S.va, nw);
        if (r) return r;
        prof_end(c, "mg_place");
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        prof_end(c, "mg_order");
    }
    prof_collect(c);
    mark_done(c, c->mg_done);
    if (out) {
        out->n_lines = L;
        out->rows = nw;
        out->data_lines = kept;
        out->warn_lines = head[1 + VCFXG_MG_BAD];
        out->general_records = head[1 + 5];
    }
    return VCFXG_OK;
}

int vcfxg_merge_status(vcfxg_ctx *c, uint64_t first, uint64_t count, uint8_t *status) {
    return c ? fetch_status(c, StatusOwner::merge, c->mg_done, first, count, status) : VCFXG_E_ARG;
}

int vcfxg_merge_counts(const vcfxg_ctx *c, uint64_t counts[8]) {
    if (!c || !counts) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->mg_done)) return VCFXG_E_STATE;
    std::memcpy(counts, c->mg_counts, sizeof c->mg_counts);
    return VCFXG_OK;
}

int vcfxg_merge_files(vcfxg_ctx *c, uint64_t *first_line, uint64_t *bad) {
    if (!c || !first_line || !bad) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->mg_done)) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t K1 = (uint64_t)c->mg_files + 1;
    const uint64_t *fm = P<uint64_t>(c->mg_fmeta);
    HIPCHK(c, hipMemcpyAsync(first_line, fm + K1, 8 * K1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(bad, fm + 4 * K1, 8 * (K1 - 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_merge_order(vcfxg_ctx *c, uint64_t first, uint64_t count, uint32_t *lines) {
    return c ? fetch_order(c, c->mg_done, c->mg_sort.va, c->mg_out.n, first, count, lines) : VCFXG_E_ARG;
}

// Output lines [first, first + k): as many as fit srt_block bytes, one at least, gathered into the text.
int vcfxg_merge_text(vcfxg_ctx *c, uint64_t first, uint64_t *lines_taken, uint64_t *bytes) {
    if (!c) return VCFXG_E_ARG;
    if (lines_taken) *lines_taken = 0;
    if (bytes) *bytes = 0;
    if (!c->indexed || !is_done(c, c->mg_done)) return VCFXG_E_STATE;
    if (first > c->mg_out.n) return VCFXG_E_ARG;
    return text_block(c, c->mg_out, P<char>(c->input), first, c->mg_out.n, c->srt_block, "mg_gather", lines_taken, bytes);
}

}  // extern "C"
