// vcfxg_api_srt.hip -- VCFX_sorter (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(vcfxg::kSrtEmpty == VCFXG_SRT_EMPTY && vcfxg::kSrtKept == VCFXG_SRT_KEPT && vcfxg::kSrtPre == VCFXG_SRT_PRE &&
                  vcfxg::kSrtBad == VCFXG_SRT_BAD && vcfxg::kSrtHeader == VCFXG_SRT_HEADER &&
                  vcfxg::kSrtWindow == VCFXG_SRT_WINDOW,
              "sorter line statuses");

extern "C" {

// The key pass and the class pass over every indexed line, the written lines' (key, line) pairs
// compacted in line order (a scan; ONE host synchronisation for their number, the status counts
// and the longest CHROM, which size the sort), hipcub's stable radix sort (natural: one pass over
// (id, POS); lexicographic: (length, POS), then CHROM's words from the last to the first, each
// gathered through the order so far), the output lines' lengths and their scan.
int vcfxg_sort(vcfxg_ctx *c, int mode, const vcfxg_srt_params *p, vcfxg_summary *out) {
    if (!c || !p || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    const uint64_t L = c->n_lines;
    if (L >= (1ull << 31)) return VCFXG_E_ARG;  // (the scans and the sort count their items in an int)
    HIPCHK(c, hipSetDevice(c->device));
    claim_status(c, StatusOwner::sort);
    c->srt_done = {};
    c->srt_out.n = 0;
    c->srt_out.off_host.clear();
    std::memset(c->srt_counts, 0, sizeof c->srt_counts);
    if (out) std::memset(out, 0, sizeof *out);
    if (!L) {
        mark_done(c, c->srt_done);
        return VCFXG_OK;
    }
    int r = status_buffer(c, L, StatusOwner::sort);
    if (!r) r = ensure(c, c->counters, 64);
    if (!r) r = ensure(c, c->srt_pos, 4 * L);
    if (!r) r = ensure(c, c->srt_aux, 4 * L);
    if (!r) r = ensure(c, c->srt_w0, 8 * L);
    if (!r) r = ensure(c, c->srt_queue, 4 * L);
    if (!r) r = ensure(c, c->srt_written, 4 * (L + 1));
    if (!r) r = ensure(c, c->srt_ord, 8 * (L + 1));
    if (r) return r;
    const char *buf = P<char>(c->input);
    const int stdin_mode = mode == VCFXG_MODE_STDIN ? 1 : 0, natural = p->natural ? 1 : 0;
    const uint64_t *le = P<uint64_t>(c->line_end);
    unsigned long long *counters = P<unsigned long long>(c->counters);
    uint8_t *status = P<uint8_t>(c->status);
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint32_t>(c->srt_written) + L, 0, 4, c->stream));
    prof_begin(c, "srt_key");
    HIPCHK(c, vcfxg::launch_srt_key(buf, (int64_t)c->data_start, le, L, stdin_mode, natural, status, P<int32_t>(c->srt_pos),
                                    P<uint32_t>(c->srt_aux), P<uint64_t>(c->srt_w0), P<uint32_t>(c->srt_queue), counters,
                                    c->stream));
    HIPCHK(c, vcfxg::launch_srt_class(L, stdin_mode, natural, status, P<uint32_t>(c->srt_aux), P<uint32_t>(c->srt_written),
                                      counters, c->stream));
    prof_end(c, "srt_key");
    prof_begin(c, "srt_sort");
    r = exclusive_scan(c, P<uint32_t>(c->srt_written), P<uint64_t>(c->srt_ord), (size_t)L + 1);
    if (r) return r;
    static thread_local uint64_t head[9];
    HIPCHK(c, hipMemcpyAsync(&head[0], P<uint64_t>(c->srt_ord) + L, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&head[1], c->counters.p, 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nw = head[0], longest = head[8];
    for (int i = 0; i < 6; i++) c->srt_counts[i] = head[1 + i];
    if (nw) {
        SortScratch &S = c->srt_sort;
        r = sort_begin(c, S, nw);
        if (r) return r;
        HIPCHK(c, vcfxg::launch_srt_scatter(L, stdin_mode, natural, status, P<uint32_t>(c->srt_written),
                                            P<uint64_t>(c->srt_ord), P<int32_t>(c->srt_pos), P<uint32_t>(c->srt_aux), S.ka,
                                            S.va, c->stream));
        // the bits of the first pass that vary: all of (id, POS); POS and as much of the length word
        // as the longest CHROM fills (stdin mode's empty CHROM sets them all)
        r = sort_pass(c, S, nw, natural || stdin_mode ? 64 : 32 + bit_width(longest + 1));
        // (the last word's low bytes are all ones only in stdin mode's empty CHROM, which the length
        // word has already put last)
        if (!r && !natural)
            r = sort_string_words(c, S, nw, longest, [&](uint64_t w, uint32_t shift) -> int {
                HIPCHK(c, vcfxg::launch_srt_word(buf, (int64_t)c->data_start, le, nw, stdin_mode, (uint32_t)w, shift, S.va,
                                                 status, P<uint32_t>(c->srt_aux), P<uint64_t>(c->srt_w0), S.ka, c->stream));
                return VCFXG_OK;
            });
        if (r) return r;
        prof_end(c, "srt_sort");
        prof_begin(c, "srt_place");
        r = place_lines(c, c->srt_out, le, (int64_t)c->data_start, S.va, nw);
        if (r) return r;
        prof_end(c, "srt_place");
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        prof_end(c, "srt_sort");
    }
    prof_collect(c);
    mark_done(c, c->srt_done);
    if (out) {
        out->n_lines = L;
        out->rows = nw;
        out->data_lines = head[1 + VCFXG_SRT_KEPT];
        out->warn_lines = head[1 + VCFXG_SRT_PRE] + head[1 + VCFXG_SRT_BAD];
        out->general_records = head[1 + 5];
    }
    return VCFXG_OK;
}

int vcfxg_sort_status(vcfxg_ctx *c, uint64_t first, uint64_t count, uint8_t *status) {
    return c ? fetch_status(c, StatusOwner::sort, c->srt_done, first, count, status) : VCFXG_E_ARG;
}

int vcfxg_sort_counts(const vcfxg_ctx *c, uint64_t counts[6]) {
    if (!c || !counts) return VCFXG_E_ARG;
    std::memcpy(counts, c->srt_counts, sizeof c->srt_counts);
    return VCFXG_OK;
}

int vcfxg_sort_order(vcfxg_ctx *c, uint64_t first, uint64_t count, uint32_t *lines) {
    return c ? fetch_order(c, c->srt_done, c->srt_sort.va, c->srt_out.n, first, count, lines) : VCFXG_E_ARG;
}

// Output lines [first, first + k): as many as fit srt_block bytes, one at least, gathered into the text.
int vcfxg_sort_text(vcfxg_ctx *c, uint64_t first, uint64_t *lines_taken, uint64_t *bytes) {
    if (!c) return VCFXG_E_ARG;
    if (lines_taken) *lines_taken = 0;
    if (bytes) *bytes = 0;
    if (!c->indexed || !is_done(c, c->srt_done)) return VCFXG_E_STATE;
    if (first > c->srt_out.n) return VCFXG_E_ARG;
    return text_block(c, c->srt_out, P<char>(c->input), first, c->srt_out.n, c->srt_block, "srt_gather", lines_taken, bytes);
}

}  // extern "C"
