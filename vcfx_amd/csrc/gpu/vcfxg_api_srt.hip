// vcfxg_api_srt.hip -- VCFX_sorter (the C ABI of include/vcfx_gpu.h)
#include <hipcub/hipcub.hpp>

#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(vcfxg::kSrtEmpty == VCFXG_SRT_EMPTY && vcfxg::kSrtKept == VCFXG_SRT_KEPT && vcfxg::kSrtPre == VCFXG_SRT_PRE &&
                  vcfxg::kSrtBad == VCFXG_SRT_BAD && vcfxg::kSrtHeader == VCFXG_SRT_HEADER &&
                  vcfxg::kSrtWindow == VCFXG_SRT_WINDOW,
              "sorter line statuses");

static int srt_bits(uint64_t x) {
    int b = 0;
    while (x) {
        b++;
        x >>= 1;
    }
    return b;
}

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
    c->srt_done = false;
    c->srt_nw = 0;
    c->srt_off_host.clear();
    std::memset(c->srt_counts, 0, sizeof c->srt_counts);
    if (out) std::memset(out, 0, sizeof *out);
    if (!L) {
        c->srt_done = true;
        return VCFXG_OK;
    }
    int r = ensure(c, c->status, L + 1);
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
        r = ensure(c, c->srt_k0, 8 * nw);
        if (!r) r = ensure(c, c->srt_k1, 8 * nw);
        if (!r) r = ensure(c, c->srt_v0, 4 * nw);
        if (!r) r = ensure(c, c->srt_v1, 4 * nw);
        if (!r) r = ensure(c, c->srt_len, 8 * (nw + 1));
        if (!r) r = ensure(c, c->srt_off, 8 * (nw + 1));
        if (!r) r = ensure(c, c->srt_src, 8 * (nw + 1));
        if (r) return r;
        uint64_t *k0 = P<uint64_t>(c->srt_k0), *k1 = P<uint64_t>(c->srt_k1);
        uint32_t *va = P<uint32_t>(c->srt_v0), *vb = P<uint32_t>(c->srt_v1);
        size_t t_sort = 0;
        HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, k0, k1, va, vb, (int)nw, 0, 64, c->stream));
        r = ensure(c, c->srt_tmp, t_sort);
        if (r) return r;
        HIPCHK(c, vcfxg::launch_srt_scatter(L, stdin_mode, natural, status, P<uint32_t>(c->srt_written),
                                            P<uint64_t>(c->srt_ord), P<int32_t>(c->srt_pos), P<uint32_t>(c->srt_aux), k0, va,
                                            c->stream));
        // the bits of the first pass that vary: all of (id, POS); POS and as much of the length word
        // as the longest CHROM fills (stdin mode's empty CHROM sets them all)
        const int end0 = natural || stdin_mode ? 64 : 32 + srt_bits(longest + 1);
        HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(c->srt_tmp.p, t_sort, k0, k1, va, vb, (int)nw, 0, end0, c->stream));
        std::swap(va, vb);
        if (!natural) {
            const uint64_t W = (longest + 7) / 8;
            for (uint64_t w = W; w-- > 0;) {
                // the last word's low bytes are zero padding in every CHROM (all ones only in stdin
                // mode's empty CHROM, which the length word has already put last): shifted out, so
                // the sort's bit range starts at 0 (the library's merge path, which takes 1 K to 1 M
                // items, builds its mask with a shift by begin + bits, undefined when that is 64)
                const int shift = w == W - 1 && longest % 8 ? (int)(8 * (8 - longest % 8)) : 0;
                HIPCHK(c, vcfxg::launch_srt_word(buf, (int64_t)c->data_start, le, nw, stdin_mode, (uint32_t)w, (uint32_t)shift,
                                                 va, status, P<uint32_t>(c->srt_aux), P<uint64_t>(c->srt_w0), k0, c->stream));
                HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(c->srt_tmp.p, t_sort, k0, k1, va, vb, (int)nw, 0, 64 - shift,
                                                             c->stream));
                std::swap(va, vb);
            }
        }
        c->srt_in_v1 = va == P<uint32_t>(c->srt_v1);
        prof_end(c, "srt_sort");
        prof_begin(c, "srt_place");
        HIPCHK(c, vcfxg::launch_srt_len((int64_t)c->data_start, le, nw, va, P<uint64_t>(c->srt_len), P<uint64_t>(c->srt_src),
                                        c->stream));
        r = exclusive_scan(c, P<uint64_t>(c->srt_len), P<uint64_t>(c->srt_off), (size_t)nw + 1);
        if (r) return r;
        prof_end(c, "srt_place");
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        prof_end(c, "srt_sort");
    }
    prof_collect(c);
    c->srt_nw = nw;
    c->srt_done = true;
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
    if (!c || (!status && count)) return VCFXG_E_ARG;
    if (!c->indexed || !c->srt_done) return VCFXG_E_STATE;
    if (first > c->n_lines || count > c->n_lines - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(status, P<uint8_t>(c->status) + first, count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_sort_counts(const vcfxg_ctx *c, uint64_t counts[6]) {
    if (!c || !counts) return VCFXG_E_ARG;
    std::memcpy(counts, c->srt_counts, sizeof c->srt_counts);
    return VCFXG_OK;
}

int vcfxg_sort_order(vcfxg_ctx *c, uint64_t first, uint64_t count, uint32_t *lines) {
    if (!c || (!lines && count)) return VCFXG_E_ARG;
    if (!c->indexed || !c->srt_done) return VCFXG_E_STATE;
    if (first > c->srt_nw || count > c->srt_nw - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t *order = P<uint32_t>(c->srt_in_v1 ? c->srt_v1 : c->srt_v0);
    HIPCHK(c, hipMemcpyAsync(lines, order + first, 4 * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

// Output lines [first, first + k): as many as fit srt_block bytes, one at least (the offsets are
// read back once per sort; the cut is a search in them), gathered into the text.
int vcfxg_sort_text(vcfxg_ctx *c, uint64_t first, uint64_t *lines_taken, uint64_t *bytes) {
    if (!c) return VCFXG_E_ARG;
    if (lines_taken) *lines_taken = 0;
    if (bytes) *bytes = 0;
    if (!c->indexed || !c->srt_done) return VCFXG_E_STATE;
    const uint64_t nw = c->srt_nw;
    if (first > nw) return VCFXG_E_ARG;
    c->text_bytes = 0;
    if (first == nw) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->srt_off_host.size() != nw + 1) {
        c->srt_off_host.resize(nw + 1);
        HIPCHK(c, hipMemcpyAsync(c->srt_off_host.data(), c->srt_off.p, 8 * (nw + 1), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const uint64_t *off = c->srt_off_host.data();
    uint64_t k = (uint64_t)(std::upper_bound(off + first + 1, off + nw + 1, off[first] + c->srt_block) - (off + first + 1));
    if (!k) k = 1;
    const uint64_t n = off[first + k] - off[first];
    int r = ensure(c, c->text, n + 32);
    if (r) return r;
    prof_begin(c, "srt_gather");
    HIPCHK(c, vcfxg::launch_srt_gather(P<char>(c->input), P<uint64_t>(c->srt_off), P<uint64_t>(c->srt_src), first, k, n,
                                       c->srt_nt, P<char>(c->text), c->stream));
    prof_end(c, "srt_gather");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = n;
    if (lines_taken) *lines_taken = k;
    if (bytes) *bytes = n;
    return VCFXG_OK;
}

}  // extern "C"
