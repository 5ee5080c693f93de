// vcfxg_api_mg.hip -- VCFX_merger (the C ABI of include/vcfx_gpu.h)
#include <hipcub/hipcub.hpp>

#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(vcfxg::kMgEmpty == VCFXG_MG_EMPTY && vcfxg::kMgKept == VCFXG_MG_KEPT && vcfxg::kMgBad == VCFXG_MG_BAD &&
                  vcfxg::kMgHeader == VCFXG_MG_HEADER && vcfxg::kMgDropped == VCFXG_MG_DROPPED &&
                  vcfxg::kMgWindow == VCFXG_MG_WINDOW,
              "merger line statuses");

static int mg_bits(uint64_t x) {
    int b = 0;
    while (x) {
        b++;
        x >>= 1;
    }
    return b;
}

extern "C" {

// The files' first lines, the key pass and the class pass over every indexed line, the written
// lines compacted in line order (a scan; ONE host synchronisation for their number, the counts and
// the longest key string, which size the sort).  -s: the ordered check (a synchronisation for its
// flag).  Sort path: hipcub's stable radix sort, least significant part first (POS, the key
// string's length, its words from the last to the first; natural: then num and the prefix), each
// part gathered through the order so far; every bit range starts at 0 (the sorter's finding about
// the library's merge path).  Walk path: launch after launch of at most mg_walk_steps steps: a step
// writes a line, so ceil(kept lines / steps) launches end it, with no host read between them.  Then
// the output lines' lengths and their scan.
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
    c->mg_done = false;
    c->mg_nw = 0;
    c->mg_files = K;
    c->mg_off_host.clear();
    std::memset(c->mg_counts, 0, sizeof c->mg_counts);
    const int sorted = p->assume_sorted ? 1 : 0, natural = p->natural ? 1 : 0;
    c->mg_counts[6] = VCFXG_MG_PATH_SORT;
    c->mg_counts[7] = K;
    if (out) std::memset(out, 0, sizeof *out);
    const uint64_t K1 = (uint64_t)K + 1;
    int r = ensure(c, c->status, L + 1);
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
        c->mg_done = true;
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
        r = ensure(c, c->mg_k0, 8 * nw);
        if (!r) r = ensure(c, c->mg_k1, 8 * nw);
        if (!r) r = ensure(c, c->mg_v0, 4 * nw);
        if (!r) r = ensure(c, c->mg_v1, 4 * nw);
        if (!r) r = ensure(c, c->mg_len, 8 * (nw + 1));
        if (!r) r = ensure(c, c->mg_off, 8 * (nw + 1));
        if (!r) r = ensure(c, c->mg_src, 8 * (nw + 1));
        if (r) return r;
        uint64_t *k0 = P<uint64_t>(c->mg_k0), *k1 = P<uint64_t>(c->mg_k1);
        uint32_t *va = P<uint32_t>(c->mg_v0), *vb = P<uint32_t>(c->mg_v1);
        HIPCHK(c, vcfxg::launch_mg_scatter(L, written, ord, va, c->stream));
        bool walk = false;
        if (sorted) {
            HIPCHK(c, vcfxg::launch_mg_ordered(M, nw, va, counters, c->stream));
            static thread_local uint64_t unordered;
            HIPCHK(c, hipMemcpyAsync(&unordered, counters + 8, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            walk = unordered != 0;
        }
        if (!walk) {
            size_t t_sort = 0;
            HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, k0, k1, va, vb, (int)nw, 0, 64, c->stream));
            r = ensure(c, c->mg_tmp, t_sort);
            if (r) return r;
            auto pass = [&](int part, uint64_t w, uint32_t shift, int end_bit) -> int {
                HIPCHK(c, vcfxg::launch_mg_part(M, nw, part, w, shift, va, k0, c->stream));
                HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(c->mg_tmp.p, t_sort, k0, k1, va, vb, (int)nw, 0, end_bit, c->stream));
                std::swap(va, vb);
                return VCFXG_OK;
            };
            r = pass(kMgPartPos, 0, 0, 64);
            if (!r) r = pass(kMgPartLen, 0, 0, mg_bits(longest + 1));
            const uint64_t W = (longest + 7) / 8;
            for (uint64_t w = W; !r && w-- > 0;) {
                // the last word's low bytes are zero padding in every key string: shifted out
                const uint32_t shift = w == W - 1 && longest % 8 ? (uint32_t)(8 * (8 - longest % 8)) : 0;
                r = pass(kMgPartWord, w, shift, 64 - (int)shift);
            }
            if (natural) {
                if (!r) r = pass(kMgPartNum, 0, 0, 64);
                if (!r) r = pass(kMgPartPrefix, 0, 0, 27);
            }
            if (r) return r;
        } else {
            c->mg_counts[6] = VCFXG_MG_PATH_WALK;
            uint64_t *state = P<uint64_t>(c->mg_state);
            HIPCHK(c, hipMemsetAsync(state, 0, 64, c->stream));
            HIPCHK(c, vcfxg::launch_mg_walk_init(M, ord, va, vb, counters, state, c->stream));
            const uint64_t steps = c->mg_walk_steps, launches = std::max<uint64_t>((kept + steps - 1) / steps, 1);
            for (uint64_t k = 0; k < launches; k++) HIPCHK(c, vcfxg::launch_mg_walk(M, va, vb, steps, state, c->stream));
            std::swap(va, vb);
        }
        c->mg_in_v1 = va == P<uint32_t>(c->mg_v1);
        prof_end(c, "mg_order");
        prof_begin(c, "mg_place");
        HIPCHK(c, vcfxg::launch_srt_len(0, M.line_end, nw, va, P<uint64_t>(c->mg_len), P<uint64_t>(c->mg_src), c->stream));
        r = exclusive_scan(c, P<uint64_t>(c->mg_len), P<uint64_t>(c->mg_off), (size_t)nw + 1);
        if (r) return r;
        prof_end(c, "mg_place");
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        prof_end(c, "mg_order");
    }
    prof_collect(c);
    c->mg_nw = nw;
    c->mg_done = true;
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
    if (!c || (!status && count)) return VCFXG_E_ARG;
    if (!c->indexed || !c->mg_done) return VCFXG_E_STATE;
    if (first > c->n_lines || count > c->n_lines - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(status, P<uint8_t>(c->status) + first, count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_merge_counts(const vcfxg_ctx *c, uint64_t counts[8]) {
    if (!c || !counts) return VCFXG_E_ARG;
    if (!c->indexed || !c->mg_done) return VCFXG_E_STATE;
    std::memcpy(counts, c->mg_counts, sizeof c->mg_counts);
    return VCFXG_OK;
}

int vcfxg_merge_files(vcfxg_ctx *c, uint64_t *first_line, uint64_t *bad) {
    if (!c || !first_line || !bad) return VCFXG_E_ARG;
    if (!c->indexed || !c->mg_done) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t K1 = (uint64_t)c->mg_files + 1;
    const uint64_t *fm = P<uint64_t>(c->mg_fmeta);
    HIPCHK(c, hipMemcpyAsync(first_line, fm + K1, 8 * K1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(bad, fm + 4 * K1, 8 * (K1 - 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_merge_order(vcfxg_ctx *c, uint64_t first, uint64_t count, uint32_t *lines) {
    if (!c || (!lines && count)) return VCFXG_E_ARG;
    if (!c->indexed || !c->mg_done) return VCFXG_E_STATE;
    if (first > c->mg_nw || count > c->mg_nw - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t *order = P<uint32_t>(c->mg_in_v1 ? c->mg_v1 : c->mg_v0);
    HIPCHK(c, hipMemcpyAsync(lines, order + first, 4 * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

// Output lines [first, first + k): as many as fit srt_block bytes, one at least (the offsets are
// read back once per merge; the cut is a search in them), gathered into the text by the sorter's
// gather.
int vcfxg_merge_text(vcfxg_ctx *c, uint64_t first, uint64_t *lines_taken, uint64_t *bytes) {
    if (!c) return VCFXG_E_ARG;
    if (lines_taken) *lines_taken = 0;
    if (bytes) *bytes = 0;
    if (!c->indexed || !c->mg_done) return VCFXG_E_STATE;
    const uint64_t nw = c->mg_nw;
    if (first > nw) return VCFXG_E_ARG;
    c->text_bytes = 0;
    if (first == nw) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->mg_off_host.size() != nw + 1) {
        c->mg_off_host.resize(nw + 1);
        HIPCHK(c, hipMemcpyAsync(c->mg_off_host.data(), c->mg_off.p, 8 * (nw + 1), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const uint64_t *off = c->mg_off_host.data();
    uint64_t k = (uint64_t)(std::upper_bound(off + first + 1, off + nw + 1, off[first] + c->srt_block) - (off + first + 1));
    if (!k) k = 1;
    const uint64_t n = off[first + k] - off[first];
    int r = ensure(c, c->text, n + 32);
    if (r) return r;
    prof_begin(c, "mg_gather");
    HIPCHK(c, vcfxg::launch_srt_gather(P<char>(c->input), P<uint64_t>(c->mg_off), P<uint64_t>(c->mg_src), first, k, n,
                                       c->srt_nt, P<char>(c->text), c->stream));
    prof_end(c, "mg_gather");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = n;
    if (lines_taken) *lines_taken = k;
    if (bytes) *bytes = n;
    return VCFXG_OK;
}

}  // extern "C"
