// vcfxg_api_fa.hip -- VCFX_fasta_converter over a block of indexed lines (the C ABI of
// include/vcfx_gpu.h): scan, column numbering, the bases of the block's columns, their transpose
// into the text (one host synchronisation for the block's column count)
#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(kFaEmpty == VCFXG_FA_EMPTY && kFaColumn == VCFXG_FA_COLUMN && kFaSkipped == VCFXG_FA_SKIPPED &&
                  kFaHeader == VCFXG_FA_HEADER && kFaChrom == VCFXG_FA_CHROM && kFaLine == VCFXG_FA_LINE &&
                  kFaTileSamples == VCFXG_FA_TILE_SAMPLES && kFaTileCols == VCFXG_FA_TILE_COLUMNS &&
                  kFaTable == VCFXG_FA_TABLE,
              "fasta_converter constants");

// The block [l0, l0 + n): statuses, flags, FaMeta, column numbers; tail[0] = its columns,
// tail[1] = its "#CHROM" lines (after a synchronisation).
static int fa_scan_block(vcfxg_ctx *c, uint64_t l0, uint64_t n, int mode, uint32_t n_samples, uint64_t tail[2]) {
    int r = af_buffers(c, c->n_lines, StatusOwner::fasta);
    if (!r) r = ensure(c, c->fa_flag, 4 * (n + 1));
    if (!r) r = ensure(c, c->fa_col, 8 * (n + 1));
    if (!r) r = ensure(c, c->fa_meta, sizeof(FaMeta) * n);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint32_t>(c->fa_flag) + n, 0, 4, c->stream));
    prof_begin(c, "fa_scan");
    HIPCHK(c, launch_fa_scan(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end), l0, n,
                             mode == VCFXG_MODE_STDIN, n_samples, P<uint8_t>(c->status), P<uint32_t>(c->fa_flag),
                             P<FaMeta>(c->fa_meta), P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "fa_scan");
    prof_begin(c, "fa_number");
    r = exclusive_scan(c, P<uint32_t>(c->fa_flag), P<uint64_t>(c->fa_col), (size_t)n + 1);
    prof_end(c, "fa_number");
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(&tail[0], P<uint64_t>(c->fa_col) + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&tail[1], P<unsigned long long>(c->counters) + 1, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fa_l0 = l0;
    c->fa_n = n;
    c->fa_cols = tail[0];
    mark_done(c, c->fa_scanned);
    return VCFXG_OK;
}

static bool fa_args(vcfxg_ctx *c, uint64_t l0, uint64_t l1, int mode) {
    return c && (mode == VCFXG_MODE_FILE || mode == VCFXG_MODE_STDIN) && l0 <= l1;
}

extern "C" {

int vcfxg_fasta_scan(vcfxg_ctx *c, uint64_t l0, uint64_t l1, int mode, uint32_t n_samples, vcfxg_summary *out) {
    if (!fa_args(c, l0, l1, mode)) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    if (l1 > c->n_lines) return VCFXG_E_ARG;
    l1 = std::min(l1, l0 + c->fa_block);
    HIPCHK(c, hipSetDevice(c->device));
    c->fa_scanned = {};
    if (out) std::memset(out, 0, sizeof *out);
    if (l1 == l0) return VCFXG_OK;
    static thread_local uint64_t tail[2];
    const int r = fa_scan_block(c, l0, l1 - l0, mode, n_samples, tail);
    if (r) return r;
    prof_collect(c);
    if (out) {
        out->n_lines = l1 - l0;
        out->rows = tail[0];
        out->warn_lines = tail[1];
    }
    return VCFXG_OK;
}

int vcfxg_fasta_status(vcfxg_ctx *c, uint64_t first, uint64_t count, uint8_t *status, uint64_t *col) {
    if (!c || (!status && !col && count)) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->fa_scanned) || (status && c->status_owner != StatusOwner::fasta)) return VCFXG_E_STATE;
    if (first < c->fa_l0 || first + count > c->fa_l0 + c->fa_n) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    if (status)
        HIPCHK(c, hipMemcpyAsync(status, P<uint8_t>(c->status) + first, count, hipMemcpyDeviceToHost, c->stream));
    if (col)
        HIPCHK(c, hipMemcpyAsync(col, P<uint64_t>(c->fa_col) + (first - c->fa_l0), 8 * count, hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_fasta_begin(vcfxg_ctx *c, uint64_t text_bytes) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    const int r = ensure(c, c->text, text_bytes + 16);
    if (r) return r;
    c->text_bytes = text_bytes;
    c->fa_text = text_bytes;
    mark_done(c, c->fa_begun);
    return VCFXG_OK;
}

int vcfxg_fasta(vcfxg_ctx *c, uint64_t l0, uint64_t l1, const vcfxg_fa_params *p, vcfxg_summary *out) {
    if (!p || !fa_args(c, l0, l1, p->mode) || (p->n_samples && !p->row_off)) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->fa_begun) || c->text_bytes != c->fa_text) return VCFXG_E_STATE;
    DENSE(c);
    if (l1 > c->n_lines) return VCFXG_E_ARG;
    l1 = std::min(l1, l0 + c->fa_block);
    HIPCHK(c, hipSetDevice(c->device));
    c->fa_scanned = {};
    if (out) std::memset(out, 0, sizeof *out);
    if (l1 == l0) return VCFXG_OK;
    const uint64_t n = l1 - l0, ns = p->n_samples;
    // every byte the transpose writes lies inside the text: a row's last byte is the '\n' after
    // column total_cols - 1
    for (uint64_t s = 0; s < ns; s++) {
        const uint64_t sk = p->skip ? p->skip[s] : 0;
        if (sk > p->total_cols) return VCFXG_E_ARG;
        const uint64_t v = p->total_cols - sk, len = v + (v + kFaLine - 1) / kFaLine;
        if (p->row_off[s] > c->fa_text || len > c->fa_text - p->row_off[s]) return VCFXG_E_ARG;
    }
    static thread_local uint64_t tail[3];
    int r = fa_scan_block(c, l0, n, p->mode, p->n_samples, tail);
    if (r) return r;
    const uint64_t cols = tail[0];
    if (p->first_col > p->total_cols || cols > p->total_cols - p->first_col) return VCFXG_E_ARG;
    tail[2] = 0;
    if (cols && ns) {
        const uint64_t pitch = (ns + 15) & ~15ull;
        r = ensure(c, c->fa_M, cols * pitch);
        if (!r) r = ensure(c, c->fa_rowoff, 8 * ns);
        if (!r && p->skip) r = ensure(c, c->fa_skip, 8 * ns);
        if (r) return r;
        HIPCHK(c, hipMemcpyAsync(c->fa_rowoff.p, p->row_off, 8 * ns, hipMemcpyHostToDevice, c->stream));
        if (p->skip) HIPCHK(c, hipMemcpyAsync(c->fa_skip.p, p->skip, 8 * ns, hipMemcpyHostToDevice, c->stream));
        prof_begin(c, "fa_bases");
        HIPCHK(c, launch_fa_bases(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end), l0, n,
                                  P<uint8_t>(c->status), P<uint64_t>(c->fa_col), P<FaMeta>(c->fa_meta), p->n_samples, pitch,
                                  P<uint8_t>(c->fa_M), P<unsigned long long>(c->counters), c->stream));
        prof_end(c, "fa_bases");
        prof_begin(c, "fa_transpose");
        HIPCHK(c, launch_fa_transpose(P<uint8_t>(c->fa_M), pitch, cols, p->n_samples, p->first_col, p->total_cols,
                                      P<uint64_t>(c->fa_rowoff), p->skip ? P<uint64_t>(c->fa_skip) : nullptr,
                                      P<char>(c->text), c->stream));
        prof_end(c, "fa_transpose");
        HIPCHK(c, hipMemcpyAsync(&tail[2], c->counters.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (row_off / skip are the caller's again)
    }
    prof_collect(c);
    if (out) {
        out->n_lines = n;
        out->rows = cols;
        out->warn_lines = tail[1];
        out->general_records = tail[2];
        out->text_bytes = c->fa_text;
    }
    return VCFXG_OK;
}

}  // extern "C"
