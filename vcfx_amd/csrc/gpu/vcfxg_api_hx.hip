// vcfxg_api_hx.hip -- VCFX_haplotype_extractor over the indexed lines (the C ABI of include/vcfx_gpu.h):
// the scan and the segmentation (two host synchronisations: the member count sizes the member arrays,
// the block count the block arrays), the block table and the rows' layout (one: the text's size), the
// rows' text (none before the caller fetches it)
#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(kHxEmpty == VCFXG_HX_EMPTY && kHxHeader == VCFXG_HX_HEADER && kHxShort == VCFXG_HX_SHORT &&
                  kHxBadPos == VCFXG_HX_BADPOS && kHxNoGt == VCFXG_HX_NOGT && kHxUnphased == VCFXG_HX_UNPHASED &&
                  kHxMember == VCFXG_HX_MEMBER && kHxTileMembers == VCFXG_HX_TILE_MEMBERS &&
                  kHxTileSamples == VCFXG_HX_TILE_SAMPLES && kHxCellBytes == VCFXG_HX_CELL_BYTES,
              "haplotype_extractor constants");

template <typename T>
static int hx_fetch(vcfxg_ctx *c, DevBuf &b, uint64_t first, uint64_t count, T *host) {
    if (host && count)
        HIPCHK(c, hipMemcpyAsync(host, P<T>(b) + first, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream));
    return VCFXG_OK;
}

extern "C" {

int vcfxg_haplotype_scan(vcfxg_ctx *c, const vcfxg_hx_params *p, vcfxg_summary *out) {
    if (!c || !p || (p->mode != VCFXG_MODE_FILE && p->mode != VCFXG_MODE_STDIN) || !p->n_samples) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    HIPCHK(c, hipSetDevice(c->device));
    claim_status(c, StatusOwner::haplotype);
    c->hx_scanned = c->hx_laid = {};
    if (out) std::memset(out, 0, sizeof *out);
    const uint64_t n = c->n_lines, ns = p->n_samples;
    c->hx_ns = p->n_samples;
    c->hx_nm = c->hx_nb = 0;
    if (!n) {
        mark_done(c, c->hx_scanned);
        return VCFXG_OK;
    }
    if (n > (~0ull / kHxCellBytes) / ns) return VCFXG_E_NOMEM;
    int r = af_buffers(c, n, StatusOwner::haplotype);
    if (!r) r = ensure(c, c->hx_pos, 8 * n);
    if (!r) r = ensure(c, c->hx_flag, 4 * (n + 1));
    if (!r) r = ensure(c, c->hx_mnum, 8 * (n + 1));
    if (!r) r = ensure(c, c->hx_clen, 4 * n);
    if (!r) r = ensure(c, c->hx_fixed, 4 * n);
    if (!r) r = ensure(c, c->hx_general, 4 * (n + 1));
    if (!r) r = ensure(c, c->hx_gnum, 8 * (n + 1));
    if (!r) r = ensure(c, c->hx_lmember, 8 * n);
    if (!r) r = ensure(c, c->hx_lblock, 8 * n);
    if (!r) r = ensure(c, c->hx_lflip, 4 * n);
    if (!r) r = ensure(c, c->hx_cells, kHxCellBytes * n * ns);
    if (r) return r;
    const char *buf = P<char>(c->input);
    const uint64_t *le = P<uint64_t>(c->line_end);
    HIPCHK(c, hipMemsetAsync(P<uint32_t>(c->hx_flag) + n, 0, 4, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint32_t>(c->hx_general) + n, 0, 4, c->stream));
    prof_begin(c, "hx_scan");
    HIPCHK(c, launch_hx_scan(buf, (int64_t)c->data_start, le, n, p->mode == VCFXG_MODE_STDIN, p->n_samples,
                             P<uint8_t>(c->status), P<int64_t>(c->hx_pos), P<uint32_t>(c->hx_flag), P<uint32_t>(c->hx_clen),
                             P<uint32_t>(c->hx_fixed), P<uint32_t>(c->hx_general), P<uint64_t>(c->hx_cells), c->stream));
    prof_end(c, "hx_scan");
    prof_begin(c, "hx_number");
    r = exclusive_scan(c, P<uint32_t>(c->hx_flag), P<uint64_t>(c->hx_mnum), (size_t)n + 1);
    if (!r) r = exclusive_scan(c, P<uint32_t>(c->hx_general), P<uint64_t>(c->hx_gnum), (size_t)n + 1);
    prof_end(c, "hx_number");
    if (r) return r;
    static thread_local uint64_t tail[3];
    HIPCHK(c, hipMemcpyAsync(&tail[0], P<uint64_t>(c->hx_mnum) + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&tail[2], P<uint64_t>(c->hx_gnum) + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nm = tail[0];
    r = ensure(c, c->hx_mline, 8 * (nm + 1));
    if (!r) r = ensure(c, c->hx_start, 4 * (nm + 1));
    if (!r) r = ensure(c, c->hx_bnum, 8 * (nm + 1));
    if (!r) r = ensure(c, c->hx_flip, 4 * (nm + 1));
    if (r) return r;
    prof_begin(c, "hx_segment");
    HIPCHK(c, launch_hx_members(n, P<uint32_t>(c->hx_flag), P<uint64_t>(c->hx_mnum), P<uint64_t>(c->hx_mline),
                                P<uint64_t>(c->hx_lmember), P<uint64_t>(c->hx_lblock), P<uint32_t>(c->hx_lflip), c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint32_t>(c->hx_start) + nm, 0, 4, c->stream));
    HIPCHK(c, launch_hx_break(buf, (int64_t)c->data_start, le, nm, P<uint64_t>(c->hx_mline), P<int64_t>(c->hx_pos),
                              P<uint32_t>(c->hx_clen), P<uint32_t>(c->hx_fixed), P<uint64_t>(c->hx_cells), p->n_samples,
                              p->block_size, p->check != 0,
                              P<uint32_t>(c->hx_start), P<uint32_t>(c->hx_flip), c->stream));
    r = exclusive_scan(c, P<uint32_t>(c->hx_start), P<uint64_t>(c->hx_bnum), (size_t)nm + 1);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(&tail[1], P<uint64_t>(c->hx_bnum) + nm, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nb = tail[1];
    r = ensure(c, c->hx_first, 8 * (nb + 1));
    if (!r) r = ensure(c, c->hx_last, 8 * (nb + 1));
    if (r) return r;
    HIPCHK(c, launch_hx_blocks(nm, P<uint64_t>(c->hx_mline), P<uint32_t>(c->hx_start), P<uint64_t>(c->hx_bnum),
                               P<uint32_t>(c->hx_flip), P<uint64_t>(c->hx_first), P<uint64_t>(c->hx_last),
                               P<uint64_t>(c->hx_lblock), P<uint32_t>(c->hx_lflip), c->stream));
    prof_end(c, "hx_segment");
    prof_collect(c);
    c->hx_nm = nm;
    c->hx_nb = nb;
    mark_done(c, c->hx_scanned);
    if (out) {
        out->n_lines = n;
        out->rows = nm;
        out->data_lines = nb;
        out->general_records = tail[2];
    }
    return VCFXG_OK;
}

int vcfxg_haplotype_lines(vcfxg_ctx *c, uint64_t first, uint64_t count, uint8_t *status, int64_t *pos, uint64_t *member,
                          uint64_t *block, uint32_t *flip) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->hx_scanned) || (status && c->status_owner != StatusOwner::haplotype)) return VCFXG_E_STATE;
    if (first > c->n_lines || count > c->n_lines - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    int r = hx_fetch(c, c->status, first, count, status);
    if (!r) r = hx_fetch(c, c->hx_pos, first, count, pos);
    if (!r) r = hx_fetch(c, c->hx_lmember, first, count, member);
    if (!r) r = hx_fetch(c, c->hx_lblock, first, count, block);
    if (!r) r = hx_fetch(c, c->hx_lflip, first, count, flip);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_haplotype_blocks(vcfxg_ctx *c, vcfxg_summary *out) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->hx_scanned)) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    c->hx_laid = {};
    if (out) std::memset(out, 0, sizeof *out);
    const uint64_t nm = c->hx_nm, nb = c->hx_nb, ns = c->hx_ns, nt = hx_tiles(nm);
    c->hx_text = 0;
    if (nm) {
        if (nt > (~0ull / 8) / ns || nb > (~0ull / 8) / ns) return VCFXG_E_NOMEM;
        int r = ensure(c, c->hx_agg, 8 * nt * ns);
        if (!r) r = ensure(c, c->hx_carry, 8 * nt * ns);
        if (!r) r = ensure(c, c->hx_tstart, 4 * nt);
        if (!r) r = ensure(c, c->hx_base, 8 * nb * ns);
        if (!r) r = ensure(c, c->hx_head, 4 * nb);
        if (!r) r = ensure(c, c->hx_rowlen, 8 * (nb + 1));
        if (!r) r = ensure(c, c->hx_rowoff, 8 * (nb + 1));
        if (!r) r = ensure(c, c->hx_bstart, 8 * nb);
        if (!r) r = ensure(c, c->hx_bend, 8 * nb);
        if (r) return r;
        HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->hx_rowlen) + nb, 0, 8, c->stream));
        prof_begin(c, "hx_layout");
        HIPCHK(c, launch_hx_layout(nm, nb, c->hx_ns, P<uint64_t>(c->hx_mline), P<uint32_t>(c->hx_start),
                                   P<uint64_t>(c->hx_bnum), P<uint32_t>(c->hx_fixed), P<uint64_t>(c->hx_cells),
                                   P<uint64_t>(c->hx_first),
                                   P<uint64_t>(c->hx_last), P<int64_t>(c->hx_pos), P<uint32_t>(c->hx_clen),
                                   P<uint64_t>(c->hx_agg), P<uint32_t>(c->hx_tstart), P<uint64_t>(c->hx_carry),
                                   P<uint64_t>(c->hx_base), P<uint32_t>(c->hx_head), P<uint64_t>(c->hx_rowlen),
                                   P<int64_t>(c->hx_bstart), P<int64_t>(c->hx_bend), c->stream));
        r = exclusive_scan(c, P<uint64_t>(c->hx_rowlen), P<uint64_t>(c->hx_rowoff), (size_t)nb + 1);
        prof_end(c, "hx_layout");
        if (r) return r;
        static thread_local uint64_t tail;
        HIPCHK(c, hipMemcpyAsync(&tail, P<uint64_t>(c->hx_rowoff) + nb, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->hx_text = tail;
    }
    prof_collect(c);
    mark_done(c, c->hx_laid);
    if (out) {
        out->n_lines = c->n_lines;
        out->rows = nb;
        out->data_lines = nm;
        out->text_bytes = c->hx_text;
    }
    return VCFXG_OK;
}

int vcfxg_haplotype_table(vcfxg_ctx *c, uint64_t first, uint64_t count, uint64_t *first_member, uint64_t *last_member,
                          int64_t *start, int64_t *end, uint64_t *row_off, uint64_t *row_len) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->hx_scanned) || !is_done(c, c->hx_laid)) return VCFXG_E_STATE;
    if (first > c->hx_nb || count > c->hx_nb - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    int r = hx_fetch(c, c->hx_first, first, count, first_member);
    if (!r) r = hx_fetch(c, c->hx_last, first, count, last_member);
    if (!r) r = hx_fetch(c, c->hx_bstart, first, count, start);
    if (!r) r = hx_fetch(c, c->hx_bend, first, count, end);
    if (!r) r = hx_fetch(c, c->hx_rowoff, first, count, row_off);
    if (!r) r = hx_fetch(c, c->hx_rowlen, first, count, row_len);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_haplotype_text(vcfxg_ctx *c, vcfxg_summary *out) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->hx_scanned) || !is_done(c, c->hx_laid)) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    if (out) std::memset(out, 0, sizeof *out);
    const uint64_t nm = c->hx_nm, nb = c->hx_nb;
    const int r = ensure(c, c->text, c->hx_text + 16);
    if (r) return r;
    c->text_bytes = c->hx_text;
    const char *buf = P<char>(c->input);
    const uint64_t *le = P<uint64_t>(c->line_end);
    prof_begin(c, "hx_heads");
    HIPCHK(c, launch_hx_heads(buf, (int64_t)c->data_start, le, nb, P<uint64_t>(c->hx_first), P<uint64_t>(c->hx_mline),
                              P<uint32_t>(c->hx_clen), P<int64_t>(c->hx_bstart), P<int64_t>(c->hx_bend),
                              P<uint64_t>(c->hx_rowoff), P<uint64_t>(c->hx_rowlen), P<char>(c->text), c->stream));
    prof_end(c, "hx_heads");
    prof_begin(c, "hx_emit");
    HIPCHK(c, launch_hx_emit(buf, (int64_t)c->data_start, le, nm, c->hx_ns, P<uint64_t>(c->hx_mline), P<uint32_t>(c->hx_start),
                             P<uint64_t>(c->hx_bnum), P<uint32_t>(c->hx_fixed), P<uint64_t>(c->hx_cells), P<uint64_t>(c->hx_carry),
                             P<uint64_t>(c->hx_base),
                             P<uint32_t>(c->hx_head), P<uint64_t>(c->hx_rowoff), P<char>(c->text), c->stream));
    prof_end(c, "hx_emit");
    prof_collect(c);
    if (out) {
        out->n_lines = c->n_lines;
        out->rows = nb;
        out->data_lines = nm;
        out->text_bytes = c->hx_text;
    }
    return VCFXG_OK;
}

}  // extern "C"
