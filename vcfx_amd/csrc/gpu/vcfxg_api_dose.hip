// vcfxg_api_dose.hip -- VCFX_dosage_calculator and VCFX_haplotype_phaser, which share the dosage
// walk as their line index (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"

using namespace vcfxg;

extern "C" {

// the dosage walk: line ends + per fixed-stride record its samples / "NA" samples, compacted to
// the dense per-line arrays (line_end, alt = ns, tot = na, status, af_meta = LineMeta); the
// context is indexed afterwards.  *overflow: a walker ran out of line slots (short lines)
static int dose_walk_index(vcfxg_ctx *c, size_t data_start, int mode, uint64_t *L_out, bool *overflow,
                           bool head) {
    new_index(c);
    HIPCHK(c, hipSetDevice(c->device));
    const WalkPlan pl = walk_plan(c, data_start);
    if (!pl.fits_gt16) {  // the caller's index path
        c->walk_overflowed = true;
        *overflow = true;
        return VCFXG_OK;
    }
    int r = af_walk_to_dense(c, pl, mode, "dose_walk", 16, false, true, head);
    if (r) return r;
    static thread_local uint64_t h[2];  // overflow flag, lines
    HIPCHK(c, hipMemcpyAsync(&h[0], c->wk_small.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&h[1], c->d_nlines.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *overflow = (h[0] & 0xFFFFFFFFull) != 0;
    if (*overflow) {
        c->walk_overflowed = true;
        return VCFXG_OK;
    }
    c->data_start = data_start;
    c->n_lines = h[1];
    c->indexed = true;
    *L_out = h[1];
    return VCFXG_OK;
}

// VCFX_dosage_calculator over [data_start, n): the line index, the row lengths, a scan, the
// rows (one host synchronisation for the text size).  Records of >= 512 B (a GT-dense VCF): the
// walk reads each record once for its line end and (fixed-stride records) its samples and "NA"
// samples -- no index sweep, no row-length pass over the records; the other lines take the
// exact row-length pass; VCFXG_DOSE_WALK=0 keeps the index + two-pass schedule
//
// On such input the first attempt is the HEAD walk (DoseHeadOp): a GT-only record whose '\n' is
// where the previous fixed-stride record predicts it is taken as a fixed-stride row without
// "NA" and its samples are not read by the walk -- only the record heads are -- so the input is
// read about once in all (by k_dose_fmt, which checks every sample byte of those rows while it
// writes them).  A row that fails the check (an "NA", a wider sample, ...) flags the call,
// which is then redone with the sweeping walk; an input that failed once keeps the sweeping
// walk until the next load.  VCFXG_DOSE_HEAD=0 always sweeps.
static int dose_walk_index(vcfxg_ctx *c, size_t data_start, int mode, uint64_t *L_out, bool *overflow, bool head);
static int dosage_region_once(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out, bool head, bool *redo);

int vcfxg_dosage_region(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out) {
    if (!c || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    if (data_start > c->n) data_start = c->n;
    static const bool head_ok = [] {
        const char *e = getenv("VCFXG_DOSE_HEAD");
        return !(e && e[0] == '0');
    }();
    bool redo = false;
    int r = dosage_region_once(c, data_start, mode, out, head_ok && !c->dose_head_failed, &redo);
    if (r || !redo) return r;
    c->dose_head_failed = true;
    return dosage_region_once(c, data_start, mode, out, false, &redo);
}

static int dosage_region_once(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out, bool head, bool *redo) {
    static const bool walk_ok = [] {
        const char *e = getenv("VCFXG_DOSE_WALK");
        return !(e && e[0] == '0');
    }();
    const bool walk = walk_ok && af_knob_allows_walk(c) && walk_wanted(c, true) && walk_plan(c, data_start).nw > 0;
    uint64_t L = 0;
    int r;
    bool walked = false;
    head = head && walk;
    if (walk) {
        bool ovf = false;
        r = dose_walk_index(c, data_start, mode, &L, &ovf, head);
        if (r) return r;
        walked = !ovf;
    }
    head = head && walked;
    if (!walked) {
        r = vcfxg_index(c, data_start, &L);
        if (r) return r;
    }
    HIPCHK(c, hipSetDevice(c->device));
    r = af_buffers(c, L, StatusOwner::other);
    if (!r) r = ensure(c, c->dose_meta, vcfxg::dose_meta_bytes() * (L + 1));
    if (r) return r;
    const char *buf = P<char>(c->input);
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->rowlen) + L, 0, 8, c->stream));
    prof_begin(c, "dose_len");
    if (walked)
        HIPCHK(c, vcfxg::launch_dose_from_walk(P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), L, c->af_meta.p,
                                               P<int32_t>(c->alt), P<int32_t>(c->tot), P<uint8_t>(c->status),
                                               P<uint64_t>(c->rowlen), c->dose_meta.p,
                                               P<unsigned long long>(c->counters), c->stream));
    HIPCHK(c, vcfxg::launch_dose_len(buf, (int64_t)data_start, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), L,
                                     mode, P<uint8_t>(c->status), P<uint64_t>(c->rowlen), c->dose_meta.p,
                                     P<unsigned long long>(c->counters), c->stream, walked));
    prof_end(c, "dose_len");
    prof_begin(c, "dose_rows");
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)L + 1);
    if (r) return r;
    prof_end(c, "dose_rows");
    static thread_local uint64_t tail[6];
    HIPCHK(c, hipMemcpyAsync(&tail[0], P<uint64_t>(c->rowoff) + L, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&tail[1], c->counters.p, 40, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t text = tail[0];
    r = ensure(c, c->text, text + 1);
    if (r) return r;
    // (the head walk's rows are checked by the formatting pass: a failed check flags the call)
    unsigned *bad = head ? reinterpret_cast<unsigned *>(P<uint64_t>(c->wk_small) + 4) : nullptr;
    static thread_local unsigned bad_h;
    bad_h = 0;
    if (bad) HIPCHK(c, hipMemsetAsync(bad, 0, 4, c->stream));
    prof_begin(c, "dose_fmt");
    HIPCHK(c, vcfxg::launch_dose_fmt(buf, (int64_t)data_start, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), L,
                                     P<uint8_t>(c->status), c->dose_meta.p, P<uint64_t>(c->rowoff), P<char>(c->text),
                                     ~0ull, tail[2], c->stream, bad, tail[5]));
    prof_end(c, "dose_fmt");
    if (bad) HIPCHK(c, hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (bad_h) {  // some row the head walk took is not a fixed-stride row without "NA": redo
        *redo = true;
        c->text_bytes = 0;
        return VCFXG_OK;
    }
    c->text_bytes = text;
    if (out) {
        out->n_lines = L;
        out->rows = tail[1];
        out->data_lines = tail[1] + tail[3];
        out->warn_lines = tail[3];
        out->general_records = tail[4];
        out->text_bytes = text;
    }
    return VCFXG_OK;
}

// VCFX_haplotype_phaser over [data_start, n): index, the per-line parse into genotype rows, the
// variant compaction (one host synchronisation for the variant count), the pair pass, a scan
// and the entries (a second synchronisation)
// VCFX_haplotype_phaser.  Records of >= 512 B, GT-only (a GT-dense VCF): the line index comes
// from the dosage HEAD walk (record heads only; a GT-only record whose '\n' is where the
// previous fixed-stride record predicts it is taken unswept), and k_ph_lines' fixed-stride
// sweep, which reads every record anyway, validates the unswept records' interiors; a record it
// cannot validate flags the call, which is redone on vcfxg_index (and this input keeps the
// index).  VCFXG_PH_WALK=0: always the index.
static int phaser_once(vcfxg_ctx *c, size_t data_start, int mode, double thr, uint32_t hint, vcfxg_summary *out,
                       bool walk, bool *redo);

int vcfxg_haplotype_phaser(vcfxg_ctx *c, size_t data_start, int mode, double thr, uint32_t hint, vcfxg_summary *out) {
    if (!c || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    if (data_start > c->n) data_start = c->n;
    static const bool walk_ok = [] {
        const char *e = getenv("VCFXG_PH_WALK");
        return !(e && e[0] == '0');
    }();
    const bool walk = walk_ok && !c->ph_head_failed && af_knob_allows_walk(c) && walk_wanted(c, true) &&
                      walk_plan(c, data_start).nw > 0;
    bool redo = false;
    int r = phaser_once(c, data_start, mode, thr, hint, out, walk, &redo);
    if (r || !redo) return r;
    c->ph_head_failed = true;
    return phaser_once(c, data_start, mode, thr, hint, out, false, &redo);
}

static int phaser_once(vcfxg_ctx *c, size_t data_start, int mode, double thr, uint32_t hint, vcfxg_summary *out,
                       bool walk, bool *redo) {
    *redo = false;
    uint64_t L = 0;
    int r;
    bool walked = false;
    if (walk) {
        bool ovf = false;
        note_schedule(c, "ph_head_walk");
        r = dose_walk_index(c, data_start, mode, &L, &ovf, true);
        if (r) return r;
        walked = !ovf;
    }
    if (!walked) {
        note_schedule(c, "ph_index");
        r = vcfxg_index(c, data_start, &L);
        if (r) return r;
    }
    HIPCHK(c, hipSetDevice(c->device));
    unsigned *bad = walked ? reinterpret_cast<unsigned *>(P<uint64_t>(c->wk_small) + 4) : nullptr;
    const char *buf = P<char>(c->input);
    uint64_t kpad = ((uint64_t)std::max<uint32_t>(hint, 16) + 15) & ~15ull;
    static thread_local uint64_t h[2];
    for (int pass = 0;; pass++) {
        r = ensure(c, c->ph_G, L * kpad + 16);
        if (!r) r = af_buffers(c, L, StatusOwner::other);
        if (!r) r = ensure(c, c->ph_isvar, 4 * (L + 1));
        if (!r) r = ensure(c, c->ph_info, vcfxg::ph_line_bytes() * (L + 1));
        if (!r) r = ensure(c, c->ph_vnum, 8 * (L + 1));
        if (!r) r = ensure(c, c->ph_vline, 8 * (L + 1));
        if (r) return r;
        HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
        HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->counters) + 4, 0, 8, c->stream));
        if (bad) HIPCHK(c, hipMemsetAsync(bad, 0, 4, c->stream));
        prof_begin(c, "ph_lines");
        HIPCHK(c, vcfxg::launch_ph_lines(buf, (int64_t)data_start, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), L,
                                         mode, (uint32_t)kpad, P<int8_t>(c->ph_G), P<uint8_t>(c->status),
                                         P<uint32_t>(c->ph_isvar), c->ph_info.p, P<unsigned long long>(c->counters),
                                         c->stream, walked ? c->af_meta.p : nullptr, bad));
        prof_end(c, "ph_lines");
        if (L) {
            r = exclusive_scan(c, P<uint32_t>(c->ph_isvar), P<uint64_t>(c->ph_vnum), (size_t)L);
            if (r) return r;
            HIPCHK(c, vcfxg::launch_ph_compact(P<uint32_t>(c->ph_isvar), P<uint64_t>(c->ph_vnum), P<uint64_t>(c->d_nlines),
                                               L, P<uint64_t>(c->ph_vline), P<uint64_t>(c->counters) + 4, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(h, P<uint64_t>(c->counters) + 3, 16, hipMemcpyDeviceToHost, c->stream));
        static thread_local unsigned bad_h;
        bad_h = 0;
        if (bad) HIPCHK(c, hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (bad_h) {  // an unswept record the parse could not validate: the call again on the index
            *redo = true;
            return VCFXG_OK;
        }
        if (h[0] > kpad && pass == 0) {  // a record wider than the rows: once more with rows that fit
            kpad = (h[0] + 15) & ~15ull;
            continue;
        }
        break;
    }
    const uint64_t V = h[1];
    r = ensure(c, c->ph_flags, V + 1);
    if (!r) r = ensure(c, c->ph_r2, 8 * (V + 1));
    if (!r) r = ensure(c, c->rowlen, 8 * (V + 1));
    if (!r) r = ensure(c, c->rowoff, 8 * (V + 1));
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->rowlen) + V, 0, 8, c->stream));
    prof_begin(c, "ph_pairs");
    HIPCHK(c, vcfxg::launch_ph_pairs(buf, P<uint64_t>(c->ph_vline), P<uint64_t>(c->counters) + 4, V, c->ph_info.p,
                                     P<int8_t>(c->ph_G), (uint32_t)kpad, thr, P<uint8_t>(c->ph_flags),
                                     P<uint64_t>(c->rowlen), P<double>(c->ph_r2), c->stream));
    prof_end(c, "ph_pairs");
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)V + 1);
    if (r) return r;
    static thread_local uint64_t text;
    HIPCHK(c, hipMemcpyAsync(&text, P<uint64_t>(c->rowoff) + V, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    r = ensure(c, c->text, text + 1);
    if (r) return r;
    prof_begin(c, "ph_fmt");
    HIPCHK(c, vcfxg::launch_ph_fmt(buf, P<uint64_t>(c->ph_vline), P<uint64_t>(c->counters) + 4, V, c->ph_info.p,
                                   P<uint64_t>(c->rowoff), P<char>(c->text), c->stream));
    prof_end(c, "ph_fmt");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = text;
    c->ph_nvar = V;
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = L;
        out->rows = V;
        out->text_bytes = text;
    }
    return VCFXG_OK;
}

int vcfxg_phaser_variants(vcfxg_ctx *c, uint8_t *flags, double *r2, uint64_t *offs) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    const uint64_t V = c->ph_nvar;
    if (flags && V) HIPCHK(c, hipMemcpyAsync(flags, c->ph_flags.p, V, hipMemcpyDeviceToHost, c->stream));
    if (r2 && V) HIPCHK(c, hipMemcpyAsync(r2, c->ph_r2.p, 8 * V, hipMemcpyDeviceToHost, c->stream));
    if (offs) HIPCHK(c, hipMemcpyAsync(offs, c->rowoff.p, 8 * (V + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

}  // extern "C"
