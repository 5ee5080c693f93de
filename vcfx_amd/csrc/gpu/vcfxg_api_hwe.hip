// vcfxg_api_hwe.hip -- VCFX_hwe_tester (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"

using namespace vcfxg;

extern "C" {

// VCFX_hwe_tester over [data_start, n).  walk: the AF walk with the HWE reducer (records of
// >= 512 B on average), its compaction and k_hwe_lines for the lines it left; else the line
// index and k_hwe_lines on every line.  Then the row rules + lengths, the scan, the rows into
// the previous call's text capacity and ONE host synchronisation (as af_region_walk); rows
// past the capacity are formatted again once it has grown.  A walker over its line capacity
// reruns the call without the walk.
static int hwe_region_impl(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out, bool walk) {
    new_index(c);
    HIPCHK(c, hipSetDevice(c->device));
    const WalkPlan pl = walk_plan(c, data_start);
    const int64_t lo = pl.lo;
    walk = walk && pl.nw > 0;
    const char *buf = P<char>(c->input);
    int r = ensure(c, c->wk_small, 128);
    if (r) return r;
    uint64_t *small = P<uint64_t>(c->wk_small);  // [0] overflow flag, [4..10] summary, [11] rechecks
    unsigned *ovf = reinterpret_cast<unsigned *>(small);
    uint64_t cap = 0;
    if (walk) {
        // (no pl.fits_gt16 check: the packed GT-line count it guards goes to counters[0..1], which
        // are zeroed below before anything reads them)
        cap = pl.cap;
        r = ensure(c, c->hwe_rc, sizeof(vcfxg_hwe_recheck) * (cap + 1));
        // mode 0: both HWE modes strip the trailing '\r' before the record is parsed
        if (!r) r = af_walk_to_dense(c, pl, 0, "hwe_walk", 96, true, false, false);
        if (r) return r;
    } else {
        uint64_t L = 0;
        r = vcfxg_index(c, data_start, &L);
        if (r) return r;
        cap = L;
        r = af_buffers(c, cap, StatusOwner::other);
        if (!r) r = ensure(c, c->hwe_aux, 4 * (cap + 1));
        if (!r) r = ensure(c, c->hwe_rc, sizeof(vcfxg_hwe_recheck) * (cap + 1));
        if (r) return r;
        HIPCHK(c, hipMemsetAsync(small, 0, 96, c->stream));
    }
    // (the walk's compaction counts GT lines for AF in counters[0..1]: rows are counted below)
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    prof_begin(c, "hwe_lines");
    HIPCHK(c, vcfxg::launch_hwe_lines(buf, lo, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), cap, mode,
                                      walk ? c->af_meta.p : nullptr, P<int32_t>(c->alt), P<int32_t>(c->tot),
                                      P<int32_t>(c->hwe_aux), P<uint32_t>(c->rowpre), P<uint8_t>(c->status),
                                      P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "hwe_lines");
    prof_begin(c, "hwe_rows");
    HIPCHK(c, vcfxg::launch_hwe_rowlen(P<uint64_t>(c->d_nlines), cap, mode, walk ? c->af_meta.p : nullptr,
                                       P<uint32_t>(c->rowpre), P<uint8_t>(c->status), P<uint64_t>(c->rowlen),
                                       P<unsigned long long>(c->counters), c->stream));
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)cap + 1);
    if (r) return r;
    HIPCHK(c, vcfxg::launch_af_summary(P<uint64_t>(c->d_nlines), P<uint64_t>(c->rowoff),
                                       P<unsigned long long>(c->counters), ovf, small + 4, c->stream));
    prof_end(c, "hwe_rows");
    const uint64_t tcap = std::max<uint64_t>(c->text_hint, 1u << 16);
    r = ensure(c, c->text, tcap + 1);
    if (r) return r;
    unsigned long long *rc_n = reinterpret_cast<unsigned long long *>(small + 11);
    prof_begin(c, "hwe_format");
    HIPCHK(c, vcfxg::launch_hwe_format(buf, lo, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), cap, mode,
                                       P<int32_t>(c->alt), P<int32_t>(c->tot), P<int32_t>(c->hwe_aux),
                                       P<uint32_t>(c->rowpre), P<uint8_t>(c->status), P<uint64_t>(c->rowoff),
                                       P<char>(c->text), tcap, c->hwe_ulps, c->hwe_rc.p, rc_n, cap + 1, c->stream));
    prof_end(c, "hwe_format");
    static thread_local uint64_t sm[8];
    HIPCHK(c, hipMemcpyAsync(sm, small + 4, sizeof sm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (walk && sm[6]) {  // a walker ran out of line slots (short lines): no walk
        prof_collect(c);
        c->walk_overflowed = true;
        return hwe_region_impl(c, data_start, mode, out, false);
    }
    const uint64_t L = sm[0], text = sm[1];
    c->text_hint = text;
    if (text > tcap) {  // the text outgrew the previous capacity: all rows again
        r = ensure(c, c->text, text + 1);
        if (r) return r;
        HIPCHK(c, hipMemsetAsync(rc_n, 0, 8, c->stream));
        prof_begin(c, "hwe_format");
        HIPCHK(c, vcfxg::launch_hwe_format(buf, lo, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), L, mode,
                                           P<int32_t>(c->alt), P<int32_t>(c->tot), P<int32_t>(c->hwe_aux),
                                           P<uint32_t>(c->rowpre), P<uint8_t>(c->status), P<uint64_t>(c->rowoff),
                                           P<char>(c->text), ~0ull, c->hwe_ulps, c->hwe_rc.p, rc_n, cap + 1,
                                           c->stream));
        prof_end(c, "hwe_format");
        HIPCHK(c, hipMemcpyAsync(&sm[7], rc_n, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    prof_collect(c);
    c->data_start = data_start;
    c->n_lines = L;
    c->indexed = true;
    c->text_bytes = text;
    c->hwe_rc_n = sm[7];
    if (out) {
        out->n_lines = L;
        out->rows = sm[2];
        out->data_lines = 0;
        out->warn_lines = 0;
        out->general_records = sm[5];
        out->text_bytes = text;
    }
    return VCFXG_OK;
}

int vcfxg_hwe_region(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out) {
    if (!c || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    if (data_start > c->n) data_start = c->n;
    // the AF schedule knob selects here too: 3 / 8 = no walk, 7 = the walk
    const bool walk = c->af_path == 7 || (af_knob_allows_walk(c) && walk_wanted(c, true));
    return hwe_region_impl(c, data_start, mode, out, walk);
}

int vcfxg_hwe_rechecks(vcfxg_ctx *c, vcfxg_hwe_recheck *out, uint64_t cap, uint64_t *n) {
    if (!c || !n || (!out && cap)) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    *n = c->hwe_rc_n;
    const uint64_t k = std::min(cap, c->hwe_rc_n);
    if (!k) return VCFXG_OK;
    HIPCHK(c, hipMemcpyAsync(out, c->hwe_rc.p, k * sizeof(vcfxg_hwe_recheck), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

}  // extern "C"
