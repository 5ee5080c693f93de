// vcfxg_api_cc.hip -- VCFX_cross_sample_concordance (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"

using namespace vcfxg;

extern "C" {

// walk: the record walk with the concordance reducer (records of >= 512 B on average, every
// header column selected once), its compaction and k_cc_lines for the lines it left; else the line
// index and k_cc_lines on every line.  Then the data lines' ordinals (a scan), the row lengths at
// their output places, their scan, the rows into the previous call's text capacity and ONE host
// synchronisation (as hwe_region_impl); rows past the capacity are formatted again once it has
// grown.  A walker over its line capacity reruns the call without the walk.
static int cc_region_impl(vcfxg_ctx *c, size_t data_start, int mode, const vcfxg_cc_params *p, uint32_t ns,
                          vcfxg_summary *out, bool walk) {
    new_index(c);
    HIPCHK(c, hipSetDevice(c->device));
    const WalkPlan pl = walk_plan(c, data_start);
    const int64_t lo = pl.lo;
    walk = walk && pl.nw > 0;
    const char *buf = P<char>(c->input);
    int r = ensure(c, c->wk_small, 128);
    if (!r) r = ensure(c, c->cc_small, 64);
    if (r) return r;
    unsigned *ovf = P<unsigned>(c->wk_small);
    uint64_t cap = 0;
    if (walk) {
        cap = pl.cap;
        // mode 0: the file mode strips the trailing '\r' before the record is parsed
        r = af_walk_to_dense(c, pl, mode == VCFXG_MODE_FILE ? 0 : 1, "cc_walk", 96, false, false, false, true);
        if (r) return r;
        note_schedule(c, "cc_walk");
    } else {
        uint64_t L = 0;
        r = vcfxg_index(c, data_start, &L);
        if (r) return r;
        note_schedule(c, "cc_two_sweep");
        if (!L) {  // nothing after data_start
            if (out) std::memset(out, 0, sizeof *out);
            return VCFXG_OK;
        }
        cap = L;
        r = af_buffers(c, cap, StatusOwner::other);
        if (r) return r;
        HIPCHK(c, hipMemsetAsync(c->wk_small.p, 0, 96, c->stream));
    }
    r = ensure(c, c->cc_isdata, 4 * (cap + 1));
    if (!r) r = ensure(c, c->cc_ord, 8 * (cap + 1));
    if (r) return r;
    // (the walk's compaction counts GT lines for AF in counters[0..1]: rows are counted below)
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(c->cc_isdata.p, 0, 4 * (cap + 1), c->stream));
    HIPCHK(c, hipMemsetAsync(c->rowlen.p, 0, 8 * (cap + 1), c->stream));
    const uint32_t *mult = p->mult ? P<uint32_t>(c->cc_mult) : nullptr;
    const uint64_t *nl = P<uint64_t>(c->d_nlines);
    prof_begin(c, "cc_lines");
    HIPCHK(c, vcfxg::launch_cc_lines(buf, lo, P<uint64_t>(c->line_end), nl, cap, mode, ns, mult, (uint32_t)p->n_mult,
                                     walk ? c->af_meta.p : nullptr, P<int32_t>(c->alt), P<int32_t>(c->tot),
                                     P<uint32_t>(c->rowpre), P<uint8_t>(c->status), P<uint32_t>(c->cc_isdata),
                                     P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "cc_lines");
    prof_begin(c, "cc_rows");
    r = exclusive_scan(c, P<uint32_t>(c->cc_isdata), P<uint64_t>(c->cc_ord), (size_t)cap + 1);
    if (r) return r;
    HIPCHK(c, vcfxg::launch_cc_rowlen(nl, cap, p->threads, P<uint64_t>(c->cc_ord), P<uint32_t>(c->cc_isdata),
                                      P<uint8_t>(c->status), P<int32_t>(c->alt), P<int32_t>(c->tot),
                                      P<uint32_t>(c->rowpre), P<uint64_t>(c->rowlen), c->stream));
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)cap + 1);
    if (r) return r;
    HIPCHK(c, vcfxg::launch_cc_summary(nl, P<uint64_t>(c->cc_ord), P<uint64_t>(c->rowoff),
                                       P<unsigned long long>(c->counters), ovf, P<uint64_t>(c->cc_small), c->stream));
    prof_end(c, "cc_rows");
    const uint64_t tcap = std::max<uint64_t>(c->text_hint, 1u << 16);
    r = ensure(c, c->text, tcap + 1);
    if (r) return r;
    auto format = [&](uint64_t text_cap) {
        prof_begin(c, "cc_format");
        const hipError_t e = vcfxg::launch_cc_format(buf, lo, P<uint64_t>(c->line_end), nl, cap, p->threads,
                                                     P<uint64_t>(c->cc_ord), P<uint8_t>(c->status), P<int32_t>(c->alt),
                                                     P<int32_t>(c->tot), P<uint32_t>(c->rowpre), P<uint64_t>(c->rowoff),
                                                     P<char>(c->text), text_cap, c->stream);
        prof_end(c, "cc_format");
        return e;
    };
    HIPCHK(c, format(tcap));
    static thread_local uint64_t sm[8];
    HIPCHK(c, hipMemcpyAsync(sm, c->cc_small.p, sizeof sm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (walk && sm[7]) {  // a walker ran out of line slots (short lines): no walk
        prof_collect(c);
        c->walk_overflowed = true;
        return cc_region_impl(c, data_start, mode, p, ns, out, false);
    }
    const uint64_t L = sm[6], text = sm[1];
    c->text_hint = text;
    if (text > tcap) {  // the text outgrew the previous capacity: all rows again
        r = ensure(c, c->text, text + 1);
        if (r) return r;
        HIPCHK(c, format(~0ull));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    prof_collect(c);
    c->data_start = data_start;
    c->n_lines = L;
    c->indexed = true;
    c->text_bytes = text;
    c->cc_totals[0] = sm[2];
    c->cc_totals[1] = sm[3];
    c->cc_totals[2] = sm[4];
    c->cc_totals[3] = sm[0];
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = L;
        out->rows = sm[2] + sm[3] + sm[4];
        out->data_lines = sm[0];
        out->text_bytes = text;
        out->general_records = sm[5];
    }
    return VCFXG_OK;
}

int vcfxg_concordance_region(vcfxg_ctx *c, size_t data_start, int mode, const vcfxg_cc_params *p, vcfxg_summary *out) {
    if (!c || !p || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN) || (p->n_mult && !p->mult) ||
        p->n_mult >= (1ull << 31) || p->n_samples >= (1u << 31))
        return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    if (data_start > c->n) data_start = c->n;
    HIPCHK(c, hipSetDevice(c->device));
    c->text_bytes = 0;
    std::memset(c->cc_totals, 0, sizeof c->cc_totals);
    // the walk's sweep counts every sample of a record once: right when each of ns columns is
    // selected once (k_cc_lines takes the records with another sample count)
    bool once = true;
    uint32_t ns = p->n_samples;
    if (p->mult) {
        for (uint64_t i = 0; i < p->n_mult && once; i++) once = p->mult[i] == 1u;
        if (mode == VCFXG_MODE_FILE) ns = (uint32_t)p->n_mult;  // (file mode has no field rule on ns)
        else once = once && p->n_mult == p->n_samples;
        int r = ensure(c, c->cc_mult, 4 * (size_t)p->n_mult + 4);
        if (r) return r;
        // (pageable host memory: the copy has left the caller's array when the call returns)
        HIPCHK(c, hipMemcpyAsync(c->cc_mult.p, p->mult, 4 * (size_t)p->n_mult, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    // the AF schedule knob selects here too: 3 / 8 = no walk, 7 = the walk
    const bool walk = once && ns > 0 && (c->af_path == 7 || (af_knob_allows_walk(c) && walk_wanted(c, true)));
    return cc_region_impl(c, data_start, mode, p, ns, out, walk);
}

int vcfxg_concordance_totals(const vcfxg_ctx *c, uint64_t totals[4]) {
    if (!c || !totals) return VCFXG_E_ARG;
    std::memcpy(totals, c->cc_totals, sizeof c->cc_totals);
    return VCFXG_OK;
}

int vcfxg_chrom_lines(vcfxg_ctx *c, size_t data_start, uint64_t *starts, uint64_t cap, uint64_t *n) {
    if (!c || !n || (!starts && cap)) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    *n = 0;
    uint64_t L = 0;
    int r = vcfxg_index(c, data_start, &L);
    if (r) return r;
    if (!L) return VCFXG_OK;
    r = ensure(c, c->cc_chrom, 8 * (cap + 1));
    if (!r) r = ensure(c, c->cc_small, 64);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->cc_small.p, 0, 8, c->stream));
    prof_begin(c, "cc_chrom");
    HIPCHK(c, vcfxg::launch_cc_chrom(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end),
                                     P<uint64_t>(c->d_nlines), L, P<uint64_t>(c->cc_chrom), cap,
                                     P<unsigned long long>(c->cc_small), c->stream));
    prof_end(c, "cc_chrom");
    static thread_local uint64_t k;
    HIPCHK(c, hipMemcpyAsync(&k, c->cc_small.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n = k;
    const uint64_t m = std::min(k, cap);
    if (m) {
        HIPCHK(c, hipMemcpyAsync(starts, c->cc_chrom.p, 8 * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::sort(starts, starts + m);
    }
    prof_collect(c);
    return VCFXG_OK;
}

}  // extern "C"
