// vcfxg_api_ib.hip -- VCFX_inbreeding_calculator (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"

using namespace vcfxg;

extern "C" {

// VCFX_inbreeding_calculator.  The records are taken in blocks: ib_block indexed lines on the
// index schedule; on the walk schedule whole walkers, max(ib_block / cap_w, 1) of them with cap_w
// line slots each (so a block there holds at most about ib_block lines, and at least one
// walker's).  Per block: stage A (the walk over the block's chunks, or the per-line kernel), the
// per-record table and the per-sample chain, all on the context's stream; the per-sample state
// stays on the device between the blocks.  One host synchronisation at the end (the walk's
// overflow flag, the counts, the text size); a walker overflow repeats the call on the index.
static int ib_region_impl(vcfxg_ctx *c, size_t data_start, int mode, const vcfxg_ib_params *p, vcfxg_summary *out,
                          bool walk) {
    new_index(c);
    HIPCHK(c, hipSetDevice(c->device));
    const WalkPlan pl = walk_plan(c, data_start);  // (k_ib_walk packs no 16-bit count: no fits_gt16 check)
    const int64_t lo = pl.lo, hi = pl.hi, C = pl.C, nw = pl.nw;
    walk = walk && nw > 0;
    const char *buf = P<char>(c->input);
    const uint32_t ns = p->n_samples, ld = (ns + 15u) & ~15u;
    const uint64_t nb = p->name_off[ns];
    c->ac_noff_host.assign(p->name_off, p->name_off + ns + 1);
    c->ac_names_host.assign(p->names ? p->names : "", (size_t)nb);
    int r = ensure(c, c->ib_small, 64);
    if (!r) r = ensure(c, c->ib_sum, 8 * (size_t)ns);
    if (!r) r = ensure(c, c->ib_obs, 8 * (size_t)ns);
    if (!r) r = ensure(c, c->ib_used, 8 * (size_t)ns);
    if (!r) r = ensure(c, c->ib_carried, 4 * (size_t)ns);
    if (!r) r = ensure(c, c->ac_noff, 8 * ((size_t)ns + 1));
    if (!r) r = ensure(c, c->ac_names, nb + 1);
    const uint64_t tcap = nb + (uint64_t)ns * 50;  // a row: name, '\t', at most 47 value bytes, '\n'
    if (!r) r = ensure(c, c->text, tcap + 1);
    if (r) return r;
    c->ib_ns = 0;
    uint64_t *small = P<uint64_t>(c->ib_small);  // [0] overflow flag, [1] text bytes
    unsigned *ovf = reinterpret_cast<unsigned *>(small);
    unsigned long long *counters = P<unsigned long long>(c->counters);
    HIPCHK(c, hipMemsetAsync(small, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(counters, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ib_sum.p, 0, 8 * (size_t)ns, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ib_obs.p, 0, 8 * (size_t)ns, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ib_used.p, 0, 8 * (size_t)ns, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ib_carried.p, 0, 4 * (size_t)ns, c->stream));  // (:532: the buffer starts as zeros)
    HIPCHK(c, hipMemcpyAsync(c->ac_noff.p, c->ac_noff_host.data(), 8 * ((size_t)ns + 1), hipMemcpyHostToDevice, c->stream));
    if (nb) HIPCHK(c, hipMemcpyAsync(c->ac_names.p, c->ac_names_host.data(), nb, hipMemcpyHostToDevice, c->stream));
    const int glob = p->freq_mode == 1, skipb = p->skip_boundary != 0, countb = p->count_boundary_as_used != 0;
    auto block = [&](uint32_t G, uint32_t cap_w) -> int {
        prof_begin(c, "ib_table");
        HIPCHK(c, vcfxg::launch_ib_table(c->ib_meta.p, P<uint32_t>(c->ib_cnt), P<uint32_t>(c->ib_offs), G, cap_w, glob,
                                         c->ib_tab.p, c->stream));
        prof_end(c, "ib_table");
        prof_begin(c, "ib_pack");
        HIPCHK(c, vcfxg::launch_ib_pack(P<int8_t>(c->ib_codes), ld, c->ib_tab.p, P<uint32_t>(c->ib_offs) + G,
                                        (uint64_t)G * cap_w, c->ib_packed.p, ns, c->stream));
        prof_end(c, "ib_pack");
        prof_begin(c, "ib_chain");
        HIPCHK(c, vcfxg::launch_ib_chain(c->ib_tab.p, P<uint32_t>(c->ib_offs) + G, (uint64_t)G * cap_w, c->ib_packed.p,
                                         ns, mode, skipb, countb, P<double>(c->ib_sum), P<uint64_t>(c->ib_obs),
                                         P<uint64_t>(c->ib_used), P<int32_t>(c->ib_carried), c->stream));
        prof_end(c, "ib_chain");
        return VCFXG_OK;
    };
    auto buffers = [&](uint64_t slots, uint64_t groups) -> int {
        int q = ensure(c, c->ib_codes, slots * ld + 16);
        if (!q) q = ensure(c, c->ib_meta, vcfxg::ib_meta_bytes() * slots);
        if (!q) q = ensure(c, c->ib_tab, vcfxg::ib_rec_bytes() * (slots + 16));
        if (!q) q = ensure(c, c->ib_packed, vcfxg::ib_packed_bytes(slots, ns));
        if (!q) q = ensure(c, c->ib_cnt, 4 * groups);
        if (!q) q = ensure(c, c->ib_offs, 4 * (groups + 1));
        return q;
    };
    uint64_t L = 0;
    if (walk) {
        const uint64_t cap_w = pl.cap_w;
        const uint64_t G = std::min<uint64_t>(std::max<uint64_t>(c->ib_block / cap_w, 1), (uint64_t)nw);
        r = buffers(G * cap_w, G);
        if (r) return r;
        note_schedule(c, "ib:walk");
        for (int64_t w0 = 0; w0 < nw; w0 += (int64_t)G) {
            const uint32_t g = (uint32_t)std::min<int64_t>((int64_t)G, nw - w0);
            prof_begin(c, "ib_walk");
            HIPCHK(c, vcfxg::launch_ib_walk(buf, lo, hi, C, w0, nw, g, (uint32_t)cap_w, mode, ns, ld,
                                            P<int8_t>(c->ib_codes), c->ib_meta.p, P<uint32_t>(c->ib_cnt), ovf, counters,
                                            c->stream));
            prof_end(c, "ib_walk");
            r = block(g, (uint32_t)cap_w);
            if (r) return r;
        }
    } else {
        r = vcfxg_index(c, data_start, &L);
        if (r) return r;
        const uint64_t B = std::max<uint64_t>(std::min<uint64_t>(c->ib_block, L), 1);
        r = buffers(B, 1);
        if (r) return r;
        note_schedule(c, "ib:index");
        for (uint64_t l0 = 0; l0 < L; l0 += B) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(B, L - l0);
            prof_begin(c, "ib_lines");
            HIPCHK(c, vcfxg::launch_ib_lines(buf, lo, P<uint64_t>(c->line_end), l0, n, mode, ns, ld,
                                             P<int8_t>(c->ib_codes), c->ib_meta.p, P<uint32_t>(c->ib_cnt), counters,
                                             c->stream));
            prof_end(c, "ib_lines");
            r = block(1, (uint32_t)B);
            if (r) return r;
        }
    }
    prof_begin(c, "ib_rows");
    HIPCHK(c, vcfxg::launch_ib_rows(P<double>(c->ib_sum), P<uint64_t>(c->ib_obs), P<uint64_t>(c->ib_used), ns,
                                    P<char>(c->ac_names), P<uint64_t>(c->ac_noff), P<char>(c->text), small + 1,
                                    c->stream));
    prof_end(c, "ib_rows");
    static thread_local uint64_t sm[2];
    static thread_local unsigned long long cn[4];
    HIPCHK(c, hipMemcpyAsync(sm, small, sizeof sm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cn, counters, sizeof cn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (walk && (sm[0] & 0xFFFFFFFFu)) {  // a walker ran out of line slots (short lines): no walk
        c->walk_overflowed = true;
        return ib_region_impl(c, data_start, mode, p, out, false);
    }
    c->ib_ns = ns;
    c->text_bytes = sm[1];
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = cn[3];
        out->rows = cn[1];
        out->data_lines = cn[0];
        out->general_records = cn[2];
        out->text_bytes = sm[1];
    }
    return VCFXG_OK;
}

int vcfxg_inbreeding_region(vcfxg_ctx *c, size_t data_start, int mode, const vcfxg_ib_params *p, vcfxg_summary *out) {
    if (!c || !p || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN) || !p->n_samples || !p->name_off ||
        p->n_samples >= (1u << 30) || p->name_off[0] != 0 || (p->name_off[p->n_samples] && !p->names) ||
        p->freq_mode < 0 || p->freq_mode > 1)
        return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    if (data_start > c->n) data_start = c->n;
    // the AF schedule knob selects here too: 3 / 8 = the index, 7 = the walk
    const bool walk = c->af_path == 7 || (af_knob_allows_walk(c) && walk_wanted(c, false));
    return ib_region_impl(c, data_start, mode, p, out, walk);
}

int vcfxg_inbreeding_samples(vcfxg_ctx *c, double *sum_exp, uint64_t *obs_het, uint64_t *used) {
    if (!c) return VCFXG_E_ARG;
    if (!c->ib_ns) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t b = 8 * (size_t)c->ib_ns;
    if (sum_exp) HIPCHK(c, hipMemcpyAsync(sum_exp, c->ib_sum.p, b, hipMemcpyDeviceToHost, c->stream));
    if (obs_het) HIPCHK(c, hipMemcpyAsync(obs_het, c->ib_obs.p, b, hipMemcpyDeviceToHost, c->stream));
    if (used) HIPCHK(c, hipMemcpyAsync(used, c->ib_used.p, b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

}  // extern "C"
