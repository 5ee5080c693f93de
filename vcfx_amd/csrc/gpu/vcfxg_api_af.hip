// vcfxg_api_af.hip -- VCFX_allele_freq_calc: the per-line call, the two-sweep and walk region
// schedules and the dense per-line arrays of the last walk (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"

namespace vcfxg {

// the dense per-line arrays (line_end, alt, tot, rowpre, status, meta) of the last walk
// region call, compacted from its walker regions (k_walk_compact; counters discarded)
int ensure_dense(vcfxg_ctx *c) {
    if (!c->dense_pending) return VCFXG_OK;
    c->dense_pending = false;
    const uint64_t L = c->n_lines;
    int r = dense_buffers(c, L);
    if (!r) r = ensure(c, c->scratch_small, 64);
    if (r) return r;
    return walk_compact(c, c->dense_nw, c->dense_cap_w, P<unsigned long long>(c->scratch_small), false,
                        P<uint64_t>(c->wk_bs));
}

}  // namespace vcfxg

using namespace vcfxg;

extern "C" {

static int af_rows(vcfxg_ctx *c, int mode, vcfxg_summary *out);

int vcfxg_allele_freq(vcfxg_ctx *c, int mode, vcfxg_summary *out) {
    if (!c || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t L = c->n_lines;
    int r = af_buffers(c, L, StatusOwner::other);
    if (r) return r;
    const char *buf = P<char>(c->input);
    const uint64_t *nl_dev = P<uint64_t>(c->d_nlines);
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    r = ensure(c, c->af_meta, vcfxg::af_meta_bytes() * (L + 1));
    if (r) return r;
    prof_begin(c, "af_records");
    HIPCHK(c, vcfxg::launch_af_meta_sweep(buf, (int64_t)c->data_start, P<uint64_t>(c->line_end), nl_dev, L, mode,
                                          c->af_meta.p, P<int32_t>(c->alt), P<int32_t>(c->tot), P<uint32_t>(c->rowpre),
                                          P<uint8_t>(c->status), P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "af_records");
    return af_rows(c, mode, out);
}


// Default region path, asynchronous: the two-sweep schedule (index sweep + scan +
// compaction, head pass + fixed-stride sweep + the per-line rest, row lengths + scan) runs
// with the line count kept on the device -- buffers sized by the count of the previous call
// (else the no-overflow bound of idx_pos_cap() lines per 16 KiB chunk), compaction and
// kernels guarded by it -- and ONE host synchronisation reads a small summary (lines, text
// bytes, counters, failure) before the formatting kernel.  A failure (a chunk with more
// newlines than the scratch keeps, or more lines than the capacity) reruns the call on the
// synchronous path.
static int af_region_async(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out) {
    new_index(c);
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t lo = (int64_t)data_start, hi = (int64_t)c->n;
    const int64_t nc = vcfxg::idx_wchunks(lo, hi);
    if (!nc) {
        int r = vcfxg_index(c, data_start, nullptr);
        return r ? r : vcfxg_allele_freq(c, mode, out);
    }
    const size_t pcap = (size_t)vcfxg::idx_pos_cap();
    const uint64_t bound = (uint64_t)nc * pcap + 2;
    const uint64_t cap = c->af_line_cap ? std::min<uint64_t>(c->af_line_cap + 1, bound) : bound;
    int r = ensure(c, c->idx_counts, sizeof(uint32_t) * (size_t)(nc + 1));
    if (!r) r = ensure(c, c->idx_offs, sizeof(uint64_t) * (size_t)(nc + 1));
    if (!r) r = ensure(c, c->idx_pos, sizeof(uint64_t) * (size_t)nc * pcap + 64);
    if (!r) r = ensure(c, c->line_end, 8 * (cap + 1));
    if (!r) r = af_buffers(c, cap, StatusOwner::other);
    if (!r) r = ensure(c, c->af_meta, vcfxg::af_meta_bytes() * (cap + 1));
    if (!r) r = ensure(c, c->async_small, 128);
    if (r) return r;
    const char *buf = P<char>(c->input);
    uint64_t *small = P<uint64_t>(c->async_small);  // [0] 0, [1] n, [2] flags, [4..10] summary
    unsigned *idx_ovf = reinterpret_cast<unsigned *>(small + 2), *failf = idx_ovf + 1;
    HIPCHK(c, hipMemsetAsync(small, 0, 32, c->stream));
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    prof_begin(c, "line_count");
    HIPCHK(c, vcfxg::launch_idx_count(buf, lo, hi, P<uint32_t>(c->idx_counts), P<uint64_t>(c->idx_pos), idx_ovf,
                                      c->stream));
    prof_end(c, "line_count");
    HIPCHK(c, hipMemsetAsync(P<uint32_t>(c->idx_counts) + nc, 0, sizeof(uint32_t), c->stream));
    r = exclusive_scan(c, P<uint32_t>(c->idx_counts), P<uint64_t>(c->idx_offs), (size_t)nc + 1);
    if (r) return r;
    prof_begin(c, "line_compact");
    HIPCHK(c, vcfxg::launch_nl_compact_cap(lo, hi, P<uint32_t>(c->idx_counts), P<uint64_t>(c->idx_offs),
                                           P<uint64_t>(c->idx_pos), P<uint64_t>(c->line_end), cap, c->stream));
    HIPCHK(c, vcfxg::launch_idx_finish(P<uint64_t>(c->idx_offs), nc, idx_ovf, c->last_byte != '\n' ? 1 : 0, hi, cap,
                                       P<uint64_t>(c->line_end), small + 1, failf, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_nlines.p, small + 1, 8, hipMemcpyDeviceToDevice, c->stream));
    prof_end(c, "line_compact");
    prof_begin(c, "af_records");
    HIPCHK(c, vcfxg::launch_af_meta_sweep_range(buf, lo, P<uint64_t>(c->line_end), small, cap, mode, c->af_meta.p,
                                                P<int32_t>(c->alt), P<int32_t>(c->tot), P<uint32_t>(c->rowpre),
                                                P<uint8_t>(c->status), P<unsigned long long>(c->counters), c->stream));
    HIPCHK(c, vcfxg::launch_af_complex(buf, lo, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), cap, mode,
                                       c->af_meta.p, P<int32_t>(c->alt), P<int32_t>(c->tot), P<uint32_t>(c->rowpre),
                                       P<uint8_t>(c->status), P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "af_records");
    prof_begin(c, "af_rows");
    HIPCHK(c, vcfxg::launch_af_rowlen(P<uint32_t>(c->rowpre), P<uint8_t>(c->status), P<uint64_t>(c->d_nlines), cap,
                                      P<uint64_t>(c->rowlen), c->stream));
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)cap + 1);
    if (r) return r;
    HIPCHK(c, vcfxg::launch_af_summary(P<uint64_t>(c->d_nlines), P<uint64_t>(c->rowoff),
                                       P<unsigned long long>(c->counters), failf, small + 4, c->stream));
    prof_end(c, "af_rows");
    static thread_local uint64_t sm[7];
    HIPCHK(c, hipMemcpyAsync(sm, small + 4, sizeof sm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sm[6]) {  // rerun synchronously (and learn the exact line count)
        prof_collect(c);
        c->af_line_cap = 0;
        r = vcfxg_index(c, data_start, nullptr);
        if (!r) r = vcfxg_allele_freq(c, mode, out);
        if (!r) c->af_line_cap = c->n_lines;
        return r;
    }
    const uint64_t L = sm[0], text = sm[1];
    c->af_line_cap = std::max<uint64_t>(c->af_line_cap, L);
    r = ensure(c, c->text, text + 1);
    if (r) return r;
    prof_begin(c, "af_format");
    HIPCHK(c, vcfxg::launch_af_format(buf, lo, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), L, mode,
                                      P<int32_t>(c->alt), P<int32_t>(c->tot), P<uint32_t>(c->rowpre),
                                      P<uint8_t>(c->status), P<uint64_t>(c->rowoff), P<char>(c->text), c->stream));
    prof_end(c, "af_format");
    prof_collect(c);
    c->data_start = data_start;
    c->n_lines = L;
    c->indexed = true;
    c->text_bytes = text;
    if (out) {
        out->n_lines = L;
        out->rows = sm[2];
        out->data_lines = sm[3];
        out->warn_lines = sm[4];
        out->general_records = sm[5];
        out->text_bytes = text;
    }
    return VCFXG_OK;
}

// Walk region path (default when the first data lines average >= 512 B): no separate
// index sweep.  k_af_walk reads each chunk's lines once, predicting fixed-stride record ends
// and validating them by the sample sweep itself, and leaves per walker its lines' results,
// its rows' bytes and a list of the lines for the exact per-line path.  The tail works on the
// walkers' regions directly: k_af_cx (the listed lines), k_walker_scan (one block: walker line
// and text offsets + the call summary), k_af_format_w (rows, into the previous call's text
// capacity), then ONE host synchronisation.  The dense per-line arrays (line ends, counts,
// statuses) are compacted from the regions only when a later call asks for them
// (ensure_dense).  A walker over its line capacity, or an overlong leftover list, reruns the
// call on the two-sweep schedule (and later calls on this input use it directly).
static int af_region_walk(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out, bool gf = false) {
    new_index(c);
    HIPCHK(c, hipSetDevice(c->device));
    const WalkPlan pl = walk_plan(c, data_start, 0, !gf);  // (the GT-only walk: the plan's layout)
    const int64_t lo = pl.lo, hi = pl.hi, nw = pl.nw;
    if (!nw) {
        int r = vcfxg_index(c, data_start, nullptr);
        return r ? r : vcfxg_allele_freq(c, mode, out);
    }
    const uint64_t cap_w = pl.cap_w, cap = pl.cap;
    if (!pl.fits_gt16) {  // the two-sweep schedule, as after a walk that ran out of line slots
        c->walk_overflowed = true;
        return note_schedule(c, "af_two_sweep"), af_region_async(c, data_start, mode, out);
    }
    int r = walk_buffers(c, pl);
    if (!r) r = ensure(c, c->wk_text, 8 * (size_t)(nw + 1));
    if (!r) r = ensure(c, c->wk_toff, 8 * (size_t)(nw + 1));
    if (!r) r = ensure(c, c->wk_start, 8 * (size_t)(nw + 1));
    if (!r) r = ensure(c, c->wk_cx, 8 * cap);
    const int64_t nbs = (nw + vcfxg::kWalkerScanBlock - 1) / vcfxg::kWalkerScanBlock;
    if (!r) r = ensure(c, c->wk_bs, 8 * (size_t)(5 * nbs + 4));
    if (!r) r = ensure(c, c->af_small, 128);
    // a walker's rows as text: ~ 13 rows x 31 B on the config 2 shard; a walker whose rows
    // outgrow its stage is formatted from the arrays instead
    constexpr uint32_t kStageCap = 2048;
    if (!r) r = ensure(c, c->wk_stage, (size_t)kStageCap * (size_t)nw);
    if (!r) r = ensure(c, c->wk_dirty, (size_t)nw);
    if (r) return r;
    r = ensure_sum_host(c);
    if (r) return r;
    const char *buf = P<char>(c->input);
    // [0] walk overflow flag (u32), [1] leftover count, [2..5] counters: zero on entry (k_walker_scan
    // clears them for the next call); [6] walker-scan arrivals (u32, reset by its last block)
    uint64_t *bpre_a = P<uint64_t>(c->wk_bs), *bpre_b = bpre_a + nbs + 1, *bsum = bpre_b + nbs + 1;
    uint64_t *small = P<uint64_t>(c->af_small);
    unsigned *ovf = reinterpret_cast<unsigned *>(small);
    unsigned long long *cx_n = reinterpret_cast<unsigned long long *>(small + 1);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(small + 2);
    if (c->af_small_dirty) HIPCHK(c, hipMemsetAsync(small, 0, 128, c->stream));
    c->af_small_dirty = true;  // until the call has synchronised
    vcfxg::WalkTail tail;
    tail.wtext = P<uint64_t>(c->wk_text);
    tail.wstart = P<uint64_t>(c->wk_start);
    tail.cx_list = P<uint64_t>(c->wk_cx);
    tail.cx_n = cx_n;
    tail.cx_cap = cap;
    tail.stage = P<char>(c->wk_stage);
    tail.stage_cap = kStageCap;
    tail.wdirty = P<uint8_t>(c->wk_dirty);
    // (the GT-first walk has one sweep of its own)
    const int depth = gf ? vcfxg::kAfDepthDefault : pl.af_depth;
    const bool roll = !gf && pl.af_roll;
    if (!gf) {
        c->last_af_depth = depth, c->last_af_roll = roll;
        c->last_walk_layout = pl.lay, c->last_walk_layout_kind = pl.lay_kind, c->last_walk_resident = pl.resident;
    }
    prof_begin(c, "af_walk");
    HIPCHK(c, vcfxg::launch_af_walk(buf, lo, hi, pl.lay, mode, c->hint_span, cap_w, P<uint64_t>(c->wk_le),
                                    P<int32_t>(c->wk_alt), P<int32_t>(c->wk_tot), P<uint32_t>(c->wk_rowpre),
                                    P<uint8_t>(c->wk_status), c->wk_meta.p, P<uint64_t>(c->wk_count),
                                    P<uint32_t>(c->wk_gt), ovf, c->stream, nullptr, &tail, false, gf, false, depth,
                                    roll));
    prof_end(c, "af_walk");
    prof_begin(c, "af_complex");
    // the grid: a wave per leftover line of the previous call (usually none; 16 blocks at least)
    const uint64_t cx_grid_lines = std::min<uint64_t>(cap, std::max<uint64_t>(c->cx_hint, 64));
    HIPCHK(c, vcfxg::launch_af_cx(buf, mode, cap_w, tail.cx_list, cx_n, cap, cx_grid_lines, tail.wstart,
                                  P<uint64_t>(c->wk_le), c->wk_meta.p, P<int32_t>(c->wk_alt), P<int32_t>(c->wk_tot),
                                  P<uint32_t>(c->wk_rowpre), P<uint8_t>(c->wk_status), tail.wtext, cnt, c->stream));
    prof_end(c, "af_complex");
    prof_begin(c, "af_rows");
    uint64_t *sm = c->sum_host;  // lines, text bytes, counters[0..3], walk overflow, leftovers
    HIPCHK(c, vcfxg::launch_walker_scan(nw, P<uint64_t>(c->wk_count), tail.wtext, P<uint32_t>(c->wk_gt),
                                        P<uint64_t>(c->wk_offs), P<uint64_t>(c->wk_toff), bpre_a, bpre_b, bsum,
                                        reinterpret_cast<unsigned *>(small + 6), cnt, ovf, P<uint64_t>(c->d_nlines),
                                        c->sum_dev, c->stream, small));
    prof_end(c, "af_rows");
    // the rows go out before the host has seen their total: into the text capacity of the
    // previous call (rows past it are skipped, and all are written again below once it has
    // grown), so the call synchronises with the host once
    const uint64_t tcap = std::max<uint64_t>(c->text_hint, 1u << 16);
    r = ensure(c, c->text, tcap + 1);
    if (r) return r;
    prof_begin(c, "af_format");
    HIPCHK(c, vcfxg::launch_af_format_w(buf, mode, nw, cap_w, P<uint64_t>(c->wk_count), P<uint64_t>(c->wk_toff),
                                        bpre_b, tail.wstart, P<uint64_t>(c->wk_le), P<int32_t>(c->wk_alt),
                                        P<int32_t>(c->wk_tot), P<uint32_t>(c->wk_rowpre), P<uint8_t>(c->wk_status),
                                        P<char>(c->text), tcap, c->stream, &tail));
    prof_end(c, "af_format");
    // (the leftover list holds every slot at most once: it cannot overflow its capacity)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->af_small_dirty = false;
    c->cx_hint = sm[7];
    if (sm[6]) {  // a walker ran out of line slots (short lines): the two-sweep schedule
        prof_collect(c);
        c->walk_overflowed = true;
        return af_region_async(c, data_start, mode, out);
    }
    const uint64_t L = sm[0], text = sm[1];
    c->text_hint = text;
    if (text > tcap) {  // the text outgrew the previous capacity: all rows again
        r = ensure(c, c->text, text + 1);
        if (r) return r;
        prof_begin(c, "af_format");
        HIPCHK(c, vcfxg::launch_af_format_w(buf, mode, nw, cap_w, P<uint64_t>(c->wk_count), P<uint64_t>(c->wk_toff),
                                            bpre_b, tail.wstart, P<uint64_t>(c->wk_le), P<int32_t>(c->wk_alt),
                                            P<int32_t>(c->wk_tot), P<uint32_t>(c->wk_rowpre),
                                            P<uint8_t>(c->wk_status), P<char>(c->text), ~0ull, c->stream, &tail));
        prof_end(c, "af_format");
    }
    prof_collect(c);
    c->data_start = data_start;
    c->n_lines = L;
    c->indexed = true;
    c->text_bytes = text;
    c->dense_nw = nw;  // the dense arrays come from the regions on demand
    c->dense_cap_w = cap_w;
    c->dense_pending = true;
    if (out) {
        out->n_lines = L;
        out->rows = sm[2];
        out->data_lines = sm[3];
        out->warn_lines = sm[4];
        out->general_records = sm[5];
        out->text_bytes = text;
    }
    return VCFXG_OK;
}

int vcfxg_allele_freq_region(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out) {
    if (!c || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    if (data_start > c->n) data_start = c->n;
    if (c->af_path == 7) return note_schedule(c, "af_walk"), af_region_walk(c, data_start, mode, out);
    if (c->af_path == 8) return note_schedule(c, "af_two_sweep"), af_region_async(c, data_start, mode, out);
    if (c->af_path == 3) {  // synchronous two-sweep schedule: index + record kernels
        note_schedule(c, "af_two_sweep_sync");
        int r = vcfxg_index(c, data_start, nullptr);
        return r ? r : vcfxg_allele_freq(c, mode, out);
    }
    // records of >= 512 B on average (a GT-dense VCF): the walk schedule, no index sweep; the
    // GT-first walk for "GT:..." records (VCFXG_AF_GF_WALK=0: the index sweep + per-line sweep)
    if (walk_wanted(c, true))
        return note_schedule(c, "af_walk"), af_region_walk(c, data_start, mode, out);
    static const bool gf_ok = [] {
        const char *e = getenv("VCFXG_AF_GF_WALK");
        return !(e && e[0] == '0');
    }();
    if (gf_ok && c->hint_gt_first && walk_wanted(c, false))
        return note_schedule(c, "af_walk_gt_first"), af_region_walk(c, data_start, mode, out, true);
    return note_schedule(c, "af_two_sweep"), af_region_async(c, data_start, mode, out);
}

static int af_rows(vcfxg_ctx *c, int mode, vcfxg_summary *out) {
    const uint64_t L = c->n_lines;
    const char *buf = P<char>(c->input);
    const uint64_t *nl_dev = P<uint64_t>(c->d_nlines);
    int r;
    prof_begin(c, "af_rows");
    HIPCHK(c, vcfxg::launch_af_rowlen(P<uint32_t>(c->rowpre), P<uint8_t>(c->status), nl_dev, L, P<uint64_t>(c->rowlen),
                                      c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->rowlen) + L, 0, 8, c->stream));
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)L + 1);
    if (r) return r;
    prof_end(c, "af_rows");
    static thread_local uint64_t host_tail[5];
    HIPCHK(c, hipMemcpyAsync(&host_tail[0], P<uint64_t>(c->rowoff) + L, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&host_tail[1], c->counters.p, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t text = host_tail[0];
    r = ensure(c, c->text, text + 1);
    if (r) return r;
    prof_begin(c, "af_format");
    HIPCHK(c, vcfxg::launch_af_format(buf, (int64_t)c->data_start, P<uint64_t>(c->line_end), nl_dev, L, mode,
                                      P<int32_t>(c->alt), P<int32_t>(c->tot), P<uint32_t>(c->rowpre),
                                      P<uint8_t>(c->status), P<uint64_t>(c->rowoff), P<char>(c->text), c->stream));
    prof_end(c, "af_format");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = text;
    if (out) {
        out->n_lines = L;
        out->rows = host_tail[1];
        out->data_lines = host_tail[2];
        out->warn_lines = host_tail[3];
        out->general_records = host_tail[4];
        out->text_bytes = text;
    }
    return VCFXG_OK;
}

}  // extern "C"
