// vcfxg_api_walk.hip -- what the record walks share on the host: the walkers' plan (chunk, count,
// line slots), the input-derived half of each entry point's walk / index choice, the buffer
// lists, and the two "walk, scan, compact into the dense per-line arrays" sequences (the AF walk
// with its reducers, the filter / query walk).  Each entry point keeps its own knobs.
#include "vcfxg_ctx.h"

// VCFXG_AF_DEPTH_LIVE=1 (A/B builds only): VCFXG_AF_DEPTH is read at every call instead of when
// the context opens, and 1 selects the batches of kAfDepthDefault whatever the input -- so ONE
// context, with one placement of the input in HBM, times every sweep (two contexts running the
// same kernel on the same bytes differed by 3 % here: as much as the sweeps differ)
#ifndef VCFXG_AF_DEPTH_LIVE
#define VCFXG_AF_DEPTH_LIVE 0
#endif

namespace vcfxg {

// walkers of the AF GT-only walk's (depth, roll) kernel resident on the device at a time: the
// blocks a CU holds x its CUs x the walkers of a block, queried once per context and instantiation
static int64_t walk_resident(const vcfxg_ctx *c, int depth, bool roll) {
    if (c->walk_resident_knob > 0) return c->walk_resident_knob;
    if (depth < 0 || depth > kAfDepthMax) return 0;
    int64_t &S = c->walk_resident[roll ? 1 : 0][depth];
    if (!S) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess) cus = 0;
        S = (int64_t)af_walk_resident_blocks(depth, roll) * cus * af_walk_waves_per_block();
        if (S <= 0) S = -1;  // (asked, unknown: the uniform layout)
    }
    return S > 0 ? S : 0;
}

// The AF GT-only walk's default layout: a main chunk of 256 KiB (where VCFXG_WALK_CHUNK does not
// set one), fitted to whole generations of the resident walkers, the last generation's bytes in
// half-size walkers -- where the region is at least one generation of that main chunk; a smaller
// region keeps the uniform walk_chunk.  A function of the region and the resident walkers alone.
// Measured on the 427,409 x 2,504 shard (profiles/af_layout_sweep.json, in one context per process):
// 3-6 % under the uniform 128 KiB chunks in every process; fit alone at 128 KiB: nothing.
static constexpr int64_t kAfMainChunk = 256 << 10;
static constexpr WalkLayoutKnob kDefaultLayout = {kLayoutTaper, 2, 1};

WalkPlan walk_plan(const vcfxg_ctx *c, size_t data_start, int64_t chunk, bool af_gt_only) {
    WalkPlan p;
    p.lo = (int64_t)data_start;
    p.hi = (int64_t)c->n;
    int64_t C0 = chunk ? chunk : c->walk_chunk;
    int knob = c->af_depth_knob;
    WalkLayoutKnob lk = c->walk_layout_knob;
#if VCFXG_AF_DEPTH_LIVE
    knob = getenv("VCFXG_AF_DEPTH") ? atoi(getenv("VCFXG_AF_DEPTH")) : 0;
    lk = parse_walk_layout(getenv("VCFXG_WALK_LAYOUT"));
    if (!chunk && getenv("VCFXG_WALK_CHUNK"))
        C0 = std::min<int64_t>(std::max<int64_t>(atol(getenv("VCFXG_WALK_CHUNK")), 4096), 8 << 20);
#endif
    af_sweep_plan(c->hint_span, knob, p.af_depth, p.af_roll);
    if (!af_gt_only) lk = WalkLayoutKnob{kLayoutUniform, 1, 0};
    if (lk.kind == kLayoutDefault) {
        const int64_t main = chunk || getenv("VCFXG_WALK_CHUNK") ? C0 : std::max(C0, kAfMainChunk);
        const int64_t S = walk_resident(c, p.af_depth, p.af_roll);
        if (S > 0 && (p.hi - p.lo + main - 1) / main >= S) {
            lk = kDefaultLayout;
            C0 = main;
        } else {
            lk = WalkLayoutKnob{kLayoutUniform, 1, 0};
        }
    }
    p.resident = lk.kind == kLayoutFit || lk.kind == kLayoutTaper ? walk_resident(c, p.af_depth, p.af_roll) : 0;
    p.lay_kind = lk;
    p.lay = walk_layout_plan(p.lo, p.hi, C0, p.resident, lk, af_walk_waves_per_block(), VCFXG_WALK_XCD != 0,
                             &p.lay_kind.kind);
    p.C = p.lay.C;
    p.nw = p.lay.nw;
    // a walker's line slots: twice the lines its chunk holds at the hinted mean length
    p.cap_w = (uint64_t)(2 * p.C / std::max<int64_t>(c->hint_line, 64)) + 16;
    p.cap = (uint64_t)p.nw * p.cap_w;
    // k_af_walk packs a walker's GT-line counts as wgt = ngt | ngf << 16: short records in a large
    // VCFXG_WALK_CHUNK, or a forced walk on them, do not fit.  The AF walk, the dosage / phaser walk
    // index and the LD walk then take their index paths, as after a walk that ran out of line
    // slots.  (The HWE walk launches k_af_walk too but never reads the packed count -- it zeroes
    // `counters` after the compaction -- and the fq, md and ib walks pack none: no check there.)
    p.fits_gt16 = p.cap_w <= 0xFFFF;
    return p;
}

// The AF GT-only walk's sweep for records of `span` sample bytes (the hinted 4 * samples - 1; up
// to 15 more before the sample start in the sweep's first 16 B block): kMeasuredDepth[wave-steps
// of the record], the depth whose rolling, non-temporal sweep an A/B on that record size showed
// faster than the batches of kAfDepthDefault (0: none, those batches -- today's kernel bit for
// bit).  Measured so far: 10 wave-steps, the 2,504-sample shard, where depth 10 (the
// whole record in one batch, 4 waves per SIMD) ran 8-10 % under the default in one context, 1-2 %
// under the rolling depths 6 and 12 and 3 % under 8.  Records of other sizes, and those longer
// than kAfDepthMax steps, keep the default until they are measured.
static constexpr int kMeasuredDepth[kAfDepthMax + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 10, 0, 0};
void af_sweep_plan(int64_t span, int knob, int &depth, bool &roll) {
    depth = kAfDepthDefault;
    roll = false;
#if VCFXG_AF_DEPTH_LIVE
    if (knob == 1) return;
#endif
    if (af_depth_compiled(knob)) {
        depth = knob;
        roll = true;
        return;
    }
    if (span <= 0) return;
    const int64_t steps = (span + 15 + kAfWaveStep - 1) / kAfWaveStep;
    if (steps <= kAfDepthMax && af_depth_compiled(kMeasuredDepth[steps])) {
        depth = kMeasuredDepth[steps];
        roll = true;
    }
}

bool walk_wanted(const vcfxg_ctx *c, bool need_gt_only) {
    return c->hint_line >= 512 && (!need_gt_only || c->hint_gt_only) && !c->walk_overflowed;
}

bool af_knob_allows_walk(const vcfxg_ctx *c) { return c->af_path != 3 && c->af_path != 8; }

int status_buffer(vcfxg_ctx *c, uint64_t L, StatusOwner owner) {
    claim_status(c, owner);
    return ensure(c, c->status, L + 1);
}

int af_buffers(vcfxg_ctx *c, uint64_t L, StatusOwner owner) {
    int r = ensure(c, c->alt, 4 * (L + 1));
    if (!r) r = ensure(c, c->tot, 4 * (L + 1));
    if (!r) r = ensure(c, c->rowpre, 4 * (L + 1));
    if (!r) r = status_buffer(c, L, owner);
    if (!r) r = ensure(c, c->rowlen, 8 * (L + 1));
    if (!r) r = ensure(c, c->rowoff, 8 * (L + 1));
    return r;
}

// the mapped host words the tail kernels write the call summaries into (AF walk [0..7],
// filter / query walk [8..17])
int ensure_sum_host(vcfxg_ctx *c) {
    if (c->sum_host) return VCFXG_OK;
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&c->sum_host), 256, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(c->sum_host, 0, 256);
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&c->sum_dev), c->sum_host, 0));
    return VCFXG_OK;
}

// k_af_walk's per-walker regions (line ends, counts, row prefixes, statuses, meta) and counts
int walk_buffers(vcfxg_ctx *c, const WalkPlan &p) {
    int r = ensure(c, c->wk_le, 8 * p.cap);
    if (!r) r = ensure(c, c->wk_alt, 4 * p.cap);
    if (!r) r = ensure(c, c->wk_tot, 4 * p.cap);
    if (!r) r = ensure(c, c->wk_rowpre, 4 * p.cap);
    if (!r) r = ensure(c, c->wk_status, p.cap);
    if (!r) r = ensure(c, c->wk_meta, af_meta_bytes() * p.cap);
    if (!r) r = ensure(c, c->wk_count, 8 * (size_t)(p.nw + 1));
    if (!r) r = ensure(c, c->wk_offs, 8 * (size_t)(p.nw + 1));
    if (!r) r = ensure(c, c->wk_gt, 4 * (size_t)p.nw);
    return r;
}

// the dense per-line arrays the regions are compacted into, for up to L lines
int dense_buffers(vcfxg_ctx *c, uint64_t L) {
    int r = ensure(c, c->line_end, 8 * (L + 1));
    if (!r) r = af_buffers(c, L, StatusOwner::other);
    if (!r) r = ensure(c, c->af_meta, af_meta_bytes() * (L + 1));
    return r;
}

// k_walk_compact: the walkers' regions (at wk_offs, the scan of their line counts) into the dense
// arrays; aux: wk_aux -> hwe_aux as well; bpre: the walker-scan's block prefixes (ensure_dense)
int walk_compact(vcfxg_ctx *c, int64_t nw, uint64_t cap_w, unsigned long long *counters, bool aux,
                 const uint64_t *bpre) {
    HIPCHK(c, launch_walk_compact(nw, cap_w, P<uint64_t>(c->wk_offs), P<uint32_t>(c->wk_gt), P<uint64_t>(c->wk_le),
                                  P<int32_t>(c->wk_alt), P<int32_t>(c->wk_tot), P<uint32_t>(c->wk_rowpre),
                                  P<uint8_t>(c->wk_status), c->wk_meta.p, P<uint64_t>(c->line_end), P<int32_t>(c->alt),
                                  P<int32_t>(c->tot), P<uint32_t>(c->rowpre), P<uint8_t>(c->status), c->af_meta.p,
                                  P<uint64_t>(c->d_nlines), counters, c->stream, aux ? P<int32_t>(c->wk_aux) : nullptr,
                                  aux ? P<int32_t>(c->hwe_aux) : nullptr, bpre));
    return VCFXG_OK;
}

// The AF walk with one of its reducers (aux: HWE's hom-alt counts; dose / head: the dosage walk
// and its head-only form), then the scan of the walkers' line counts and the compaction: the
// dense arrays hold the lines afterwards, d_nlines their count, counters[0..1] the compaction's
// GT-line counts.  The first small_zero bytes of wk_small are zeroed; its first word is the
// walk's overflow flag.  The walk is profiled as prof_name, the rest as "walk_compact".
int af_walk_to_dense(vcfxg_ctx *c, const WalkPlan &p, int mode, const char *prof_name, size_t small_zero, bool aux,
                     bool dose, bool head, bool cc) {
    int r = walk_buffers(c, p);
    if (!r && aux) r = ensure(c, c->wk_aux, 4 * p.cap);
    if (!r) r = ensure(c, c->wk_small, 128);
    if (!r) r = dense_buffers(c, p.cap);
    if (!r && aux) r = ensure(c, c->hwe_aux, 4 * (p.cap + 1));
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->wk_small.p, 0, small_zero, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->wk_count) + p.nw, 0, 8, c->stream));
    prof_begin(c, prof_name);
    if (cc)
        HIPCHK(c, launch_cc_walk(P<char>(c->input), p.lo, p.hi, p.lay, mode, c->hint_span, p.cap_w, P<uint64_t>(c->wk_le),
                                 P<int32_t>(c->wk_alt), P<int32_t>(c->wk_tot), P<uint32_t>(c->wk_rowpre),
                                 P<uint8_t>(c->wk_status), c->wk_meta.p, P<uint64_t>(c->wk_count), P<uint32_t>(c->wk_gt),
                                 P<unsigned>(c->wk_small), c->stream));
    else
        HIPCHK(c, launch_af_walk(P<char>(c->input), p.lo, p.hi, p.lay, mode, c->hint_span, p.cap_w, P<uint64_t>(c->wk_le),
                             P<int32_t>(c->wk_alt), P<int32_t>(c->wk_tot), P<uint32_t>(c->wk_rowpre),
                             P<uint8_t>(c->wk_status), c->wk_meta.p, P<uint64_t>(c->wk_count), P<uint32_t>(c->wk_gt),
                             P<unsigned>(c->wk_small), c->stream, aux ? P<int32_t>(c->wk_aux) : nullptr, nullptr, dose,
                             false, head, kAfDepthDefault, false));  // (the HWE / dosage walks: their own sweeps)
    prof_end(c, prof_name);
    prof_begin(c, "walk_compact");
    r = exclusive_scan(c, P<uint64_t>(c->wk_count), P<uint64_t>(c->wk_offs), (size_t)p.nw + 1);
    if (r) return r;
    r = walk_compact(c, p.nw, p.cap_w, P<unsigned long long>(c->counters), aux, nullptr);
    if (r) return r;
    prof_end(c, "walk_compact");
    return VCFXG_OK;
}

// The filter / query walk `what` (meta for every reducer but record_filter's, tab offsets for
// record_filter's) into line_end / status / af_meta / rf_tabs: k_fq_walk (profiled as walk_name),
// then, inside rest_name, which is left open for the caller's per-line kernels, the scan and
// k_fq_compact.  The overflow slot and the 8 counters of fq_small are zero on entry: k_fq_done
// (fq_walk_done) zeroed them after the last call, unless that call did not get that far
// (fq_small_dirty); k_fq_walk zeroes wk_count[nw], the scan's last entry.
int fq_walk_to_dense(vcfxg_ctx *c, const WalkPlan &p, int what, int strip_cr, const RfArgs &ra, const char *q_dev,
                     int qlen, int strict, int qa, int qb, const char *walk_name, const char *rest_name) {
    const bool tabs = what == kFqRF || what == kFqBoth, meta = what != kFqRF;
    const size_t mb = af_meta_bytes();
    int r = ensure(c, c->wk_le, 8 * p.cap);
    if (!r) r = ensure(c, c->wk_status, p.cap);
    if (!r && meta) r = ensure(c, c->wk_meta, mb * p.cap);
    if (!r && tabs) r = ensure(c, c->wk_tabs, 16 * p.cap);
    if (!r && tabs) r = ensure(c, c->rf_tabs, 16 * (p.cap + 1));
    if (!r) r = ensure(c, c->wk_count, 8 * (size_t)(p.nw + 1));
    if (!r) r = ensure(c, c->wk_offs, 8 * (size_t)(p.nw + 1));
    if (!r) r = ensure(c, c->fq_small, 128);
    if (!r) r = ensure(c, c->line_end, 8 * (p.cap + 1));
    if (!r) r = status_buffer(c, p.cap, StatusOwner::other);
    if (!r && meta) r = ensure(c, c->af_meta, mb * (p.cap + 1));
    if (!r) r = ensure_sum_host(c);
    if (r) return r;
    if (c->fq_small_dirty) HIPCHK(c, hipMemsetAsync(c->fq_small.p, 0, 128, c->stream));
    c->fq_small_dirty = true;  // until the call has synchronised
    prof_begin(c, walk_name);
    // (wk_tabs / rf_tabs may be null or stale without record_filter: its kernels alone read them)
    HIPCHK(c, launch_fq_walk(what, P<char>(c->input), p.lo, p.hi, p.C, strip_cr, c->hint_span, p.cap_w, ra,
                             q_dev, qlen, strict, qa, qb, P<uint64_t>(c->wk_le), P<uint8_t>(c->wk_status),
                             c->wk_meta.p, c->wk_tabs.p, P<uint64_t>(c->wk_count), P<unsigned>(c->fq_small), c->stream));
    prof_end(c, walk_name);
    prof_begin(c, rest_name);
    r = exclusive_scan(c, P<uint64_t>(c->wk_count), P<uint64_t>(c->wk_offs), (size_t)p.nw + 1);
    if (r) return r;
    HIPCHK(c, launch_fq_compact(what, p.nw, p.cap_w, P<uint64_t>(c->wk_offs), P<uint64_t>(c->wk_le),
                                P<uint8_t>(c->wk_status), c->wk_meta.p, c->wk_tabs.p, P<uint64_t>(c->line_end),
                                P<uint8_t>(c->status), c->af_meta.p, c->rf_tabs.p, P<uint64_t>(c->d_nlines), c->stream));
    return VCFXG_OK;
}

// k_fq_done and the call's ONE host synchronisation: counters[0..7], the line count and the
// overflow slot are in sum_host[8..17] afterwards, and fq_small is zero again
int fq_walk_done(vcfxg_ctx *c) {
    HIPCHK(c, launch_fq_done(P<unsigned long long>(c->fq_small) + 1, P<uint64_t>(c->d_nlines), P<uint64_t>(c->fq_small),
                             c->sum_dev + 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fq_small_dirty = false;
    return VCFXG_OK;
}

}  // namespace vcfxg
