// vcfxg_ctx.h -- the device context behind the C ABI (include/vcfx_gpu.h) and the host-side
// helpers its translation units (vcfxg_api*.hip, vcfxg_comm.hip) share.  Private: not installed,
// and nothing under include/ sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vcfx_gpu.h"
#include "vcfxg_env.h"
#include "vcfxg_kernels.h"
#include "vcfxg_rf.h"

// A device allocation that frees itself (non-copyable, movable).  alloc and release are the only places
// that call hipMalloc / hipFree for a buffer, and the only ones that change `live`, the capacities that
// the DevBufs of the process hold (vcfxg_device_bytes_live).
struct DevBuf {
    static inline std::atomic<uint64_t> live{0};
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {  // (what this held goes to o, and is freed with it)
        std::swap(p, o.p), std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { (void)release(); }
    hipError_t alloc(size_t bytes) {  // for an empty buffer, which stays empty when the device has none
        void *np = nullptr;
        const hipError_t e = hipMalloc(&np, bytes);
        if (e == hipSuccess) p = np, cap = bytes, live += bytes;
        return e;
    }
    hipError_t release() {  // empty afterwards, whatever hipFree says (the caller has waited for readers)
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        live -= cap;
        p = nullptr, cap = 0;
        return e;
    }
};

// Whose per-line statuses c->status holds.  Every call that writes the buffer claims it first
// (claim_status); a status fetch is served only to the owner.
enum class StatusOwner { none, other, dedup, sort, diff, merge, region, fasta, haplotype };
// "This call has run on the current index": the index generation (vcfxg_ctx::index_gen) it completed
// on; a new index outdates every tool's results at once (mark_done / is_done below; = {} withdraws).
struct Done { uint64_t gen = 0; };

// The stages the keyed line tools share (vcfxg_api_keyed.hip).  Every tool owns its instances, so
// its orders, counts and texts stay readable after another tool ran on the context; the per-line
// status buffer is the context's one, and holds the last writer's statuses only (StatusOwner).
// A stable radix sort of (64-bit key part, line) pairs, pass after pass: (ka, va) holds the pairs to
// sort, and after a pass the sorted ones; va is the order so far.
struct SortScratch {
    DevBuf k0, k1, v0, v1, tmp;
    size_t t_sort = 0;
    uint64_t *ka = nullptr, *kb = nullptr;
    uint32_t *va = nullptr, *vb = nullptr;
};
// n output lines as one text: per line its bytes, their scan (n + 1 offsets; on the host once a text
// call has fetched them) and its first source byte.
struct TextOrder {
    DevBuf len, off, src;
    std::vector<uint64_t> off_host;
    uint64_t n = 0;
};

struct vcfxg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // input
    DevBuf input;
    size_t n = 0;
    int last_byte = -1;  // input[n-1] (host copy), -1 if empty
    bool loaded = false;
    bool ingesting = false;               // between vcfxg_ingest_begin and the final chunk
    bool hints_pending = false;           // no ingested chunk has held a data line yet
    const char *last_schedule = "";       // the schedule of the last region call (note_schedule)
    std::vector<std::pair<size_t, hipEvent_t>> ingest_ev;  // (input bytes copied once it fires, event)
    std::vector<hipEvent_t> ingest_ev_free;
    // index
    DevBuf idx_counts, idx_offs, idx_pos, line_end, d_nlines, scan_tmp;
    size_t data_start = 0;
    uint64_t n_lines = 0;
    bool indexed = false;
    uint64_t index_gen = 1;  // bumped wherever a new index replaces the old one (new_index)
    // per-line results
    DevBuf alt, tot, rowpre, status, rowlen, rowoff, text, counters, query, crit, pool;
    StatusOwner status_owner = StatusOwner::none;
    std::string query_host, crit_host, pool_host;  // host sources of in-flight async copies
    // LD
    DevBuf ld_G, ld_lines, ld_vidx, ld_valid, ld_Gc, ld_vars, ld_plen, ld_poff, ld_prefix, ld_cid, ld_blocks, ld_cnt,
        ld_off, ld_pairs, ld_fast, ld_gflag, ld_Gp, ld_rowoff, ld_Gv, ld_Gq, dose_meta;
    // LD walk (vcfxg_ld_prepare_region): walker counts, valid-line counts and their scan, flags +
    // summary; ld_gc_ready: ld_Gc holds the compact int8 rows (the walk gathers them only when
    // some variant misses a call)
    DevBuf ld_wcnt, ld_wval, ld_vbase, ld_small, ld_pend;
    // vcfxg_bgzf_stage: the compressed stream's size and the bytes staged so far (into bgz_in, on
    // copy_stream); vcfxg_bgzf_inflate: members already launched and their output bytes
    size_t bgz_total = 0, bgz_staged = 0;
    uint64_t bgz_handed = 0;  // members of the last BGZF ingest the lane decoder handed over
    uint64_t bgz_launched = 0, bgz_out = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t bgz_copy_ev = nullptr;  // the latest staged copy
    // the inflate batches run round robin on their own streams (one stream would serialise each
    // batch's tail), joined before the device input completes; two: batches are 32,768 members
    // (hostio.cpp), and a fresh context pays ~7 ms to create a stream
    static constexpr int kBgzStreams = 2;
    hipStream_t bgz_stream[kBgzStreams] = {};
    hipEvent_t bgz_ev[kBgzStreams] = {};
    int bgz_next = 0;
    bool ld_gc_ready = false;
    bool ld_vq = false;  // ld_Gv / ld_Gq (valid-mask and squared-dosage FP4 planes) are current
    int n_cu = 0;
    DevBuf async_small;         // asynchronous AF path: line range {0, n}, failure flags, summary
    DevBuf ld_temp, ld_quarters, ld_stage_ctr;  // LD: pairs staged by the count pass
    uint64_t ld_temp_cap = 0;
    // test hook: a fixed (small) staging capacity exercises the overflow -> emit-pass path
    uint64_t ld_stage_cap_fixed = vcfxg::env_u64("VCFXG_LD_STAGE_CAP", 0);
    DevBuf af_meta;             // AF head pass output (k_af_meta)
    // walk AF path (vcfxg_af_walk.hip): per-walker regions, counts, scan, flags
    DevBuf wk_le, wk_alt, wk_tot, wk_rowpre, wk_status, wk_meta, wk_count, wk_offs, wk_gt, wk_small;
    DevBuf wk_tabs, rf_tabs;    // filter / query walk: per-line tab offsets (per walker, dense)
    // AF walk region tail: per walker row bytes, text offsets, first line start; leftover list
    DevBuf wk_text, wk_toff, wk_start, wk_cx, wk_bs, scratch_small, byte_cnt;
    // AF walk: flags / counters that k_walker_scan zeroes after reading them (af_small_dirty: a
    // call did not get that far, so the next one clears them first), and the call summary the
    // same kernel writes straight into mapped host memory (no copy before the synchronisation)
    DevBuf af_small;
    bool af_small_dirty = true;
    DevBuf wk_stage, wk_dirty;  // AF walk: each walker's rows as text (kStageCap bytes), its clean flag
    uint64_t *sum_host = nullptr, *sum_dev = nullptr;
    uint64_t cx_hint = ~0ull;  // leftover lines of the previous AF walk (sizes k_af_cx's grid)
    // filter / query walk: overflow slot + 8 counters, zeroed by k_fq_done after each call
    // (fq_small_dirty as af_small_dirty); its summary goes to sum_host[8..17]
    DevBuf fq_small;
    bool fq_small_dirty = true;
    uint64_t fq_lines_hint = 0;  // lines of the previous filter / query walk (sizes k_fq_finish's grid)
    // the bytes last uploaded to query / crit / pool and the buffer they went to: an unchanged
    // query or criteria list is not copied again (any other writer resets the pointer)
    std::string query_dev, crit_dev, pool_dev;
    void *query_dev_p = nullptr, *crit_dev_p = nullptr, *pool_dev_p = nullptr;
    // the last AF walk left its per-line results in walker regions only (ensure_dense)
    bool dense_pending = false;
    int64_t dense_nw = 0;
    uint64_t dense_cap_w = 0;
    // VCFX_hwe_tester: hom-alt counts (dense, per walker), the host-recheck list and its length
    DevBuf hwe_aux, wk_aux, hwe_rc;
    // VCFX_allele_counter: slots' sample indices, name offsets and bytes, per-wave sample tables
    DevBuf ac_eff, ac_noff, ac_names, ac_scratch, ac_etab, ac_nib;
    std::vector<uint32_t> ac_eff_host;
    std::vector<uint64_t> ac_noff_host;
    std::string ac_names_host;
    std::vector<uint8_t> ac_etab_host;
    // VCFX_haplotype_phaser: genotype rows (by line), per-line info, variant -> line, pair flags
    DevBuf ph_G, ph_isvar, ph_info, ph_vnum, ph_vline, ph_flags, ph_r2;
    uint64_t ph_nvar = 0;
    uint64_t hwe_rc_n = 0;
    // VCFX_inbreeding_calculator: one block's code rows, meta, table and walker counts; the
    // per-sample state carried from block to block (sumExp, obsHet, usedCount, carried code)
    DevBuf ib_codes, ib_meta, ib_tab, ib_packed, ib_cnt, ib_offs, ib_sum, ib_obs, ib_used, ib_carried, ib_small;
    uint32_t ib_ns = 0;  // samples of the last vcfxg_inbreeding_region call (0: none yet)
    // VCFX_sample_extractor: the kept-field bitmask; lines per call (read when the context opens;
    // tests make many blocks, and blocks of one line, with small values)
    DevBuf sx_mask;
    std::vector<uint32_t> sx_mask_host;
    uint64_t sx_block = vcfxg::env_u64("VCFXG_SX_BLOCK", 65536, 1, 1u << 24);
    // VCFX_cross_sample_concordance: column multiplicities, data-line flags and their scan, the
    // "#CHROM" line list, the summary words; the last call's totals
    DevBuf cc_mult, cc_isdata, cc_ord, cc_chrom, cc_small;
    uint64_t cc_totals[4] = {0, 0, 0, 0};
    // VCFX_duplicate_remover: per line the five tab offsets, POS and hash, the wave pass's line
    // list, the data flags and their scan; the sort of the (hash, line) pairs (its temporary storage
    // also serves the max scan); run heads and their scan, pending flags; the last call's counts per
    // status and its wave-path lines
    DevBuf dd_tabs, dd_pos, dd_hash, dd_queue, dd_isdata, dd_ord, dd_hp, dd_head, dd_left;
    SortScratch dd_sort;
    uint64_t dd_counts[6] = {0, 0, 0, 0, 0, 0};
    Done dd_done;  // vcfxg_dedup has run on this index (its statuses: while status_owner says so)
    // VCFX_sorter: per line POS, aux (chromToId or CHROM's length) and CHROM's first word, the wave
    // pass's line list, the written flags and their scan; the sort of the (key, line) pairs
    // (srt_sort.va: the order); the output lines (srt_out.n of them); the last call's counts per
    // status and its wave-path lines; text bytes
    // per vcfxg_sort_text call (read when the context opens; tests cut between every pair of lines
    // with 64); VCFXG_SRT_NT: bit 0 non-temporal loads, bit 1 non-temporal stores in the gather (both
    // by default: measured 5 to 12 % faster than neither on the bench shard, DESIGN.md "Sorting")
    DevBuf srt_pos, srt_aux, srt_w0, srt_queue, srt_written, srt_ord;
    SortScratch srt_sort;
    TextOrder srt_out;
    uint64_t srt_counts[6] = {0, 0, 0, 0, 0, 0};
    Done srt_done;
    uint64_t srt_block = vcfxg::env_u64("VCFXG_SRT_BLOCK", 256ull << 20, 1, 1ull << 36);
    int srt_nt = (int)vcfxg::env_i64("VCFXG_SRT_NT", 3) & 3;
    // VCFX_diff_tool: per line the five tab offsets, the key's length and its scan, ALT's token count,
    // POS and CHROM's natural-order parts, the key's hash, the data flags and their scan, the wave
    // passes' line list; the key text; the data lines in line order; the sort of the (hash, line)
    // pairs (its temporary storage also serves the max scan), run heads and their scan, each
    // element's class, each class's first file-2 element, pending flags; the walk's two pointers; the
    // unique flags and their scan; the unique lines' key texts as output lines (df_out.n of them, file
    // 1's first: df_nu1); the summary words; the last call's counts; text bytes per vcfxg_diff_text
    // call and steps per launch of the serial walk (read when the context opens; tests use 64 and 7)
    DevBuf df_tabs, df_klen, df_koff, df_ntok, df_posv, df_natv, df_nsuf, df_hash, df_isdata, df_ord, df_queue, df_ktext,
        df_line, df_hp, df_head, df_rep, df_first2, df_left, df_state, df_uflag, df_uord, df_sum;
    SortScratch df_sort;
    TextOrder df_out;
    uint64_t df_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t df_nu1 = 0;
    Done df_done;
    uint64_t df_block = vcfxg::env_u64("VCFXG_DF_BLOCK", 256ull << 20, 1, 1ull << 36);
    uint64_t df_walk_steps = vcfxg::env_u64("VCFXG_DF_WALK_STEPS", 1ull << 20, 1, 1ull << 24);
    // VCFX_merger: per line its file, POS and the key string's descriptor (first word, start, length;
    // with -n the prefix word and the digit run's value), the wave pass's line list, the written
    // flags and their scan; per file (K + 1 words each) its first byte, first line, first '#' line,
    // first other line, BAD lines, walk cursor and end; the sort of the (key part, line) pairs
    // (mg_sort.va: the order; first the written lines in line order, which the walk reads to write
    // vb); the output lines (mg_out.n of them); the walk's output count; the last call's counts and
    // files; steps per launch of the walk (read when the
    // context opens; tests use 7).  The text blocks are bounded by srt_block (VCFXG_SRT_BLOCK).
    DevBuf mg_file, mg_pos, mg_w0, mg_ks, mg_kl, mg_pn, mg_num, mg_queue, mg_written, mg_ord, mg_fmeta, mg_state;
    SortScratch mg_sort;
    TextOrder mg_out;
    uint64_t mg_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t mg_files = 0;
    Done mg_done;
    uint64_t mg_walk_steps = vcfxg::env_u64("VCFXG_MG_WALK_STEPS", 1ull << 20, 1, 1ull << 24);
    // VCFX_region_subsampler: the table of the last vcfxg_regions_load (it outlives loads and indexes of
    // the input): its descriptor (RsTableArgs), the names' bytes and offsets, the dictionary, the uploaded intervals (ids, starts,
    // ends: 3 n words), their sort, the sorted ids and starts, the scan keys and tile maxima, the reach,
    // per name its range, the open flags and their scan, the merged rows (rs_nm of them); the class
    // pass's wave list; the last filter's counts per status and its wave-path lines
    DevBuf rs_tab, rs_names, rs_noff, rs_dict, rs_in, rs_sid, rs_start, rs_key, rs_tile, rs_reach, rs_first, rs_last, rs_open,
        rs_ord, rs_mid, rs_mstart, rs_mend, rs_queue;
    SortScratch rs_sort;
    uint64_t rs_n = 0, rs_nm = 0;
    uint32_t rs_nchrom = 0;
    uint64_t rs_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool rs_loaded = false;  // a table is resident
    Done rs_done;            // vcfxg_region_filter has run on this index (with this table)
    // VCFX_haplotype_extractor: per line POS, member flag and its scan, CHROM's length, the fixed-stride region's
    // offset, the matrix-row flag and its scan, member / block / flip;
    // the cell matrix (lines x samples); member -> line, block-start flags and their scan, flips; per block
    // first and last member, START, END, head bytes, row length and its scan; per (tile, sample) the tile
    // sums and carries, per tile its start flag; per (block, sample) the run's offset in the row; the last
    // scan's parameters and counts
    DevBuf hx_pos, hx_flag, hx_mnum, hx_clen, hx_fixed, hx_general, hx_gnum, hx_lmember, hx_lblock, hx_lflip, hx_cells, hx_mline, hx_start, hx_bnum, hx_flip,
        hx_first, hx_last, hx_bstart, hx_bend, hx_head, hx_rowlen, hx_rowoff, hx_agg, hx_carry, hx_tstart, hx_base;
    uint64_t hx_nm = 0, hx_nb = 0, hx_text = 0;
    uint32_t hx_ns = 0;
    Done hx_scanned, hx_laid;
    // VCFX_field_extractor: the table of the last vcfxg_fields_load (it outlives loads and indexes of the
    // input) and its counts; per line the status, the row flag and its scan, the row bytes and their scan, the cell
    // matrix (lines x columns), the requested sample columns' spans and the sub-fields' FORMAT indices (the
    // cell pass's scratch); the last scan's rows and text bytes
    DevBuf fx_tab, fx_out, fx_status, fx_isrow, fx_rownum, fx_rowlen, fx_rowoff, fx_cells, fx_span, fx_sub;
    std::vector<uint32_t> fx_tab_host;
    vcfxg::FxOut fx_out_host = {};  // host sources / destinations of the scan's asynchronous copies
    uint64_t fx_tail[2] = {0, 0};
    uint32_t fx_ncols = 0, fx_nsc = 0, fx_nsub = 0;
    uint64_t fx_rows = 0, fx_text = 0;
    bool fx_loaded = false;   // a table is resident
    Done fx_scanned;          // the statuses and the matrix are the last vcfxg_fields_scan's (of this index and table)
    // VCFX_multiallelic_splitter: the table; per line of the block its tab offsets, cost and the
    // scans of nAlts and cost; each line's text offset; {lines taken, rows}; the last call's block;
    // lines and text bytes per call (read when the context opens; tests make blocks of one line)
    DevBuf ms_tab, ms_geom, ms_cost, ms_costoff, ms_rowbase, ms_lineoff, ms_small;
    std::vector<uint32_t> ms_tab_host;
    uint64_t ms_l0 = 0, ms_n = 0;
    Done ms_done;
    uint64_t ms_block = vcfxg::env_u64("VCFXG_MS_BLOCK", 65536, 1, 1u << 24);
    // VCFX_fasta_converter: per line of the block its column flag, column number and FaMeta; the
    // block's base matrix; the rows' text offsets and skipped columns; the last scan's block; the
    // text is sized by vcfxg_fasta_begin; lines per call (read when the context opens; tests end
    // blocks in the middle of a FASTA line with 1 and 7)
    DevBuf fa_flag, fa_col, fa_meta, fa_M, fa_rowoff, fa_skip;
    uint64_t fa_l0 = 0, fa_n = 0, fa_cols = 0, fa_text = 0;
    Done fa_scanned, fa_begun;
    uint64_t fa_block = vcfxg::env_u64("VCFXG_FA_BLOCK", 65536, 1, 1u << 24);
    uint64_t ms_bytes = vcfxg::env_u64("VCFXG_MS_BYTES", 512ull << 20, 1);
    // records per chain block (read when the context opens; tests cross block edges with 1, 7, 64)
    uint64_t ib_block = vcfxg::env_u64("VCFXG_IB_BLOCK", 65536, 1, 1u << 24);
    // ulps either side of the device p-value that must print the same digits (test hook: a
    // huge value sends every exp()-derived row to the host).  How near the p-values come to a
    // value where the six-digit text changes, with the C library's exp (a CPU search over whole
    // count spaces, tests/_exact_num.py hwe_nearest_boundary): the smallest distance is 4,334 ulps
    // over every triple with N <= 100 (file mode, (2, 9, 5)); at N = 97 / 301 / 2504 it is
    // 10,520,075 / 1,906,818 / 134,905 ulps in file mode and 8,177,671 / 7,635,856 / 263,560 on
    // stdin.  tests/test_gpu_count_edges.py runs those triples: the device left none to the host.
    int64_t hwe_ulps = vcfxg::env_i64("VCFXG_HWE_ULPS", 16);
    // (an override is clamped to [4 KiB, 8 MiB]: the AF walk packs a walker's GT-line count in
    // 16 bits, and its line capacity 2 * chunk / hint_line + 16 stays below 2^15 for the
    // >= 512 B records the walk takes)
    int64_t walk_chunk = vcfxg::env_i64("VCFXG_WALK_CHUNK", 128 * 1024, 4096, 8 << 20);
    const bool walk_chunk_forced = vcfxg::env_set("VCFXG_WALK_CHUNK");  // the hints leave it alone
    bool walk_overflowed = false;  // the last walk run overflowed: two-sweep schedule
    bool dose_head_failed = false;  // a dosage head walk's rows failed the check (this input)
    bool ph_head_failed = false;    // a phaser head-walk index failed the parse's check (this input)
    // host hints taken at load time from the first data line: its '\n' distance from the
    // sample start (the walk's first prediction) and the mean length of the first lines
    int64_t hint_span = 0, hint_line = 0;
    // the first data line's FORMAT is exactly "GT" (fixed-stride records: the walk's predicted
    // ends pay; "GT:AD:DP"-like records are scanned faster by the index sweep)
    bool hint_gt_only = false;
    // ... or starts with "GT:" (GT:AD:DP-like records: the GT-first walk, gt_first finding each
    // record's end in its one sweep)
    bool hint_gt_first = false;
    uint64_t af_line_cap = 0;   // two-sweep AF: line capacity the last run needed
    // region AF schedule: 0 = default (the walk schedule 7 when the first records average
    // >= 512 B, else 3), 3 = single-sweep index + head pass + fixed-stride sweep, with one host
    // synchronisation; 7 = walk (k_af_walk: predicted record ends validated by the sweep, one HBM
    // pass); 8 = the two-sweep schedule always
    int af_path = (int)vcfxg::env_i64("VCFXG_AF_FUSED", 0);
    // the AF GT-only walk's sweep depth in wave-steps: 0 = the plan's choice (walk_plan), 6 / 8 /
    // 10 / 12 = that depth, rolling past it (tests, A/B); any other value is the plan's choice
    int af_depth_knob = (int)vcfxg::env_i64("VCFXG_AF_DEPTH", 0);
    int last_af_depth = 0;        // the depth / rolling of the last AF GT-only walk launched
    bool last_af_roll = false;    // (vcfxg_last_af_depth; 0: none yet)
    // the AF GT-only walk's chunk layout (walk_plan): VCFXG_WALK_LAYOUT = uniform | fit |
    // taper:<div>:<g> | split:<div>:<K1> (a test's explicit first short round), read when the context
    // opens; unset or anything else: the plan's default
    vcfxg::WalkLayoutKnob walk_layout_knob = vcfxg::parse_walk_layout(vcfxg::env_text("VCFXG_WALK_LAYOUT"));
    // the walkers resident at a time, per compiled (depth, roll) of the AF GT-only walk (queried once
    // each; 0: not yet); VCFXG_WALK_RESIDENT overrides the query (tests: a small device's layouts on
    // small inputs)
    mutable int64_t walk_resident[2][vcfxg::kAfDepthMax + 1] = {};
    int64_t walk_resident_knob = vcfxg::env_i64("VCFXG_WALK_RESIDENT", 0);
    vcfxg::WalkLayoutKnob last_walk_layout_kind;  // of the last AF GT-only walk launched
    vcfxg::WalkLayout last_walk_layout = {};      // (vcfxg_last_walk_layout)
    int64_t last_walk_resident = 0;
    // record_filter / genotype_query region schedule: 0 = the walk (vcfxg_fq_walk.hip) when
    // the first records average >= 512 B, 1 = the walk always, -1 = index + per-tool kernels
    int fq_path = (int)vcfxg::env_i64("VCFXG_FQ_WALK", 0);
    std::vector<uint8_t> ld_gflag_host;  // per 128-variant group: all complete
    uint64_t ld_m = 0, ld_prefix_bytes = 0, ld_np = 0;
    int ld_kpad = 64, ld_ns = 0, ld_kp4 = 64;
    bool ld_chrom_ids = false;
    std::vector<uint32_t> ld_cid_host, ld_blocks_host;
    // the last streaming call's block lists: key (j0, j1, window, M, masked kernel), group
    // flags, list sizes (fast, masked, int8), the ld_blocks buffer they were copied to
    uint64_t ld_plan_key[5] = {0, 0, 0, 0, 0};
    std::vector<uint8_t> ld_plan_gf;
    uint32_t ld_plan_n[4] = {0, 0, 0, 0};
    // the sparse-missing LD kernel's data (ld_sp: some 256-group qualifies): CSR of each
    // variant's missing samples and the sample-major contribution plane
    bool ld_sp = false;
    uint64_t ld_mp = 0;
    DevBuf ld_moff, ld_midx, ld_mvar, ld_gt16, ld_sprec, ld_midx16;
    // device BGZF inflate (vcfxg_ingest_bgzf): compressed bytes, member table, output offsets,
    // per-member status, first bad member
    DevBuf bgz_in, bgz_mem, bgz_off, bgz_stat, bgz_small, bgz_perm;
    // the lane decoder's token buffers (and hand-over lists): one per inflate stream and one for
    // `stream`; its side stream (the hand-overs') and events
    DevBuf bgz_tok[kBgzStreams + 1];
    vcfxg::InflateSide bgz_side;
    void *ld_plan_dev = nullptr;
    uint64_t text_bytes = 0;
    uint64_t text_hint = 0;  // AF walk: text bytes of the previous call (the next call's capacity)
    // profiling: an event pair per launch from a pool, harvested only when the figures are
    // read (or the pending list is long): no event queries between the calls of a timed loop
    bool profiling = false;
    std::string prof_only;  // non-empty: only this kernel is timed
    struct ProfRec {
        const char *name;
        hipEvent_t a, b;
    };
    std::vector<hipEvent_t> ev_free;
    std::vector<ProfRec> ev_open, pending;
    std::map<std::string, float> ms;           // last launch
    std::map<std::string, std::pair<double, uint64_t>> acc;  // sum ms, launches
};

namespace vcfxg {

constexpr size_t kPad = 256;  // zeroed bytes after the input: 16 B loads may run past n

// a new index (vcfxg_index's, or a region call's own): pending walker regions and every tool's results go
inline void new_index(vcfxg_ctx *c) {
    c->dense_pending = false;
    c->index_gen++;
}
inline void mark_done(vcfxg_ctx *c, Done &d) { d.gen = c->index_gen; }
inline bool is_done(const vcfxg_ctx *c, const Done &d) { return d.gen == c->index_gen; }
// before a call's first launch that writes c->status
inline void claim_status(vcfxg_ctx *c, StatusOwner owner) { c->status_owner = owner; }

// ---- vcfxg_api.hip
int fail(vcfxg_ctx *c, hipError_t e, const char *what);
#define HIPCHK(ctx, x)                                          \
    do {                                                        \
        hipError_t e_ = (x);                                    \
        if (e_ != hipSuccess) return vcfxg::fail(ctx, e_, #x);  \
    } while (0)
int ensure(vcfxg_ctx *c, DevBuf &b, size_t bytes);  // (b holds `bytes` at least; its old bytes are not kept)
// b replaced by a fresh buffer of `bytes` that holds its first `keep` (the stream drained before the free)
int regrow(vcfxg_ctx *c, DevBuf &b, size_t bytes, size_t keep);
template <typename T>
T *P(DevBuf &b) {
    return reinterpret_cast<T *>(b.p);
}
// an event pair per profiled launch; prof_collect after a call harvests a long pending list
void prof_begin(vcfxg_ctx *c, const char *name);
void prof_end(vcfxg_ctx *c, const char *name);
void prof_collect(vcfxg_ctx *c);
// exclusive prefix sums of n values on the context's stream (hipcub, temporary in scan_tmp)
int exclusive_scan(vcfxg_ctx *c, const uint32_t *in, uint64_t *out, size_t n);
int exclusive_scan(vcfxg_ctx *c, const uint64_t *in, uint64_t *out, size_t n);
void note_schedule(vcfxg_ctx *c, const char *what);
bool load_hints(vcfxg_ctx *c, const char *h, size_t n);

// ---- vcfxg_api_keyed.hip: the stages the keyed line tools share
// the bits of x: the sort's end bit for a key part whose largest value is x
int bit_width(uint64_t x);
// n pairs: the buffers sized, (ka, va) = (k0, v0), the caller's to fill
int sort_begin(vcfxg_ctx *c, SortScratch &S, uint64_t n);
// one stable pass over the bits [0, end_bit) of the keys at ka: sorted pairs at (ka, va) afterwards
int sort_pass(vcfxg_ctx *c, SortScratch &S, uint64_t n, int end_bit);
// the passes over a key string of at most `longest` bytes, its 8-byte words from the last to the
// first: fill(w, shift) writes every pair's word w, shifted right by `shift` bits, to S.ka in the
// order S.va (0: no error)
template <class Fill>
int sort_string_words(vcfxg_ctx *c, SortScratch &S, uint64_t n, uint64_t longest, Fill fill) {
    const uint64_t W = (longest + 7) / 8;
    for (uint64_t w = W; w-- > 0;) {
        // the last word's low bytes are zero padding in every key string: shifted out, so the sort's
        // bit range starts at 0 (the library's merge path, which takes 1 K to 1 M items, builds its
        // mask with a shift by begin + bits, undefined when that is 64)
        const uint32_t shift = w == W - 1 && longest % 8 ? (uint32_t)(8 * (8 - longest % 8)) : 0;
        int r = fill(w, shift);
        if (!r) r = sort_pass(c, S, n, 64 - (int)shift);
        if (r) return r;
    }
    return VCFXG_OK;
}
// n output lines: T's buffers sized (place_begin; the diff tool then fills len and src itself), and
// for the indexed lines order[0 .. n) their lengths, source bytes and the scan that places them
int place_begin(vcfxg_ctx *c, TextOrder &T, uint64_t n);
int place_lines(vcfxg_ctx *c, TextOrder &T, const uint64_t *line_end, int64_t data_start, const uint32_t *order, uint64_t n);
// Output lines [first, first + taken) of T, first < hi <= T.n: as many as fit `block` bytes and end
// before line hi, one at least (the offsets are read back once; the cut is a search in them),
// gathered from src_text into the context's text under the profile region `region`.
int text_block(vcfxg_ctx *c, TextOrder &T, const char *src_text, uint64_t first, uint64_t hi, uint64_t block,
               const char *region, uint64_t *taken, uint64_t *bytes);
// the statuses of lines [first, first + count) of the index / entries [first, first + count) of an
// order of n lines, to the host (done: the tool's call has run on this index; owner: the statuses
// are served only while c->status is still that tool's, VCFXG_E_STATE otherwise)
int fetch_status(vcfxg_ctx *c, StatusOwner owner, const Done &done, uint64_t first, uint64_t count, uint8_t *status);
int fetch_order(vcfxg_ctx *c, const Done &done, const uint32_t *order, uint64_t n, uint64_t first, uint64_t count, uint32_t *lines);

// ---- vcfxg_api_af.hip
int ensure_dense(vcfxg_ctx *c);
// per-line calls on the indexed context read the dense arrays
#define DENSE(c)                          \
    do {                                  \
        int rd_ = vcfxg::ensure_dense(c); \
        if (rd_) return rd_;              \
    } while (0)

// ---- vcfxg_api_walk.hip: the record walks' plan, schedule predicates and shared sequences
// c->status sized for L lines and claimed for `owner`; af_buffers: the other per-line buffers with it
int status_buffer(vcfxg_ctx *c, uint64_t L, StatusOwner owner);
int af_buffers(vcfxg_ctx *c, uint64_t L, StatusOwner owner);
int ensure_sum_host(vcfxg_ctx *c);
// the walkers of [data_start, n): chunk C (0: the context's walk_chunk), nw walkers of cap_w line
// slots each, cap slots in all; fits_gt16: cap_w fits the 16-bit GT-line count k_af_walk packs
// af_depth / af_roll: the AF GT-only walk's sweep (launch_af_walk depth / roll), from the hinted
// sample span: a rolling non-temporal sweep of the depth that the A/B of that record size showed
// faster, else the batches of kAfDepthDefault; VCFXG_AF_DEPTH forces a compiled depth
// lay: the walkers' bytes (vcfxg_walk_layout.h): uniform chunks of C for every walk but the AF
// GT-only one (af_gt_only), whose layout the plan chooses from the region's size and the walkers
// resident at a time (VCFXG_WALK_LAYOUT forces one); C is then the larger chunk, nw = lay.nw
struct WalkPlan {
    int64_t lo, hi, C, nw;
    uint64_t cap_w, cap;
    bool fits_gt16;
    int af_depth;
    bool af_roll;
    WalkLayout lay;
    WalkLayoutKnob lay_kind;  // what the layout came to (kind; taper / split: div and g / K1 as asked)
    int64_t resident;         // the resident walkers it was planned for (0: not asked)
};
WalkPlan walk_plan(const vcfxg_ctx *c, size_t data_start, int64_t chunk = 0, bool af_gt_only = false);
void af_sweep_plan(int64_t span, int knob, int &depth, bool &roll);
// the input-derived half of "does this call walk": long records (of FORMAT exactly "GT" where the
// walk's kernel needs that) and no walk overflow on this input yet
bool walk_wanted(const vcfxg_ctx *c, bool need_gt_only);
// VCFXG_AF_FUSED is neither 3 nor 8 (the schedules without a walk)
bool af_knob_allows_walk(const vcfxg_ctx *c);
int walk_buffers(vcfxg_ctx *c, const WalkPlan &p);
int dense_buffers(vcfxg_ctx *c, uint64_t L);
int walk_compact(vcfxg_ctx *c, int64_t nw, uint64_t cap_w, unsigned long long *counters, bool aux,
                 const uint64_t *bpre);
int af_walk_to_dense(vcfxg_ctx *c, const WalkPlan &p, int mode, const char *prof_name, size_t small_zero, bool aux,
                     bool dose, bool head, bool cc = false);
int fq_walk_to_dense(vcfxg_ctx *c, const WalkPlan &p, int what, int strip_cr, const RfArgs &ra, const char *q_dev,
                     int qlen, int strict, int qa, int qb, const char *walk_name, const char *rest_name);
int fq_walk_done(vcfxg_ctx *c);

}  // namespace vcfxg
