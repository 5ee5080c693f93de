// vcfxg_kernels.h -- host-visible launchers of the record kernels (vcfxg_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "vcfxg_walk_layout.h"

namespace vcfxg {

// launch shapes: blocks of per_block items each, one at least and max_blocks at most (a grid-stride
// kernel); a block of `threads` for every `threads` items (a kernel of one item per thread)
inline unsigned grid_for(uint64_t items, uint64_t per_block, unsigned max_blocks) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, max_blocks));
}
inline dim3 flat_grid(uint64_t items, unsigned threads) { return dim3((unsigned)((items + threads - 1) / threads)); }

// per-line head summary shared by the AF / GQ head passes (k_line_meta, k_af_combine)
enum : uint8_t { kMetaEmpty = 0, kMetaGt = 1, kMetaFull = 2, kMetaHeader = 3, kMetaGated = 4 };
struct LineMeta {
    uint64_t S;       // sample region start (kMetaGt)
    uint32_t rowpre;  // bytes of "CHROM\tPOS\tID\tREF\tALT\t" (kMetaGt)
    uint8_t kind;     // kMeta*: empty (after the '\r' strip), GT-first data line, full
                      // per-line path, '#' line, gated out (fused RF|GQ: RF dropped it)
    uint8_t sep;      // byte at S + 1 (kMetaGt)
    uint8_t cr;       // a trailing '\r' was stripped
    uint8_t pad;
};
constexpr uint8_t kAfPending = 0xFF;  // AF status of a kMetaGt line whose fast sweep failed
constexpr uint8_t kGqPending = 0xFE;  // GQ: a kMetaGt line whose fast sweep failed (general sweep)
constexpr uint8_t kRfPending = 0xFD;  // RF walk: head beyond the window (k_fq_finish filters it)
constexpr uint8_t kGqFull = 0xFC;     // GQ walk: a kMetaFull line for k_gq_complex's gq_line
// HWE walk: LineMeta::pad of a kMetaGt line -- ALT holds a ',' / CHROM, POS or ALT is empty
constexpr uint8_t kHweAltComma = 1, kHweEmptyField = 2;
// dosage HEAD walk: LineMeta::pad of a GT-only record taken on its predicted end, unswept
constexpr uint8_t kWalkUnswept = 4;
// concordance walk (launch_cc_walk): LineMeta::pad of a kMetaGt line whose CHROM is empty
constexpr uint8_t kCcEmptyChrom = 8;

// single-sweep index over 16 KiB wave-chunks (idx_wchunks of them): counts + the first
// idx_pos_cap() newline offsets per chunk, then a compaction into line_end (overflow != 0:
// some chunk needs the emit sweep launch_idx_emit instead)
int idx_pos_cap();
// BGZF members inflated on the device (vcfxg_inflate.hip): one wave per member into
// out + out_off[m]; mstat[m] = 0 or the first failing check, *first_bad = the lowest bad member
// (initialise to ~0); then each member's CRC-32 against its trailer.  z1k: the images of the 32
// CRC register bits through 1 KiB of zero bytes (crc32_zero1k_basis).
struct BgzfMember {  // = vcfxg_bgzf_member
    uint64_t src_off;
    uint32_t src_len;
    uint32_t out_len;
};
struct Crc1k {
    uint32_t v[32];
};
void crc32_zero1k_basis(Crc1k *z);
// the lane decoder's side stream (the hand-overs') and the events that join it
struct InflateSide {
    hipStream_t aux = nullptr;
    hipEvent_t ev[2] = {};  // decoded, hand-overs done
};
// which: 0 = the inflate (k_inflate_decode; k_inflate_handover, the wave decoder on the members the
// lane decoder hands over, on side->aux beside k_inflate_copy), 1 = k_crc32.  first_bad[0]: the
// first bad member; the 32-bit word after it counts the hand-overs.
hipError_t launch_inflate(int which, const uint8_t *comp, const BgzfMember *mem, const uint64_t *out_off,
                          uint64_t n_members, uint8_t *out, uint32_t *mstat, unsigned long long *first_bad,
                          const Crc1k &z1k, hipStream_t s, uint64_t mbase = 0, uint32_t *tok = nullptr,
                          uint64_t tok_members = 0, const uint32_t *perm = nullptr, const InflateSide *side = nullptr);
// the lane decoder's token buffer: kTokCap 32-bit slots per member, tok_members members (launches
// of more members run in pieces), then the hand-over list of tok_members + 1 words; perm: the
// members in the order the lanes take them (largest compressed first: a wave's lanes then decode
// similar amounts).  No side: every member on the wave decoder.
constexpr uint32_t kTokCap = 6144;
// occurrences of `byte` in buf[lo, hi) added to *out (k_count_byte)
hipError_t launch_count_byte(const uint8_t *buf, uint64_t lo, uint64_t hi, uint8_t byte, unsigned long long *out,
                             hipStream_t s);
int64_t idx_wchunks(int64_t lo, int64_t hi);
hipError_t launch_idx_count(const char *buf, int64_t lo, int64_t hi, uint32_t *counts, uint64_t *pos,
                            unsigned *overflow, hipStream_t s);
hipError_t launch_idx_emit(const char *buf, int64_t lo, int64_t hi, const uint64_t *offs, uint64_t *line_end,
                           hipStream_t s);
hipError_t launch_nl_compact(int64_t lo, int64_t hi, const uint32_t *counts, const uint64_t *offs, const uint64_t *pos,
                             uint64_t *line_end, hipStream_t s);
hipError_t launch_af_records(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                             uint64_t n_lines_host, int mode, int32_t *alt, int32_t *tot, uint32_t *rowpre,
                             uint8_t *status, unsigned long long *counters, hipStream_t s);
// AF head pass (k_af_meta, meta = af_meta_bytes() per line) + sample sweep (k_af_sweep)
size_t af_meta_bytes();
hipError_t launch_af_meta_sweep(const char *buf, int64_t data_start, const uint64_t *line_end,
                                const uint64_t *n_lines_dev, uint64_t n_lines_host, int mode, void *meta, int32_t *alt,
                                int32_t *tot, uint32_t *rowpre, uint8_t *status, unsigned long long *counters,
                                hipStream_t s);
hipError_t launch_af_meta_sweep_range(const char *buf, int64_t data_start, const uint64_t *line_end,
                                      const uint64_t *range, uint64_t max_lines, int mode, void *meta, int32_t *alt,
                                      int32_t *tot, uint32_t *rowpre, uint8_t *status, unsigned long long *counters,
                                      hipStream_t s);
int64_t idx_wchunk_bytes();
// AF record pass without a separate index (vcfxg_af_walk.hip): one wave per `chunk` bytes
// walks its lines (predicted fixed-stride ends validated by the sweep); per-walker regions
// of cap_w lines, then k_walk_compact (offs = exclusive scan of wcount)
int64_t af_walkers(int64_t lo, int64_t hi, int64_t chunk);
// walkers (waves) per block of k_af_walk, and the blocks of one instantiation of it that a CU holds
// at a time (hipOccupancyMaxActiveBlocksPerMultiprocessor on the current device; 0 on error)
int af_walk_waves_per_block();
int af_walk_resident_blocks(int depth, bool roll);
// the AF walk's region tail (all null: the walk only fills its regions): per walker its row
// bytes (GT lines) and first line start, and the list of region slots left to the exact
// per-line path (kMetaFull lines, GT lines off the fixed-stride sweep)
struct WalkTail {
    uint64_t *wtext = nullptr;
    uint64_t *wstart = nullptr;
    uint64_t *cx_list = nullptr;
    unsigned long long *cx_n = nullptr;
    uint64_t cx_cap = 0;
    // AF: each walker's rows as text, composed by the walk itself into its stage_cap bytes of
    // stage (k_af_format_w then copies them out whole); wdirty[w] = 1 when the walker left a
    // line to k_af_cx or its rows outgrew its stage (its rows are formatted from the arrays)
    char *stage = nullptr;
    uint32_t stage_cap = 0;
    uint8_t *wdirty = nullptr;
};
// depth / roll: the sample sweep's wave-steps (KiB of a record) in flight, and whether a record
// longer than that continues rolling (vcfxg_gt.h af_fixed).  Every walk is compiled for the
// batches of kAfDepthDefault; the AF GT-only walk also for the rolling sweeps of
// af_depth_compiled.  Anything else: hipErrorInvalidValue
constexpr int kAfDepthDefault = 6, kAfDepthMax = 12;
constexpr int kAfWaveStep = 1024;  // bytes of a wave-step (vcfxg_device.h kWaveStep, for the host's plan)
constexpr bool af_depth_compiled(int d) { return d == 6 || d == 8 || d == 10 || d == 12; }
// lay: the walkers' bytes (vcfxg_walk_layout.h; walk_layout_make over [lo, hi) with kWalkWaves
// walkers a block): its grid is launched, its first nw walkers write their regions
hipError_t launch_af_walk(const char *buf, int64_t lo, int64_t hi, const WalkLayout &lay, int mode, int64_t span0,
                          uint64_t cap_w, uint64_t *le_b, int32_t *alt_b, int32_t *tot_b, uint32_t *rowpre_b,
                          uint8_t *status_b, void *meta_b, uint64_t *wcount, uint32_t *wgt, unsigned *overflow,
                          hipStream_t s, int32_t *hwe_aux_b = nullptr, const WalkTail *tail = nullptr,
                          bool dose = false, bool gt_first_walk = false, bool dose_head = false,
                          int depth = kAfDepthDefault, bool roll = false);
// the same walk with the concordance reducer (vcfxg_cc.hip: k_af_walk<CcOp>): valid samples and
// distinct keys of every fixed-stride record as alt_b / tot_b
hipError_t launch_cc_walk(const char *buf, int64_t lo, int64_t hi, const WalkLayout &lay, int mode, int64_t span0,
                          uint64_t cap_w, uint64_t *le_b, int32_t *alt_b, int32_t *tot_b, uint32_t *rowpre_b,
                          uint8_t *status_b, void *meta_b, uint64_t *wcount, uint32_t *wgt, unsigned *overflow,
                          hipStream_t s);
// AF region tail without the dense per-line arrays (vcfxg_kernels.hip):
//   launch_af_cx       the walk's leftover slots: af_line / the general sweep, new rows' bytes
//                      added to their walker's total (counters as k_af_complex)
//   launch_walker_scan one block: exclusive scans of the walkers' line counts and row bytes,
//                      GT-line totals into counters[0..1], the line count to *n_lines and the
//                      7-value call summary (lines, text bytes, counters[0..3], *fail); with
//                      reset: summary[7] = reset[1] (the leftover count), then reset[0..5] = 0
//   launch_af_format_w one wave per walker region: rows into out (rows ending past cap skipped)
hipError_t launch_af_cx(const char *buf, int mode, uint64_t cap_w, const uint64_t *list, const unsigned long long *list_n,
                        uint64_t list_cap, uint64_t list_cap_host, const uint64_t *wstart, const uint64_t *le_b,
                        const void *meta_b, int32_t *alt_b, int32_t *tot_b, uint32_t *rowpre_b, uint8_t *status_b,
                        uint64_t *wtext, unsigned long long *counters, hipStream_t s);
// walker offsets are block-local: woff[w] + bpre[w / kWalkerScanBlock] (bsum: 3 per block,
// bpre_*: blocks + 1 entries; *done zero before the launch)
constexpr int kWalkerScanBlock = 1024;
hipError_t launch_walker_scan(int64_t nw, const uint64_t *wcount, const uint64_t *wtext, const uint32_t *wgt,
                              uint64_t *woff, uint64_t *wtoff, uint64_t *bpre_a, uint64_t *bpre_b, uint64_t *bsum,
                              unsigned *done, unsigned long long *counters, const unsigned *fail, uint64_t *n_lines,
                              uint64_t *summary, hipStream_t s, uint64_t *reset = nullptr);
hipError_t launch_af_format_w(const char *buf, int mode, int64_t nw, uint64_t cap_w, const uint64_t *wcount,
                              const uint64_t *wtoff, const uint64_t *bpre_b, const uint64_t *wstart,
                              const uint64_t *le_b, const int32_t *alt_b, const int32_t *tot_b, const uint32_t *rowpre_b,
                              const uint8_t *status_b, char *out, uint64_t cap, hipStream_t s, const WalkTail *tail = nullptr);
hipError_t launch_walk_compact(int64_t n_walkers, uint64_t cap_w, const uint64_t *offs, const uint32_t *wgt,
                               const uint64_t *le_b, const int32_t *alt_b, const int32_t *tot_b,
                               const uint32_t *rowpre_b, const uint8_t *status_b, const void *meta_b,
                               uint64_t *line_end, int32_t *alt, int32_t *tot, uint32_t *rowpre, uint8_t *status,
                               void *meta, uint64_t *n_lines, unsigned long long *counters, hipStream_t s,
                               const int32_t *aux_b = nullptr, int32_t *aux = nullptr, const uint64_t *bpre = nullptr);
hipError_t launch_af_complex(const char *buf, int64_t data_start, const uint64_t *line_end,
                             const uint64_t *n_lines_dev, uint64_t n_lines_host, int mode, const void *meta,
                             int32_t *alt, int32_t *tot, uint32_t *rowpre, uint8_t *status,
                             unsigned long long *counters, hipStream_t s);
// VCFX_nonref_filter per line (mode 0 mmap, 1 stdin): status 1 keep / 2 drop / 4 '#' / 0 empty;
// counters: [0] kept, [1] data lines, [3] lines off the fixed-stride sweep
// after the nonref walk: nr_line for the lines it left (kGqPending / kGqFull), counters as above
hipError_t launch_nr_complex(const char *buf, int64_t data_start, const uint64_t *line_end,
                             const uint64_t *n_lines_dev, uint64_t n_lines_host, int mode, uint8_t *status,
                             unsigned long long *counters, hipStream_t s);
hipError_t launch_nr_records(const char *buf, int64_t data_start, const uint64_t *line_end,
                             const uint64_t *n_lines_dev, uint64_t n_lines_host, int mode, uint8_t *status,
                             unsigned long long *counters, hipStream_t s);
hipError_t launch_gq_records(const char *buf, int64_t data_start, const uint64_t *line_end,
                             const uint64_t *n_lines_dev, uint64_t n_lines_host, int strip_cr, const char *q_dev,
                             int qlen, int strict, int qa, int qb, uint8_t *status, unsigned long long *counters,
                             hipStream_t s, const uint8_t *gate, void *meta = nullptr);
// k_gq_complex alone (the query's general lines after the filter / query walk): lines of
// kind kMetaFull (gq_line) and kMetaGt lines with status kGqPending (general sweep)
hipError_t launch_gq_complex(const char *buf, int64_t data_start, const uint64_t *line_end,
                             const uint64_t *n_lines_dev, uint64_t n_lines_host, int strip_cr, const char *q_dev,
                             int qlen, int strict, int qa, int qb, const void *meta, uint8_t *status,
                             unsigned long long *counters, const uint8_t *gate, hipStream_t s);
// asynchronous AF region path: capacity-guarded compaction, device-side line count and
// a one-record summary for the single host synchronisation
hipError_t launch_nl_compact_cap(int64_t lo, int64_t hi, const uint32_t *counts, const uint64_t *offs,
                                 const uint64_t *pos, uint64_t *line_end, uint64_t cap, hipStream_t s);
hipError_t launch_idx_finish(const uint64_t *offs, int64_t nchunks, const unsigned *idx_overflow, int tail, int64_t hi,
                             uint64_t cap, uint64_t *line_end, uint64_t *n_lines, unsigned *fail, hipStream_t s);
hipError_t launch_af_summary(const uint64_t *n_lines, const uint64_t *rowoff, const unsigned long long *counters,
                             const unsigned *fail, uint64_t *out, hipStream_t s);
hipError_t launch_af_rowlen(const uint32_t *rowpre, const uint8_t *status, const uint64_t *n_lines_dev,
                            uint64_t n_lines_host, uint64_t *len, hipStream_t s);
// VCFX_hwe_tester (vcfxg_hwe.hip): the exact per-line pass (meta == nullptr: every line;
// else the walk's kMetaFull / kAfPending lines), the row lengths (the walk's CHROM..ALT flags
// applied when meta != nullptr; counters[0] += rows), and the rows (rechecks: vcfxg_hwe_recheck entries, *rc_n counted)
hipError_t launch_hwe_lines(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                            uint64_t n_lines_host, int mode, const void *meta, int32_t *c0, int32_t *c1, int32_t *c2,
                            uint32_t *rowpre, uint8_t *status, unsigned long long *counters, hipStream_t s);
hipError_t launch_hwe_rowlen(const uint64_t *n_lines_dev, uint64_t n_lines_host, int mode, const void *meta,
                             const uint32_t *rowpre, uint8_t *status, uint64_t *len, unsigned long long *counters,
                             hipStream_t s);
hipError_t launch_hwe_format(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                             uint64_t n_lines_host, int mode, const int32_t *c0, const int32_t *c1, const int32_t *c2,
                             const uint32_t *rowpre, const uint8_t *status, const uint64_t *off, char *out,
                             uint64_t text_cap, int64_t ulps, void *rc, unsigned long long *rc_n, uint64_t rc_cap,
                             hipStream_t s);
// VCFX_dosage_calculator (vcfxg_dose.hip) over the indexed lines: per line status (1 row,
// 3 "< 10 fields", 0 skip), row length and meta (dose_meta_bytes() each; counters[0] rows,
// [2] warnings, [3] lines off the fixed-stride sweep); then the rows at their offsets
size_t dose_meta_bytes();
hipError_t launch_dose_len(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                           uint64_t n_lines_host, int mode, uint8_t *status, uint64_t *len, void *meta,
                           unsigned long long *counters, hipStream_t s, bool pending_only = false);
// after the dosage walk (launch_af_walk dose, compacted): the walk's fixed-stride GT-only lines
// become rows (ns = alt, na = tot), '#' / empty lines are skipped, every other line is left
// pending for launch_dose_len(pending_only); status is rewritten in place, meta is the dose meta
hipError_t launch_dose_from_walk(const uint64_t *line_end, const uint64_t *n_lines_dev, uint64_t n_lines_host,
                                 const void *walk_meta, const int32_t *ns, const int32_t *na, uint8_t *status,
                                 uint64_t *len, void *meta, unsigned long long *counters, hipStream_t s);
hipError_t launch_dose_fmt(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                           uint64_t n_lines_host, const uint8_t *status, const void *meta, const uint64_t *off,
                           char *out, uint64_t cap, uint64_t slow_rows, hipStream_t s, unsigned *bad = nullptr,
                           uint64_t na_rows = ~0ull);
// VCFX_missing_detector (vcfxg_md.hip) over the indexed lines: per line status (0 empty, 4 '#',
// 1 kept as is, kMdFlag flagged) and the flagged lines' INFO span relative to the line start;
// counters [0] data lines, [1] flagged, [2] lines ending in '\n' with a '.' in their samples;
// walk: the statuses hold the missing-detector walk's decisions (1 / kMdFlag taken as they are)
constexpr uint8_t kMdFlag = 6;
hipError_t launch_md_lines(const char *buf, int64_t data_start, int64_t n_input, const uint64_t *line_end,
                           const uint64_t *n_lines_dev, uint64_t n_lines_host, int mode, uint8_t *status,
                           int32_t *info_s, int32_t *info_e, unsigned long long *counters, hipStream_t s,
                           int walk = 0);
// VCFX_allele_counter (vcfxg_ac.hip) over indexed lines [l0, l1): per line status (1 data,
// 4 '#CHROM', 0 other), row bytes (len[li - l0]) and meta (ac_meta_bytes() each); counters
// [0] rows, [1] data lines, [2] '#CHROM' lines, [3] lines off the fixed-stride sweep.  eff:
// per output slot the sample index it reads; scratch: ac_threads() / 64 * blocks * scap u32;
// sel_lds: LDS bytes for the selection in k_ac_fmt (4 m + 4 (m + 1) + name bytes), 0 = global
size_t ac_meta_bytes();
int ac_threads();
hipError_t launch_ac_len(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t l1,
                         unsigned blocks, const uint32_t *eff, const uint64_t *noff, const char *names,
                         uint32_t *scratch, uint32_t m, uint32_t scap, int seq, int kind, int ident, int direct,
                         uint32_t *nib, uint8_t *status, uint64_t *len, void *meta, unsigned long long *counters,
                         hipStream_t s);
// direct != 0 (text rows, every name L <= 11 bytes, m <= 4096, ac_rows_lds <= ac_rows_lds_max()): k_ac_rows writes
// the fixed-stride records whose prefix is 16..64 bytes (etab: per slot 16 B, the name at bytes
// [11 - L, 11), then "\t0\t0\n", zeros in front; nib: k_ac_len's counts, per line li - l0
// ceil(m / 64) tiles of 8 dwords) and k_ac_fmt the others; k_ac_len counts the others' data lines
// in counters[4] (0: no k_ac_fmt launch needed)
hipError_t launch_ac_fmt(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t l1,
                         unsigned blocks, const uint32_t *eff, const uint64_t *noff, const char *names,
                         uint32_t *scratch, uint32_t m, uint32_t scap, int seq, int kind, uint32_t sel_lds,
                         int ident, int direct, const uint8_t *status, const void *meta, const uint64_t *off,
                         char *out, hipStream_t s);
hipError_t launch_ac_rows(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t l1,
                          unsigned blocks, const uint32_t *eff, uint32_t m, int ident, const void *etab, uint32_t L,
                          const uint32_t *nib, const void *meta, const uint64_t *off, char *out, hipStream_t s);
size_t ac_rows_lds(uint32_t m, int ident);  // k_ac_rows' dynamic LDS bytes (m <= 4096)
size_t ac_rows_lds_max();
int ac_rows_threads();
// VCFX_haplotype_phaser (vcfxg_ph.hip): per line status (kPh*), the variants' genotype codes
// (row = line, kpad bytes; counters[3] = the largest sample count past kpad), the variant ->
// line compaction, per variant the pair flags with its predecessor (bit 0 the block rule
// passes, bit 1 same CHROM) + r^2 + entry length, and the entries "v:(chrom:pos)"
enum : uint8_t { kPhSkip = 0, kPhVar = 1, kPhFew = 3, kPhHeader = 4, kPhPos = 7, kPhNoGt = 8 };
size_t ph_line_bytes();
// walk_meta (nullable): the head walk's LineMeta per line (its index); a line taken unswept
// (kWalkUnswept) that the parse does not validate by the fixed-stride sweep sets *bad
hipError_t launch_ph_lines(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                           uint64_t n_lines_host, int mode, uint32_t kpad, int8_t *G, uint8_t *status, uint32_t *isvar,
                           void *info, unsigned long long *counters, hipStream_t s, const void *walk_meta = nullptr,
                           unsigned *bad = nullptr);
hipError_t launch_ph_compact(const uint32_t *isvar, const uint64_t *vnum, const uint64_t *n_lines_dev,
                             uint64_t n_lines_host, uint64_t *vline, uint64_t *n_var, hipStream_t s);
hipError_t launch_ph_pairs(const char *buf, const uint64_t *vline, const uint64_t *n_var_dev, uint64_t n_var_host,
                           const void *info, const int8_t *G, uint32_t kpad, double thr, uint8_t *flags, uint64_t *len,
                           double *r2, hipStream_t s);
hipError_t launch_ph_fmt(const char *buf, const uint64_t *vline, const uint64_t *n_var_dev, uint64_t n_var_host,
                         const void *info, const uint64_t *off, char *out, hipStream_t s);
// text_cap: rows whose end passes it are not written (the caller checks the total)
hipError_t launch_af_format(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                            uint64_t n_lines_host, int mode, const int32_t *alt, const int32_t *tot,
                            const uint32_t *rowpre, const uint8_t *status, const uint64_t *off, char *out,
                            hipStream_t s, uint64_t text_cap = ~0ull);

// VCFX_inbreeding_calculator (vcfxg_ib.hip).  Stage A fills, per slot, a meta record
// (ib_meta_bytes(): status 0 skipped / 1 parsed / 2 used, altSum, nGood, nparsed) and a row of
// ld int8 codes: launch_ib_walk with G walkers (chunks w0 .. w0 + G of nw over [lo, hi)), walker
// g's lines in slots [g cap_w, g cap_w + cnt[g]), *ovf set when a walker has more lines than
// cap_w; or launch_ib_lines over indexed lines [l0, l0 + n) (one group: cnt[0] = n, cap_w >= n).
// counters [0] parsed records, [1] used records.  Stage B (launch_ib_table): offs = the scan of
// cnt (G + 1 entries, offs[G] = the block's records) and, in file order, one record entry
// (ib_rec_bytes()) per line: status, nparsed, slot, and for a used record the sumExp term of a
// sample of code 0 / 1 / 2 with the boundary flag bits.  Stage C (launch_ib_chain): a lane per
// sample over the block's n_rec[0] record entries (codes regrouped by launch_ib_pack), the per-sample state (sum_exp, obs_het, used,
// carried code) read and written back.  launch_ib_rows: the rows.
size_t ib_meta_bytes();
size_t ib_rec_bytes();
hipError_t launch_ib_walk(const char *buf, int64_t lo, int64_t hi, int64_t chunk, int64_t w0, int64_t nw, uint32_t G,
                          uint32_t cap_w, int mode, uint32_t ns, uint32_t ld, int8_t *codes, void *meta, uint32_t *cnt,
                          unsigned *ovf, unsigned long long *counters, hipStream_t s);
hipError_t launch_ib_lines(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint32_t n,
                           int mode, uint32_t ns, uint32_t ld, int8_t *codes, void *meta, uint32_t *cnt,
                           unsigned long long *counters, hipStream_t s);
hipError_t launch_ib_table(const void *meta, const uint32_t *cnt, uint32_t *offs, uint32_t G, uint32_t cap_w,
                           int global_freq, void *rec, hipStream_t s);
// (slots: the block's slot capacity; packed: ib_packed_bytes(slots, ns) bytes, the codes regrouped
// per 64-sample tile and 16 records; rec needs room for slots + 16 entries)
size_t ib_packed_bytes(uint64_t slots, uint32_t ns);
hipError_t launch_ib_pack(const int8_t *codes, uint32_t ld, const void *rec, const uint32_t *n_rec, uint64_t slots,
                          void *packed, uint32_t ns, hipStream_t s);
hipError_t launch_ib_chain(const void *rec, const uint32_t *n_rec, uint64_t slots, const void *packed, uint32_t ns,
                           int mode, int skip_boundary, int count_boundary, double *sum_exp, uint64_t *obs_het,
                           uint64_t *used, int32_t *carried, hipStream_t s);
hipError_t launch_ib_rows(const double *sum_exp, const uint64_t *obs_het, const uint64_t *used, uint32_t ns,
                          const char *names, const uint64_t *noff, char *out, uint64_t *text_bytes, hipStream_t s);

// VCFX_sample_extractor (vcfxg_sx.hip) over indexed lines [l0, l1), a wave per line.  mask:
// nwords + 2 words, bit f = field f of a line is kept (bits 0..8 set; the last two words zero),
// lastk the largest kept field number (8 without a kept column), m the kept columns.
// launch_sx_len: per line its status (kSx*) and output bytes (len[li - l0]); counters [0] lines
// written, [1] data lines, [2] skipped data lines, [3] '#CHROM' lines (stdin mode).
// launch_sx_write: the lines' bytes at off[li - l0] (the scan of len, l1 - l0 + 1 entries) of out
// (16 B aligned).  A line passes through a ring of sx_stage_bytes() per wave, drained every 1 KiB.
enum : uint8_t { kSxEmpty = 0, kSxRow = 1, kSxShort = 3, kSxHeader = 4, kSxNoSample = 5, kSxPre = 6, kSxChrom = 7 };
int sx_threads();
uint32_t sx_stage_bytes();
hipError_t launch_sx_len(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t l1,
                         unsigned blocks, const uint32_t *mask, uint32_t nwords, uint32_t lastk, uint32_t m,
                         int stdin_mode, int seen, uint8_t *status, uint64_t *len, unsigned long long *counters,
                         hipStream_t s);
hipError_t launch_sx_write(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t l1,
                           unsigned blocks, const uint32_t *mask, uint32_t nwords, uint32_t lastk, uint32_t m,
                           int stdin_mode, int seen, const uint8_t *status, const uint64_t *off, char *out,
                           hipStream_t s);

// VCFX_cross_sample_concordance (vcfxg_cc.hip) over the indexed lines (*n_lines_dev of them, at
// most n_lines_host).  launch_cc_lines: per line its status (0 no row, kCc*), valid calls (n_o),
// distinct keys (u_o), the bytes of CHROM..ALT (rowpre) and whether it counts as a data line
// (isdata), a wave per line; mult: per sample column (field 9 + i) how often it is selected,
// n_mult entries (nullptr: each of the first ns once); meta: nullptr, or the concordance walk's
// LineMeta (n_o / u_o / status hold its results): only the lines it left are parsed; counters
// [0] concordant, [1] discordant, [2] no-genotype rows, [3] lines parsed by this kernel.
// launch_cc_chrom: the starts of the lines that begin with "#CHROM" (the first cap of them, any
// order; *n = their number).  ord = the exclusive scan of isdata (lines + 1 entries).
// launch_cc_rowlen: len[place of the line] = its row's bytes, T = the reference's worker count
// (0: record order; len zeroed beforehand); launch_cc_summary: out[0] data lines, [1] text bytes,
// [2..5] the counters, [6] lines, [7] *fail; launch_cc_format: the rows at off[place] that end
// within text_cap.
enum : uint8_t { kCcSame = 1, kCcDiff = 2, kCcNoGt = 3 };
hipError_t launch_cc_lines(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                           uint64_t n_lines_host, int mode, uint32_t ns, const uint32_t *mult, uint32_t n_mult,
                           const void *meta, int32_t *n_o, int32_t *u_o, uint32_t *rowpre, uint8_t *status,
                           uint32_t *isdata, unsigned long long *counters, hipStream_t s);
hipError_t launch_cc_chrom(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                           uint64_t n_lines_host, uint64_t *out, uint64_t cap, unsigned long long *n, hipStream_t s);
hipError_t launch_cc_rowlen(const uint64_t *n_lines_dev, uint64_t n_lines_host, uint64_t T, const uint64_t *ord,
                            const uint32_t *isdata, const uint8_t *status, const int32_t *nn, const int32_t *uu,
                            const uint32_t *rowpre, uint64_t *len, hipStream_t s);
hipError_t launch_cc_summary(const uint64_t *n_lines_dev, const uint64_t *ord, const uint64_t *off,
                             const unsigned long long *counters, const unsigned *fail, uint64_t *out, hipStream_t s);
hipError_t launch_cc_format(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                            uint64_t n_lines_host, uint64_t T, const uint64_t *ord, const uint8_t *status,
                            const int32_t *nn, const int32_t *uu, const uint32_t *rowpre, const uint64_t *off, char *out,
                            uint64_t text_cap, hipStream_t s);

// VCFX_duplicate_remover (vcfxg_dd.hip) over the L indexed lines.  launch_dd_key: per line its
// status (kDdEmpty / kDdHeader / kDdShort, or undecided) and isdata (1 = undecided data line), and
// for a data line the offsets of its first five tabs (tabs[5 li ..], the fifth = ALT's end), POS
// and the key's hash; a lane per line over the first kDdWindow bytes, then a wave per line that
// pass does not settle (listed in queue, L entries; counters[5] counts them); n = the input's
// bytes.  launch_dd_gather: (hash masked to hash_bits when 1..63, line) at ord[line] (the
// exclusive scan of isdata).  After the stable sort of the nd pairs: launch_dd_heads hp[j] = j at
// a run's first element, else 0; head = its inclusive max scan; launch_dd_verify: heads kDdKept,
// elements equal to their head kDdDup, the others resolved in line order against their run's kept
// elements (left: nd zeroed bytes; counters[6] counts them).  launch_dd_count: counters[0..4] +=
// the lines of each status.
enum : uint8_t { kDdEmpty = 0, kDdKept = 1, kDdDup = 2, kDdShort = 3, kDdHeader = 4 };
constexpr int kDdWindow = 64;
hipError_t launch_dd_key(const char *buf, int64_t data_start, int64_t n, const uint64_t *line_end, uint64_t L,
                         int stdin_mode, uint8_t *status, uint32_t *isdata, uint64_t *tabs, int32_t *pos, uint64_t *hash,
                         uint32_t *queue, unsigned long long *counters, hipStream_t s);
hipError_t launch_dd_gather(uint64_t L, const uint32_t *isdata, const uint64_t *ord, const uint64_t *hash,
                            uint32_t hash_bits, uint64_t *keys, uint32_t *vals, hipStream_t s);
hipError_t launch_dd_heads(uint64_t nd, const uint64_t *keys, uint32_t *hp, hipStream_t s);
hipError_t launch_dd_verify(const char *buf, int64_t data_start, const uint64_t *line_end, int stdin_mode,
                            const uint64_t *tabs, const int32_t *pos, uint64_t nd, const uint64_t *keys, const uint32_t *vals,
                            const uint32_t *head, uint8_t *status, uint8_t *left, unsigned long long *counters,
                            hipStream_t s);
hipError_t launch_dd_count(uint64_t L, const uint8_t *status, unsigned long long *counters, hipStream_t s);

// VCFX_multiallelic_splitter (vcfxg_ms.hip) over n indexed lines from l0.  launch_ms_scan: per line
// its status (kMs*), nAlts (alt[line]; 0 unless it splits), and per line of the block (i = line -
// l0) the offsets of its nine tabs and its end (geom[kMsGeom i ..]; file mode drops one trailing
// tab first) and its cost nAlts x (bytes + 1).  launch_ms_cut: small[0] = the lines whose summed
// cost (costoff: the scan of cost) stays within budget, one at least; small[1] = their rows
// (rowbase: the scan of alt from l0).  launch_ms_len / launch_ms_write: a wave per row, its bytes
// counted (len[row]; counters[1] += the lines past a cap) or written at off[row] of out.  table:
// entries x {ID offset in bytes, ID length, section << 8 | class} then the ID bytes, table_bytes
// in all (a multiple of 4), one entry per ID; in LDS up to kMsTableLds bytes.  launch_ms_ranges:
// lineoff[i] = off[rowbase[i]] (n + 1 entries), counters[0] += the data lines.
enum : uint8_t { kMsEmpty = 0, kMsCopy = 1, kMsSplit = 2, kMsHeader = 4 };
enum : uint32_t { kMsOther = 0, kMsA = 1, kMsR = 2, kMsG = 3 };
enum : uint32_t { kMsInfo = 0, kMsFormat = 1 };
constexpr uint32_t kMsKeysLds = 32;      // FORMAT keys whose classes a wave keeps in LDS; later keys: looked up per use
constexpr uint32_t kMsTableLds = 16384;  // table bytes kept in LDS; larger: global loads
constexpr int kMsGeom = 10;
hipError_t launch_ms_scan(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                          int stdin_mode, uint8_t *status, int32_t *alt, uint32_t *geom, uint64_t *cost, hipStream_t s);
hipError_t launch_ms_cut(const uint64_t *costoff, const uint64_t *rowbase, uint64_t n, uint64_t budget, uint64_t *small,
                         hipStream_t s);
hipError_t launch_ms_len(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                         int stdin_mode, const uint32_t *table, uint32_t table_bytes, uint32_t entries, uint64_t rows,
                         const uint64_t *rowbase, const int32_t *alt, const uint32_t *geom, uint64_t *len,
                         unsigned long long *counters, hipStream_t s);
hipError_t launch_ms_write(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                           int stdin_mode, const uint32_t *table, uint32_t table_bytes, uint32_t entries, uint64_t rows,
                           const uint64_t *rowbase, const int32_t *alt, const uint32_t *geom, const uint64_t *off,
                           char *out, hipStream_t s);
hipError_t launch_ms_ranges(uint64_t l0, uint64_t n, const uint8_t *status, const uint64_t *rowbase,
                            const uint64_t *rowoff, uint64_t *lineoff, unsigned long long *counters, hipStream_t s);

// VCFX_fasta_converter (vcfxg_fa.hip) over n indexed lines from l0.  launch_fa_scan: per line its
// status (kFa*; stdin mode's field rule uses n_samples), per line of the block (i = line - l0) the
// column flag and FaMeta: the sample region [S, E) and ALT [alt_s, alt_e) as offsets from the line's
// start (E excludes the file mode's '\r'; S = E = 0 for a line of fewer than ten fields), the GT
// key's index (-1: none), the REF base (tab[0]) and the bases of ALT alleles 1..15; counters[1] +=
// the "#CHROM" lines.  launch_fa_bases: a wave per column line writes its n_samples bases (0 for a
// sample the line lacks) at M[col[i] * pitch ..] (col: the scan of the flags); counters[0] += the
// lines off the fixed-stride path.  launch_fa_transpose: M rows [0, ncols) are columns first_col ..
// of total_cols; sample s, column g goes to text[row_off[s] + c + c / 60], c = g - skip[s] (skip may
// be null), with the '\n' after every 60th base and after the row's last.
enum : uint8_t { kFaEmpty = 0, kFaColumn = 1, kFaSkipped = 3, kFaHeader = 4, kFaChrom = 7 };
constexpr uint32_t kFaLine = 60;         // bases per FASTA line
constexpr uint32_t kFaTileSamples = 64;  // the transpose tile
constexpr uint32_t kFaTileCols = 240;
constexpr uint32_t kFaTable = 16;        // alleles whose base the scan tabulates
struct FaMeta {
    uint32_t S, E, alt_s, alt_e;
    int32_t gi;
    uint32_t pad[3];
    uint8_t tab[16];
};
static_assert(sizeof(FaMeta) == 48, "FaMeta: twelve words");
hipError_t launch_fa_scan(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                          int stdin_mode, uint32_t n_samples, uint8_t *status, uint32_t *flag, FaMeta *meta,
                          unsigned long long *counters, hipStream_t s);
hipError_t launch_fa_bases(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                           const uint8_t *status, const uint64_t *col, const FaMeta *meta, uint32_t n_samples,
                           uint64_t pitch, uint8_t *M, unsigned long long *counters, hipStream_t s);
hipError_t launch_fa_transpose(const uint8_t *M, uint64_t pitch, uint64_t ncols, uint32_t n_samples, uint64_t first_col,
                               uint64_t total_cols, const uint64_t *row_off, const uint64_t *skip, char *text,
                               hipStream_t s);

// VCFX_sorter (vcfxg_srt.hip) over the L indexed lines.  launch_srt_key: per line its status (kSrt*,
// without kSrtPre), POS, aux (natural order: chromToId; lexicographic: CHROM's length) and, for the
// lexicographic order, CHROM's first eight bytes big-endian and zero-padded (w0); a lane per line
// whose key fields end in its first kSrtWindow bytes, then a wave per line that pass does not settle
// (queue: L entries; counters[5] counts them); counters[6] = max(L - li) over the "#CHROM" lines.
// launch_srt_class: file mode's data lines before the first "#CHROM" line become kSrtPre;
// written[li] = 1 for a line of the output (header, kept; stdin mode: empty); counters[0..4] += the
// lines per status, counters[7] = the longest kept CHROM.  launch_srt_scatter: line and first-pass
// key of every written line at ord[line] (the exclusive scan of written): natural (id, POS) in one
// word, lexicographic (CHROM length + 1) << 32 | POS; a header line's key is 0, a stdin-mode empty
// CHROM's length word all ones.  launch_srt_word: keys[j] = word w of the CHROM of line vals[j] (0
// for a header line, all ones for stdin mode's empty CHROM), shifted right by `shift` bits.  The output
// lines are placed and gathered by launch_line_len and launch_text_gather (below).
enum : uint8_t { kSrtEmpty = 0, kSrtKept = 1, kSrtPre = 2, kSrtBad = 3, kSrtHeader = 4 };
constexpr int kSrtWindow = 64;
hipError_t launch_srt_key(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t L, int stdin_mode,
                          int natural, uint8_t *status, int32_t *pos, uint32_t *aux, uint64_t *w0, uint32_t *queue,
                          unsigned long long *counters, hipStream_t s);
hipError_t launch_srt_class(uint64_t L, int stdin_mode, int natural, uint8_t *status, const uint32_t *aux,
                            uint32_t *written, unsigned long long *counters, hipStream_t s);
hipError_t launch_srt_scatter(uint64_t L, int stdin_mode, int natural, const uint8_t *status, const uint32_t *written,
                              const uint64_t *ord, const int32_t *pos, const uint32_t *aux, uint64_t *keys,
                              uint32_t *vals, hipStream_t s);
hipError_t launch_srt_word(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t nw, int stdin_mode,
                           uint32_t w, uint32_t shift, const uint32_t *vals, const uint8_t *status, const uint32_t *aux,
                           const uint64_t *w0, uint64_t *keys, hipStream_t s);
// VCFX_diff_tool (vcfxg_df.hip) over the L indexed lines of two files in one text; the lines from
// `cut` on are file 2's (launch_df_cut: counters[7] = the first line that starts at or after
// second_start).  launch_df_key: per line its status (kDfEmpty / kDfHeader / kDfSkipped, or kDfData:
// undecided) and isdata, and for a data line the offsets of its first five tabs (the fifth = ALT's
// end: the tab or the line's end without one '\r'), the key's length, ALT's token count, POS as an
// integer and CHROM's natural-order parts (the digit prefix's value after the "chr" prefix, -1
// without one, and where the rest of the name begins); a lane per line whose key fields end in its
// first kDfWindow bytes, then a wave per line that pass does not settle (queue: L entries;
// counters[5] counts them); counters[4] += the skipped lines.  launch_df_text: every data line's
// key text CHROM:POS:REF:ALT' at koff[line] of ktext (ALT' = ALT's tokens in byte order), its hash,
// and line[ord[line]] = line (ord: the exclusive scan of isdata); queue as above, counters[9].
// Default mode, after the stable sort of the nd (hash, line) pairs and the run heads
// (launch_dd_heads, max scan): launch_df_classes: rep[j] = the first element of j's run with j's
// key (exact compares; left: nd zeroed bytes, counters[6] the elements that differ from their head),
// first2[rep] = the class's first element of file 2, then each line's status.  Sorted mode:
// launch_df_ordered: counters[8] = 1 when a data line compares greater than the next one of its
// file; launch_df_bounds: each data line's status from three binary searches; launch_df_walk: at
// most `steps` steps of the two-pointer loop from state[0..1] (one wave); launch_df_drain: the lines
// the loop left are unique.  launch_df_flag: uflag[line] = 1 for a unique line (uflag[L] = 0);
// launch_df_place: len / src of every unique line at uord[line] (len[U] = 0) for launch_text_gather;
// launch_df_sum: sum[0..7] = vcfxg_diff_counts' words but the path.
enum : uint8_t { kDfEmpty = 0, kDfCommon = 1, kDfUnique = 2, kDfSkipped = 3, kDfHeader = 4, kDfRepeat = 5, kDfData = 6 };
constexpr int kDfWindow = 64;
struct DfLines {
    const char *buf;
    int64_t data_start;
    const uint64_t *line_end;
    uint64_t L;
    uint8_t *status;
    uint32_t *isdata, *ntok;
    uint64_t *tabs, *klen, *nsuf;
    int64_t *posv, *natv;
};
hipError_t launch_df_cut(const uint64_t *line_end, int64_t data_start, uint64_t L, uint64_t second_start,
                         unsigned long long *counters, hipStream_t s);
hipError_t launch_df_key(const DfLines &D, int natural, uint32_t *queue, unsigned long long *counters, hipStream_t s);
hipError_t launch_df_text(const DfLines &D, const uint64_t *ord, const uint64_t *koff, char *ktext, uint64_t *hash,
                          uint32_t *line, uint32_t *queue, unsigned long long *counters, hipStream_t s);
hipError_t launch_df_pairs(uint64_t nd, const uint32_t *line, const uint64_t *hash, uint32_t hash_bits, uint64_t *keys,
                           uint32_t *vals, hipStream_t s);
hipError_t launch_df_classes(const char *ktext, const uint64_t *koff, const uint64_t *klen, uint64_t nd, const uint64_t *keys,
                             const uint32_t *vals, const uint32_t *head, uint32_t *rep, uint32_t *first2, uint8_t *left,
                             uint8_t *status, unsigned long long *counters, hipStream_t s);
hipError_t launch_df_ordered(const DfLines &D, int natural, const uint32_t *line, uint64_t n1, uint64_t nd,
                             unsigned long long *counters, hipStream_t s);
hipError_t launch_df_bounds(const DfLines &D, int natural, const uint32_t *line, uint64_t n1, uint64_t nd, hipStream_t s);
hipError_t launch_df_walk(const DfLines &D, int natural, const uint32_t *line, uint64_t n1, uint64_t nd, uint64_t steps,
                          uint64_t *state, hipStream_t s);
hipError_t launch_df_drain(const uint32_t *line, uint64_t n1, uint64_t nd, const uint64_t *state, uint8_t *status,
                           hipStream_t s);
hipError_t launch_df_flag(uint64_t L, const uint8_t *status, uint32_t *uflag, hipStream_t s);
hipError_t launch_df_place(uint64_t L, const uint32_t *uflag, const uint64_t *uord, const uint64_t *koff,
                           const uint64_t *klen, uint64_t *len, uint64_t *src, hipStream_t s);
hipError_t launch_df_sum(uint64_t L, const uint64_t *ord, const uint64_t *uord, const unsigned long long *counters,
                         uint64_t *sum, hipStream_t s);

// VCFX_merger (vcfxg_mg.hip) over the L indexed lines of K files in one text (indexed from offset
// 0); file f's bytes begin at file_start[f] (K + 1 entries, the last one the text's size).
// launch_mg_cut: first_line[f] = the first line that starts at or after file_start[f]
// (first_line[K] = L); first_hash / first_data = L, bad = 0.  launch_mg_key: per line its file and
// status (kMgEmpty, kMgBad, kMgKept; every '#' line kMgHeader for now) and for a kept line POS and
// the key string's start, length and first eight bytes big-endian (CHROM; with natural the bytes
// after the "chr" prefix and the digit run, with pn = (prefix word << 1 | non-numeric) and num = the
// run's value); a lane per line whose second tab lies in its first kMgWindow bytes, then a wave per
// line that pass does not settle (queue: L entries; counters[5] counts them); first_hash[f] /
// first_data[f] = the file's first '#' line / first line that is neither empty nor '#'.
// launch_mg_class: counters[7] = the first file with a header candidate (K: none); the '#' lines
// of that file (with sorted: those before its first_data) stay kMgHeader, every other one becomes
// kMgDropped; written[li] = 1 for a header or kept line; counters[0..4] += the lines per status,
// bad[f] += file f's kMgBad lines, counters[6] = the longest key string of a kept line.
// launch_mg_scatter: vals[ord[line]] = line for every written line (ord: the exclusive scan of
// written).  launch_mg_part: keys[j] = one part (kMgPart*) of the key of line vals[j], 0 for a
// header line.  launch_mg_ordered: counters[8] = 1 when a kept line compares greater than the next
// kept line of its file.  launch_mg_walk_init: the header block to out, state[0] = its lines, cur[f]
// / end[f] = file f's kept lines among the written ones.  launch_mg_walk: at most `steps` steps of
// the K-way heap process from cur and state[0] (one wave).
enum : uint8_t { kMgEmpty = 0, kMgKept = 1, kMgBad = 2, kMgHeader = 3, kMgDropped = 4 };
enum { kMgPartPos = 0, kMgPartLen = 1, kMgPartWord = 2, kMgPartNum = 3, kMgPartPrefix = 4 };
constexpr int kMgWindow = 64;
struct MgLines {
    const char *buf;
    const uint64_t *line_end;
    uint64_t L;
    uint32_t K;
    int sorted, natural;
    uint8_t *status;
    uint32_t *file, *pn;
    uint64_t *w0, *ks, *kl, *num;
    int64_t *pos;
    const uint64_t *file_start;
    uint64_t *first_line, *first_hash, *first_data, *bad, *cur, *end;
};
hipError_t launch_mg_cut(const MgLines &M, hipStream_t s);
hipError_t launch_mg_key(const MgLines &M, uint32_t *queue, unsigned long long *counters, hipStream_t s);
hipError_t launch_mg_class(const MgLines &M, uint32_t *written, unsigned long long *counters, hipStream_t s);
hipError_t launch_mg_scatter(uint64_t L, const uint32_t *written, const uint64_t *ord, uint32_t *vals, hipStream_t s);
hipError_t launch_mg_part(const MgLines &M, uint64_t nw, int part, uint64_t w, uint32_t shift, const uint32_t *vals,
                          uint64_t *keys, hipStream_t s);
hipError_t launch_mg_ordered(const MgLines &M, uint64_t nw, const uint32_t *line, unsigned long long *counters,
                             hipStream_t s);
hipError_t launch_mg_walk_init(const MgLines &M, const uint64_t *ord, const uint32_t *line, uint32_t *out,
                               const unsigned long long *counters, uint64_t *state, hipStream_t s);
hipError_t launch_mg_walk(const MgLines &M, const uint32_t *line, uint32_t *out, uint64_t steps, uint64_t *state,
                          hipStream_t s);

// VCFX_region_subsampler (vcfxg_rs.hip).  The table of n intervals (name id, 1-based start, end) over
// n_chrom names: launch_rs_keys (id << 32 | start, interval) pairs for the stable sort; after it
// launch_rs_table: the sorted ids and starts, reach[j] = the furthest end among the intervals of j's
// name up to j (the running maximum of id << 32 | end: scan_key n entries, tile_max rs_scan_tiles(n)),
// per name its [first, last) in the table (n_chrom entries each, zeroed beforehand), open[j] = 1 where
// a merged interval begins (n + 1 entries, open[n] zeroed beforehand); launch_rs_rows: the merged
// intervals at ord (the exclusive scan of open); launch_rs_dict: name id + 1 into dict (dict_mask + 1
// zeroed slots, at most half of them taken) at its hash masked to hash_bits (1..63), linear probing.
// launch_rs_class over the L indexed lines against the table (an RsTableArgs in device memory: the
// kernels load its fields where they use them): per line its status (kRs*); a lane per line over its first
// kRsWindow bytes, then a wave per line that pass does not settle (queue: L entries; counters[7], zeroed
// beforehand, counts them); counters[8] (L beforehand) = the first line that starts with "#CHROM", the
// data lines before it kRsEarly; counters[0..6] += the lines of each status.
enum : uint8_t { kRsEmpty = 0, kRsHeader = 1, kRsIn = 2, kRsOut = 3, kRsEarly = 4, kRsShort = 5, kRsBadPos = 6 };
constexpr int kRsWindow = 64;
struct RsTableArgs {
    const char *names;
    const uint64_t *name_off;
    const uint32_t *dict, *first, *last;
    const int32_t *start, *reach;
    uint32_t dict_mask;
    uint64_t hash_mask;
};
inline uint64_t rs_hash_mask(uint32_t hash_bits) { return hash_bits && hash_bits < 64u ? (1ull << hash_bits) - 1u : ~0ull; }
uint64_t rs_scan_tiles(uint64_t n);
hipError_t launch_rs_keys(uint64_t n, const uint32_t *id, const int32_t *start, uint64_t *keys, uint32_t *vals, hipStream_t s);
hipError_t launch_rs_table(uint64_t n, const uint64_t *keys, const uint32_t *vals, const int32_t *end, uint32_t *sid,
                           int32_t *sstart, uint64_t *scan_key, uint64_t *tile_max, int32_t *reach, uint32_t *first,
                           uint32_t *last, uint32_t *open, hipStream_t s);
hipError_t launch_rs_rows(uint64_t n, const uint32_t *sid, const int32_t *sstart, const int32_t *reach, const uint32_t *open,
                          const uint64_t *ord, uint32_t *m_id, int32_t *m_start, int32_t *m_end, hipStream_t s);
hipError_t launch_rs_dict(uint32_t n_chrom, const char *names, const uint64_t *name_off, uint32_t hash_bits,
                          uint32_t dict_mask, uint32_t *dict, hipStream_t s);
hipError_t launch_rs_class(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t L, int stdin_mode,
                           const RsTableArgs *table, uint8_t *status, uint32_t *queue, unsigned long long *counters,
                           hipStream_t s);

// VCFX_haplotype_extractor (vcfxg_hx.hip) over the n indexed lines.  launch_hx_scan: per line its status
// (kHx*), POS, member flag, CHROM's length and, for a member, its n_samples cells (GT offset in the line |
// length << 32: kHxCellBytes each) in row `line` of the line-major matrix; a fixed-stride member (FORMAT
// "GT", every sample "a|b") stores none: fixed[line] = its sample region's offset (0 otherwise), cell s
// being (fixed + 4 s, 3); general[line] = a member with a matrix row.  launch_hx_members (mnum: the
// exclusive scan of the flags): member -> line, and per line its member number (~0 off the members, where
// lblock and lflip are ~0 too).  launch_hx_break: start[m] = member m opens a block, flip[m] = the first
// sample that flips against member m - 1 (n_samples: none; examined only under check and when CHROM and
// the signed POS difference let m extend).  launch_hx_blocks (bnum: the exclusive scan of start, nm + 1
// entries): each block's first and last member, block and flip per line.  launch_hx_layout: tiles of
// kHxTileMembers x kHxTileSamples; agg and carry hx_tiles(nm) x n_samples, tstart hx_tiles(nm); base nb x
// n_samples = the exclusive sum along the samples of the block's per-sample widths; head = the bytes of
// "CHROM\tSTART\tEND", row_len = the row with its '\n' (row_len[nb] is the caller's to zero for the scan).
// launch_hx_heads / launch_hx_emit: the rows at row_off (the exclusive scan of row_len) into text.
enum : uint8_t { kHxEmpty = 0, kHxHeader = 1, kHxShort = 2, kHxBadPos = 3, kHxNoGt = 4, kHxUnphased = 5, kHxMember = 6 };
constexpr uint32_t kHxTileMembers = 32;
constexpr uint32_t kHxTileSamples = 64;
constexpr uint32_t kHxCellBytes = 8;
uint64_t hx_tiles(uint64_t nm);
hipError_t launch_hx_scan(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t n, int stdin_mode,
                          uint32_t n_samples, uint8_t *status, int64_t *pos, uint32_t *flag, uint32_t *chrom_len,
                          uint32_t *fixed, uint32_t *general, uint64_t *cells, hipStream_t s);
hipError_t launch_hx_members(uint64_t n, const uint32_t *flag, const uint64_t *mnum, uint64_t *mline, uint64_t *lmember,
                             uint64_t *lblock, uint32_t *lflip, hipStream_t s);
hipError_t launch_hx_break(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t nm, const uint64_t *mline,
                           const int64_t *pos, const uint32_t *chrom_len, const uint32_t *fixed, const uint64_t *cells,
                           uint32_t n_samples, int64_t block_size, int check, uint32_t *start, uint32_t *flip, hipStream_t s);
hipError_t launch_hx_blocks(uint64_t nm, const uint64_t *mline, const uint32_t *start, const uint64_t *bnum,
                            const uint32_t *flip, uint64_t *first, uint64_t *last, uint64_t *lblock, uint32_t *lflip,
                            hipStream_t s);
hipError_t launch_hx_layout(uint64_t nm, uint64_t nb, uint32_t n_samples, const uint64_t *mline, const uint32_t *start,
                            const uint64_t *bnum, const uint32_t *fixed, const uint64_t *cells, const uint64_t *first,
                            const uint64_t *last, const int64_t *pos, const uint32_t *chrom_len, uint64_t *agg, uint32_t *tstart, uint64_t *carry,
                            uint64_t *base, uint32_t *head, uint64_t *row_len, int64_t *bstart, int64_t *bend,
                            hipStream_t s);
hipError_t launch_hx_heads(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t nb, const uint64_t *first,
                           const uint64_t *mline, const uint32_t *chrom_len, const int64_t *bstart, const int64_t *bend,
                           const uint64_t *row_off, const uint64_t *row_len, char *text, hipStream_t s);
hipError_t launch_hx_emit(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t nm, uint32_t n_samples,
                          const uint64_t *mline, const uint32_t *start, const uint64_t *bnum, const uint32_t *fixed,
                          const uint64_t *cells, const uint64_t *carry, const uint64_t *base, const uint32_t *head,
                          const uint64_t *row_off, char *text, hipStream_t s);

// VCFX_field_extractor (vcfxg_fx.hip) over the n indexed lines.  The table is one array of 32-bit words
// in device memory (the kernels take its pointer, never a descriptor by value): kFxHWords header words
// (kFxH*: counts, then the word offsets of the parts), per output column {kind kFx*, standard column},
// per INFO key {pool offset, length, output column}, per distinct sub-field {pool offset, length}, per
// sample cell {output column, line column (0: none), index among the requested columns, sub-field |
// named << 31}, the requested sample columns as nwords + 2 mask words (bit f = column f; two zero words
// behind) and nwords + 1 rank words (set bits before the word), the pool's bytes.  launch_fx_cells: per
// line its status (kFxEmpty / kFxHeader / kFxRow), row flag, row bytes and, for a row, its ncols cells
// {offset, length | kFxDot | kFxOne} in row `line` of the line-major matrix; spans (n x nsc x 2 words)
// and subidx (n x nsub words) are its scratch (all through an FxOut in device memory).  A named cell holds for the lines that start at or after
// names_from.  launch_fx_write: the rows at rowoff (the exclusive scan of the row bytes, n + 1 entries)
// into text (16 B aligned).
enum : uint8_t { kFxEmpty = 0, kFxHeader = 1, kFxRow = 2 };
enum : uint32_t { kFxStd = 0, kFxInfo = 1, kFxSample = 2, kFxNone = 3 };
constexpr uint32_t kFxDot = 0xFFFFFFFFu, kFxOne = 0xFFFFFFFEu;
constexpr uint32_t kFxTableLds = 16384;  // table bytes kept in LDS; larger: global loads
constexpr uint32_t kFxTileRows = 64;     // lines per block of k_fx_write
constexpr uint32_t kFxStage = 8192;      // its LDS stage
enum : uint32_t {
    kFxHNcols = 0, kFxHNkeys, kFxHNsub, kFxHNsamp, kFxHNsc, kFxHLastk, kFxHNwords, kFxHStdin,
    kFxHCols, kFxHKeys, kFxHSubs, kFxHSamp, kFxHMask, kFxHRank, kFxHPool, kFxHTotal, kFxHWords
};
inline bool fx_table_in_lds(uint32_t table_words) { return 4ull * table_words <= kFxTableLds; }
struct FxOut {  // launch_fx_cells' line index and outputs, in device memory (the kernel loads a field where it uses it)
    uint8_t *status;
    uint32_t *isrow;
    uint64_t *rowlen;
    uint32_t *cells, *spans, *subidx;
    uint64_t names_from;
    const uint64_t *line_end;  // the n indexed lines: line i is [line_end[i - 1] + 1, line_end[i]), the first from data_start
    int64_t data_start;
};
hipError_t launch_fx_cells(const char *buf, uint64_t n, const uint32_t *table, uint32_t table_words, const FxOut *out,
                           hipStream_t s);
hipError_t launch_fx_write(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t n, uint32_t ncols,
                           const uint8_t *status, const uint64_t *rowoff, const uint32_t *cells, char *out, hipStream_t s);

// The ordered-text stage of the sorter, the merger and the diff tool (vcfxg_gather.hip).
// launch_line_len: len[j] = the bytes of output line j = indexed line order[j] with its '\n', src[j] =
// its first input byte (len[nw] = 0).  launch_text_gather: output lines [first, first + k) (off: the
// scan of len) as bytes [0, off[first + k] - off[first]) of text (16 B aligned, 16 spare bytes):
// aligned 16 B stores only.  nt: bit 0 non-temporal loads, bit 1 non-temporal stores.
hipError_t launch_line_len(int64_t data_start, const uint64_t *line_end, uint64_t nw, const uint32_t *order, uint64_t *len,
                           uint64_t *src, hipStream_t s);
hipError_t launch_text_gather(const char *buf, const uint64_t *off, const uint64_t *src, uint64_t first, uint64_t k,
                              uint64_t bytes, int nt, char *text, hipStream_t s);

}  // namespace vcfxg
