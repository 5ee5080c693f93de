// vcfxg_af_walk.hip -- VCFX_allele_freq_calc's record pass without a separate line index.
//
// The data region is cut into chunks, one wave ("walker") each: C bytes, or, for the AF GT-only
// walk, the plan's two-segment layout (vcfxg_walk_layout.h: full-size walkers in the first dispatch
// rounds, shorter ones last).  A walker's lines are
// those starting in [b(chunk start), b(chunk end)), b(x) the byte after the last '\n' before x
// (vcfxg_walk.h walker_lines: two short backward scans; the line across a chunk boundary goes
// to the walker after it, which reads it first).  It walks its lines one after the other:
//
//   1. one kWin (256 B) window at the line start (4 B per lane, LDS-DMA'd during the previous
//      line's sweep) gives the first '\n' if the line is short, the first 9 tabs and the
//      FORMAT bytes (SWAR masks, one ballot, then scalar code over the matching lanes; a head
//      longer than the window gets a 1 KiB one);
//   2. the line end E: the window's '\n'; or, for a GT-only record (FORMAT == "GT"), the
//      PREDICTED end S + span (span = the '\n' distance from the sample start of the
//      walker's previous fixed-stride record, first the header's 4 * samples - 1), accepted
//      when the byte at E is '\n' (or E is the end of an input without a final '\n'); or
//      else a wave scan for the '\n';
//   3. the fixed-stride sample sweep (vcfxg_gt.h gt_fast, the reference's
//      parseGenotypeAndCount :262-293 on single-digit diploid records) over [S, E).  It
//      validates every byte of [S, E) as a digit, '.', separator or tab, so a predicted
//      end that it accepts has no '\n' before it: the bounds are exact.  If the sweep
//      rejects a predicted line, the '\n' is searched for and the line is re-swept with
//      its true bounds;
//   4. the line's end offset, counts, status and head record go to the walker's region;
//      the next line starts at E + 1 (its window is loaded before this line's sweep).
//
// So every input byte is read from HBM about once (the backward scans' bytes are the next
// walker's first line, read right after them), against twice for the separate index sweep.  k_walk_compact concatenates the regions in file order and
// k_af_complex runs the exact per-line path for everything that is not a fixed-stride
// GT-first record (kMetaFull lines, kAfPending lines), exactly as after the two-sweep
// schedule.  A walker over its line capacity raises `overflow` and the caller reruns the
// two-sweep schedule.  Head semantics follow vcfxg_meta.h head_meta (processMmap :355-470 /
// processStdin :490-556): '\r' stripped in file mode, '#' lines, empty lines, GT-first
// FORMAT, row prefix = CHROM..ALT and its tab.
#include <algorithm>
#include <type_traits>

#include "vcfxg_af_walk_kernel.h"

namespace vcfxg {

// walker regions -> dense per-line arrays in file order (offs = exclusive scan of wcount):
// kCompactSub walker regions per wave at a time, one per group of 64 / kCompactSub lanes (r05: a
// region holds ~13 lines on the 10 KB-record shards, so one region per wave left 51 of 64 lanes
// idle through every round trip), so no slot division and no work for the unused slots; the
// rows / data-line counters (every GT-first record counts as both) are reduced per block (few
// blocks: few atomics)
#ifndef VCFXG_COMPACT_SUB
#define VCFXG_COMPACT_SUB 4
#endif
constexpr int kCompactSub = VCFXG_COMPACT_SUB, kCompactLanes = kWave / kCompactSub;
__global__ __launch_bounds__(256) void k_walk_compact(int64_t n_walkers, uint64_t cap_w,
                                                      const uint64_t *__restrict__ offs,
                                                      const uint32_t *__restrict__ wgt,
                                                      const uint64_t *__restrict__ le_b,
                                                      const int32_t *__restrict__ alt_b,
                                                      const int32_t *__restrict__ tot_b,
                                                      const int32_t *__restrict__ aux_b,
                                                      const uint32_t *__restrict__ rowpre_b,
                                                      const uint8_t *__restrict__ status_b,
                                                      const LineMeta *__restrict__ meta_b, uint64_t *line_end,
                                                      int32_t *alt, int32_t *tot, int32_t *aux, uint32_t *rowpre,
                                                      uint8_t *status, LineMeta *meta, uint64_t *n_lines,
                                                      unsigned long long *counters, const uint64_t *__restrict__ bpre) {
    __shared__ uint32_t red[256 / kWave];
    uint32_t g = 0;
    const int64_t nwaves = (int64_t)gridDim.x * (256 / kWave);
    const int sub = lane() / kCompactLanes, sl = lane() % kCompactLanes;
    for (int64_t w0 = ((int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave) * kCompactSub; w0 < n_walkers;
         w0 += nwaves * kCompactSub) {
        const int64_t w = w0 + sub;
        if (w >= n_walkers) continue;
        // (bpre: block-local offsets of k_walker_scan)
        const uint64_t d0 = offs[w] + (bpre ? bpre[w / kWalkerScanBlock] : 0),
                       cnt = offs[w + 1] + (bpre ? bpre[(w + 1) / kWalkerScanBlock] : 0) - d0, s0 = (uint64_t)w * cap_w;
        g += sl == 0 ? (wgt[w] & 0xFFFFu) : 0u;
        for (uint64_t i = sl; i < cnt; i += kCompactLanes) {
            const uint64_t sl = s0 + i, d = d0 + i;
            line_end[d] = le_b[sl];
            alt[d] = alt_b[sl];
            tot[d] = tot_b[sl];
            if (aux_b) aux[d] = aux_b[sl];
            rowpre[d] = rowpre_b[sl];
            status[d] = status_b[sl];
            meta[d] = meta_b[sl];
        }
    }
    g = wave_sum(g);
    if (lane() == 0) red[threadIdx.x / kWave] = g;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < 256 / kWave; k++) t += red[k];
        if (t) {
            atomicAdd(&counters[0], (unsigned long long)t);
            atomicAdd(&counters[1], (unsigned long long)t);
        }
        if (blockIdx.x == 0) *n_lines = offs[n_walkers] + (bpre ? bpre[n_walkers / kWalkerScanBlock] : 0);
    }
}

int64_t af_walkers(int64_t lo, int64_t hi, int64_t chunk) { return hi > lo ? (hi - lo + chunk - 1) / chunk : 0; }

int af_walk_waves_per_block() { return kWalkWaves; }

// the AF GT-only walk's kernel for (depth, roll); null if not compiled
typedef decltype(&k_af_walk<AfOp>) AfWalkKernel;
static AfWalkKernel af_gt_only_kernel(int depth, bool roll) {
    if (!roll) return depth == kWalkUnroll ? k_af_walk<AfOp> : nullptr;
    return depth == 6 ? k_af_walk<AfOp, false, 6, true>
         : depth == 8 ? k_af_walk<AfOp, false, 8, true>
         : depth == 10 ? k_af_walk<AfOp, false, 10, true>
         : depth == 12 ? k_af_walk<AfOp, false, 12, true>
                       : nullptr;
}

int af_walk_resident_blocks(int depth, bool roll) {
    const AfWalkKernel k = af_gt_only_kernel(depth, roll);
    int blocks = 0;
    if (!k || hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k, kWalkThreads, 0) != hipSuccess) return 0;
    return blocks;
}

hipError_t launch_af_walk(const char *buf, int64_t lo, int64_t hi, const WalkLayout &lay, int mode, int64_t span0,
                          uint64_t cap_w, uint64_t *le_b, int32_t *alt_b, int32_t *tot_b, uint32_t *rowpre_b,
                          uint8_t *status_b, void *meta_b, uint64_t *wcount, uint32_t *wgt, unsigned *overflow,
                          hipStream_t s, int32_t *hwe_aux_b, const WalkTail *tail, bool dose, bool gt_first_walk,
                          bool dose_head, int depth, bool roll) {
    const WalkTail t = tail ? *tail : WalkTail{};
    if (!lay.nw || !lay.grid) return hipErrorInvalidValue;
    // the compiled sweeps: the batches of kWalkUnroll wave-steps for every walk; for the AF GT-only
    // walk also the rolling sweeps of af_depth_compiled
    const bool af_gt_only = !gt_first_walk && !dose && !hwe_aux_b;
    if (roll ? !(af_gt_only && af_depth_compiled(depth)) : depth != kWalkUnroll) return hipErrorInvalidValue;
    // every walk but the AF GT-only one keeps the uniform layout
    if (!af_gt_only && lay.K1 != kWalkAllRounds) return hipErrorInvalidValue;
    auto go = [&](auto kernel, int32_t *aux_b) {
        hipLaunchKernelGGL(kernel, dim3(lay.grid), dim3(kWalkThreads), 0, s, buf, lo, hi, lay, mode, span0, cap_w, le_b,
                           alt_b, tot_b, aux_b, rowpre_b, status_b, static_cast<LineMeta *>(meta_b), wcount, wgt,
                           overflow, t);
    };
    if (gt_first_walk) go(k_af_walk<AfOp, true>, nullptr);
    else if (dose && dose_head) go(k_af_walk<DoseHeadOp>, nullptr);
    else if (dose) go(k_af_walk<DoseWalkOp>, nullptr);
    else if (hwe_aux_b) go(k_af_walk<HweOp>, hwe_aux_b);
    else go(af_gt_only_kernel(depth, roll), nullptr);  // (compiled: checked above)
    return hipGetLastError();
}

hipError_t launch_walk_compact(int64_t n_walkers, uint64_t cap_w, const uint64_t *offs, const uint32_t *wgt,
                               const uint64_t *le_b, const int32_t *alt_b, const int32_t *tot_b,
                               const uint32_t *rowpre_b, const uint8_t *status_b, const void *meta_b,
                               uint64_t *line_end, int32_t *alt, int32_t *tot, uint32_t *rowpre, uint8_t *status,
                               void *meta, uint64_t *n_lines, unsigned long long *counters, hipStream_t s,
                               const int32_t *aux_b, int32_t *aux, const uint64_t *bpre) {
    const int64_t blocks = std::min<int64_t>((n_walkers + 256 / kWave - 1) / (256 / kWave), 512);
    hipLaunchKernelGGL(k_walk_compact, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), 0, s, n_walkers, cap_w,
                       offs, wgt, le_b, alt_b, tot_b, aux_b, rowpre_b, status_b, static_cast<const LineMeta *>(meta_b),
                       line_end, alt, tot, aux, rowpre, status, static_cast<LineMeta *>(meta), n_lines, counters, bpre);
    return hipGetLastError();
}

}  // namespace vcfxg
