// vcfxg_af_walk_kernel.h -- the record walk's kernel template (k_af_walk) and its per-reducer
// traits, shared by its instantiations: the AF / HWE / dosage walks of vcfxg_af_walk.hip (which
// describes the walk) and the concordance walk of vcfxg_cc.hip.
#pragma once
#include <algorithm>
#include <type_traits>

#include "vcfxg_device.h"
#include "vcfxg_gt.h"
#include "vcfxg_kernels.h"
#include "vcfxg_walk.h"

namespace vcfxg {

#ifndef VCFXG_WALK_UNROLL
#define VCFXG_WALK_UNROLL 6
#endif
constexpr int kWalkUnroll = VCFXG_WALK_UNROLL;  // wave-steps (KiB) of a record in flight per sweep step
static_assert(kWalkUnroll == kAfDepthDefault, "launch_af_walk's default depth is the batch walks' unroll");
static_assert(kAfWaveStep == kWaveStep, "the host plan's wave-step");
// the HWE walk's sweep: 5 wave-steps (its clean-step genotype classes need the registers of the
// sixth under the 96-VGPR bound; at 6 the record loop spilled)
#ifndef VCFXG_HWE_UNROLL
#define VCFXG_HWE_UNROLL 5
#endif
constexpr int kHweUnroll = VCFXG_HWE_UNROLL;
// the concordance walk's sweep: 4 wave-steps (88 VGPRs; at 5 the sorted keys of the dword path
// spilled 48 B a lane under the 96-VGPR bound)
#ifndef VCFXG_CC_UNROLL
#define VCFXG_CC_UNROLL 4
#endif
constexpr int kCcUnroll = VCFXG_CC_UNROLL;
// the GT-first walk's allele counts on per-byte flags (gt_first_af) rather than gt_first's loop
// over each lane's sample starts (VCFXG_GF_FLAGS=0: the loop, for A/B)
#ifndef VCFXG_GF_FLAGS
#define VCFXG_GF_FLAGS 1
#endif
constexpr bool kGfFlags = VCFXG_GF_FLAGS != 0;
// wave-steps in flight in the GT-first walk's sweeps (its flags take more registers per step)
#ifndef VCFXG_GF_UNROLL
#define VCFXG_GF_UNROLL 4
#endif
constexpr int kGfUnroll = VCFXG_GF_UNROLL;
// VCFXG_AF_XREC=1: the GT-only AF walk carries the next record's first wave-steps across
// records (af_fixed_x).  Measured slower (r04 A/B: af_walk 1.010-1.016 ms at 6 steps, 1.001 at
// 3, against 0.896-0.904 for the default, 112 VGPRs / occupancy 4 against 95 / 5): the
// per-record gap it hides is smaller than the occupancy it costs.  Default 0: each record's
// sweep issues its own first loads after its head's analysis
#ifndef VCFXG_AF_XREC
#define VCFXG_AF_XREC 0
#endif
// VCFXG_AF_EXPT (diagnostic builds only, rows invalid): bit 0 skips the rows' staging, bit 1
// only their frequency text
#ifndef VCFXG_AF_EXPT
#define VCFXG_AF_EXPT 0
#endif
// VCFXG_AF_EARLY=1: the GT-only AF walk issues a record's first sweep batch from its line start
// (16-aligned) before analysing its head, so the batch's latency overlaps the analysis (the
// head bytes ride along and are masked like the bytes before S)
#ifndef VCFXG_AF_EARLY
#define VCFXG_AF_EARLY 0
#endif
#define VCFXG_STR2(x) #x
#define VCFXG_STR(x) VCFXG_STR2(x)

// the walk's per-record reducer: AF allele counts (alt, total) or, for VCFX_hwe_tester, the
// genotype classes (hom-ref, het, hom-alt; the third in aux_o)
template <class Op>
struct WalkRed;
template <>
struct WalkRed<AfOp> {
    static constexpr bool kAux = false;
    __device__ static AfOp make(const char *buf, int64_t ae) { return AfOp{buf, ae, 0}; }
    __device__ static void out(const AfOp &op, uint32_t &a, uint32_t &b, uint32_t &) {
        a = op.alt;
        b = op.tot;
    }
};
template <>
struct WalkRed<HweOp> {
    static constexpr bool kAux = true;
    __device__ static HweOp make(const char *buf, int64_t ae) { return HweOp{buf, ae}; }
    __device__ static void out(const HweOp &op, uint32_t &a, uint32_t &b, uint32_t &c) {
        a = op.c0;
        b = op.c1;
        c = op.c2;
    }
};

// VCFX_cross_sample_concordance: valid samples and distinct keys (alt_o / tot_o); the head gives
// the sweep numAlt and the row rule on CHROM (LineMeta::pad)
template <>
struct WalkRed<CcOp> {
    static constexpr bool kAux = false;
    __device__ static CcOp make(const char *, int64_t) { return CcOp{}; }
    __device__ static void out(const CcOp &op, uint32_t &a, uint32_t &b, uint32_t &) {
        a = op.N;
        b = op.U;
    }
};

template <>
struct WalkRed<DoseWalkOp> {  // samples and "NA" samples of the record (alt_o / tot_o)
    static constexpr bool kAux = false;
    __device__ static DoseWalkOp make(const char *buf, int64_t ae) { return DoseWalkOp{buf, ae}; }
    __device__ static void out(const DoseWalkOp &op, uint32_t &a, uint32_t &b, uint32_t &) {
        a = op.ns;
        b = op.na;
    }
};

template <>
struct WalkRed<DoseHeadOp> : WalkRed<DoseWalkOp> {
    __device__ static DoseHeadOp make(const char *buf, int64_t ae) { return DoseHeadOp{{buf, ae}}; }
};

// kGF: the GT-first walk (records "GT:AD:DP"-like, no fixed stride to predict): a GT-first
// record whose '\n' is past the window is swept by gt_first from its sample start, which finds
// the record's end in the same pass (and issues the next window as soon as it does); a separate
// instantiation, so the GT-only walk keeps its registers
//
// kDepth / kRoll (the AfOp GT-only walk alone; every other walk keeps kWalkUnroll and its batches):
// the wave-steps af_fixed keeps in flight, and whether a record longer than that continues
// rolling, with non-temporal loads (af_fixed's kRoll path).  A record that fits kDepth wave-steps
// is fetched in ONE round trip to HBM; the 6-step batches pay two in sequence on a 10 KB record.
// Measured: the loads' policy is 7-10 % of the walk, the depth 1-2 % on top of it.
// launch_af_walk dispatches over the compiled (kDepth, kRoll); the plan chooses (walk_plan)
#ifndef VCFXG_AF_MINW
#define VCFXG_AF_MINW 5
#endif
// waves per SIMD of an instantiation: the GT-first walk at <= 128 VGPRs (4 waves; it needs 129
// unconstrained, which rounds to 136 and 3 waves); the others at <= 96 (5 waves: the HWE walk
// took 100 without the bound, 4 waves; no spills at 96), but the AF walk's deeper sweeps, whose
// 4 VGPRs a wave-step do not fit 96 without scratch: 4 waves from depth 10
#ifndef VCFXG_AF_DEEP_MINW
#define VCFXG_AF_DEEP_MINW 4
#endif
constexpr int af_walk_waves(bool gf, int depth) { return gf ? 4 : depth >= 10 ? VCFXG_AF_DEEP_MINW : VCFXG_AF_MINW; }
template <class Op, bool kGF = false, int kDepth = kWalkUnroll, bool kRoll = false>
__global__ __launch_bounds__(kWalkThreads)
#ifdef VCFXG_WALK_MAXW
__attribute__((amdgpu_waves_per_eu(1, VCFXG_WALK_MAXW)))
#else
__attribute__((amdgpu_waves_per_eu(af_walk_waves(kGF, kDepth))))
#endif
void k_af_walk(const char *__restrict__ buf, int64_t lo, int64_t hi, WalkLayout lay, int mode, int64_t span0, uint64_t cap_w, uint64_t *__restrict__ le_o, int32_t *__restrict__ alt_o,
               int32_t *__restrict__ tot_o, int32_t *__restrict__ aux_o, uint32_t *__restrict__ rowpre_o,
               uint8_t *__restrict__ status_o, LineMeta *__restrict__ meta_o, uint64_t *__restrict__ wcount,
               uint32_t *__restrict__ wgt, unsigned *overflow, WalkTail tail) {
    typedef WalkRed<Op> R;
    constexpr bool kCc = std::is_same<Op, CcOp>::value;
    static_assert((kDepth == kWalkUnroll && !kRoll) || (std::is_same<Op, AfOp>::value && !kGF),
                  "k_af_walk: a depth of its own for the AF GT-only walk alone");
    static_assert((kDepth == kWalkUnroll && !kRoll) || !(VCFXG_AF_XREC || VCFXG_AF_EARLY),
                  "k_af_walk: the carried / early loads are batch-path experiments at kWalkUnroll");
    __shared__ uint4 win[kWalkWaves][2][kWave];  // two window slots per wave (double buffer)
    // (AfOp) each walker's rows composed in LDS and copied to its global stage once, at the end:
    // stored per record, their completion held up the next record's window wait (r05 ablation:
    // af_walk 0.889 -> 0.839 ms without the per-record stores)
    constexpr bool kStageLds = std::is_same<Op, AfOp>::value;
    constexpr uint32_t kStgCap = kStageLds ? 2048u : 16u;
    __shared__ __attribute__((aligned(16))) char stg[kStageLds ? kWalkWaves : 1][kStgCap];
    const int wv = threadIdx.x / kWave;
    // this walker's bytes [cs, ce) of the layout (vcfxg_walk_layout.h; all wave-uniform)
    int64_t cs, ce, wsize;
    const int64_t wk = walk_range(lay, blockIdx.x, gridDim.x, __builtin_amdgcn_readfirstlane(wv), kWalkWaves, hi,
                                  VCFXG_WALK_XCD != 0, cs, ce, wsize);
    if (wk >= lay.nw) return;
    const int strip_cr = mode == 0 ? 1 : 0;
    int64_t L, ce2;  // this walker's lines start in [L, ce2)
    walker_lines(buf, lo, hi, cs, ce, L, ce2, wsize);
    const int64_t L0 = L;
    uint64_t wtext = 0;  // region tail (tail.wtext): bytes of this walker's GT-line rows
    int64_t span = span0;  // predicted '\n' distance from the sample start
    uint8_t cr_prev = 0;   // and the '\r' state of that record
    uint64_t n = 0;
    uint32_t ngt = 0, ngf = 0;  // GT-first lines; of them, swept whole by gt_first (kGF)
    bool dirty = false;         // AfOp staged rows: some row of this walker is not in its stage
    const uint64_t base = (uint64_t)wk * cap_w;
    // per-line results held by lane (n & 63), written out 64 lines at a time (no stores --
    // and no waits for their completion -- on the per-record path)
    uint64_t r_le = 0, r_S = 0;
    uint32_t r_alt = 0, r_tot = 0, r_aux = 0, r_pre = 0, r_k = 0;  // r_k: kind | sep << 8 | cr << 16 | status << 24
    uint32_t r_h = 0;  // HWE: the CHROM..ALT flags (LineMeta::pad)
    auto flush = [&](uint64_t first, uint32_t cnt) {
        if ((uint32_t)lane() < cnt) {
            const uint64_t o = base + first + lane();
            const uint8_t kind = (uint8_t)r_k;
            LineMeta m{};
            m.kind = kind;
            m.cr = (uint8_t)(r_k >> 16);
            m.pad = (R::kAux || kCc || std::is_same<Op, DoseHeadOp>::value) ? (uint8_t)r_h : 0;
            if (kind == kMetaGt) {
                m.S = r_S;
                m.rowpre = r_pre;
                m.sep = (uint8_t)(r_k >> 8);
            }
            le_o[o] = r_le;
            alt_o[o] = (int32_t)r_alt;
            tot_o[o] = (int32_t)r_tot;
            if (R::kAux) aux_o[o] = (int32_t)r_aux;
            rowpre_o[o] = kind == kMetaGt ? r_pre : 0u;
            status_o[o] = (uint8_t)(r_k >> 24);
            meta_o[o] = m;
        }
    };
    // (AfOp, GT-only walk) the next record's first wave-steps, issued during this record's sweep
    constexpr bool kXrec = VCFXG_AF_XREC && std::is_same<Op, AfOp>::value && !kGF;
    uint4 xv[kXrec ? kWalkUnroll : 1];
    int64_t xvb = -1;  // their base (-1: none)
    int cur = 0;
    int64_t A = L & ~(int64_t)15;  // window base of the current line (L - A < 32)
    if (L < ce2) prefetch_window(buf, A, hi, win[wv][cur]);
    constexpr bool kEarly = VCFXG_AF_EARLY && std::is_same<Op, AfOp>::value && !kGF && !kXrec;
    uint4 ev[kEarly ? kWalkUnroll : 1];
    const int64_t hlast = (hi - 1) & ~(int64_t)15;
    while (L < ce2) {
        if (n >= cap_w) {
            if (lane() == 0) atomicOr(overflow, 1u);
            break;
        }
        if constexpr (kEarly) {  // the first batch from the line start (= the window base A)
#pragma unroll
            for (int u = 0; u < kWalkUnroll; u++) {
                const int64_t g = A + u * kWaveStep + kBlockBytes * lane();
                ev[u] = load16(buf, g < hi ? g : hlast);
            }
        }
        int64_t eA = kEarly ? A : -1;  // the early batch's base (-1: used or none)
        // ---- 1. window analysis (offsets relative to A); a head that does not fit the short
        // window (no '\n' and fewer than 9 tabs in it) gets the 1 KiB window
        const int Lr = (int)(L - A);
        const uint4 *cw = win[wv][cur];
        int hr, N1r, r3 = 0, r4 = 0, r7 = 0, r8 = 0;
        uint32_t ntab, first, hflags = 0;
        // the tab positions -> r4, r7, r8 (and HWE's row rules on CHROM..ALT,
        // VCFX_hwe_tester.cpp:497-506: an ALT with a comma, an empty CHROM / POS / ALT)
        auto take = [&](const int(&rt)[9], bool comma) {
            r4 = rt[4];
            r7 = rt[7];
            r8 = rt[8];
            if (R::kAux) {
                const bool empty = rt[0] == Lr || rt[1] == rt[0] + 1 || r4 == rt[3] + 1;
                hflags = (comma ? kHweAltComma : 0u) | (empty ? kHweEmptyField : 0u);
            }
            if (kCc) {  // (processVariantLine :261: no row for an empty CHROM, file mode)
                r3 = rt[3];
                hflags = rt[0] == Lr ? kCcEmptyChrom : 0u;
            }
        };
        // the kWin window, four bytes per lane (the lane's dword stays in w4 for the byte reads
        // below: a v_readlane each instead of an LDS round trip)
        uint32_t w4 = 0;
        bool long_head = false;
        {
            // the window's LDS-DMA landed (kEarly: all but the early batch, issued after it)
            if constexpr (kEarly) asm volatile("s_waitcnt vmcnt(" VCFXG_STR(VCFXG_WALK_UNROLL) ")" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            w4 = reinterpret_cast<const uint32_t *>(cw)[lane()];
            hr = (int)std::min<int64_t>(hi - A, kWin);
            const uint32_t rg = range4(Lr, hr);
            N1r = first_match<4>(zero_bytes(w4 ^ kRepNl) & rg);
            int rt[9] = {};
            ntab = first_tabs<4>(zero_bytes(w4 ^ kRepTab) & rg, N1r >= 0 ? N1r : hr, rt);
            first = dword_byte(w4, Lr);
            if (ntab >= 9) take(rt, R::kAux && __ballot((zero_bytes(w4 ^ 0x2C2C2C2Cu) & range4(rt[3] + 1, rt[4])) != 0u));
        }
        if (N1r < 0 && ntab < 9 && first != '#' && hr == kWin) {  // (rare) a long head: the 1 KiB window
            prefetch_window(buf, A, hi, win[wv][cur], kWaveStep);
            long_head = true;
            const uint4 W = read_window(cw);
            const int b = 16 * lane();
            hr = (int)std::min<int64_t>(hi - A, kWaveStep);
            N1r = first_match<16>(eq_mask16(W, kRepNl) & range16(b, Lr, hr));
            int rt[9] = {};
            ntab = first_tabs<16>(eq_mask16(W, kRepTab) & range16(b, Lr, hr), N1r >= 0 ? N1r : hr, rt);
            if (ntab >= 9) take(rt, R::kAux && __ballot((eq_mask16(W, 0x2C2C2C2Cu) & range16(b, rt[3] + 1, rt[4])) != 0u));
        }
        // window byte o (wave-uniform, < hr)
        auto wbyte = [&](int o) { return long_head ? slot_byte(cw, o) : dword_byte(w4, o); };
        const int64_t wend = A + hr;
        int64_t t4 = -1, t8 = -1;
        bool gt_head = false, gt_only = false;
        if (ntab >= 9 && first != '#') {
            t4 = A + r4;
            t8 = A + r8;
            if (r8 - r7 >= 3 && wbyte(r7 + 1) == 'G' && wbyte(r7 + 2) == 'T') {
                gt_only = r8 - r7 == 3;
                gt_head = gt_only || wbyte(r7 + 3) == ':';
            }
        }
        // concordance: numAlt of the head's ALT [r3 + 1, r4) (countAltAlleles :170-178), before the
        // next window is issued (it reads the current slot)
        uint32_t cc_max = 0;
        if constexpr (kCc) {
            const int as = r3 + 1;
            if (gt_head && r4 > as && wbyte(as) != '.') {
                cc_max = 1;
                if (r4 - as > 1) {
                    const uint32_t cm = long_head ? eq_mask16(cw[lane()], 0x2C2C2C2Cu) & range16(16 * lane(), as, r4)
                                                  : zero_bytes(w4 ^ 0x2C2C2C2Cu) & range4(as, r4);
                    cc_max += wave_sum32((uint32_t)__popc(cm));
                }
            }
        }
        // ---- 2. line end (and its '\r' in file mode)
        int64_t E;
        uint8_t cr = 0;
        bool predicted = false;
        const bool gf = kGF && N1r < 0 && gt_head && !gt_only;  // the end comes with the sweep
        if (N1r >= 0) {
            E = A + N1r;
            cr = strip_cr && E > L && wbyte(N1r - 1) == '\r';
        } else if (gf) {
            E = hi;  // (until gt_first finds the '\n')
        } else if (gt_only && span > 0 && t8 + 1 + span <= hi) {
            // predicted from the previous fixed-stride record; its end bytes come with the
            // next window (which starts at E - 1) and are checked after the sweep
            E = t8 + 1 + span;
            cr = cr_prev;
            predicted = true;
        } else {
            E = scan_nl(buf, wend, hi);
            cr = strip_cr && E > L && __builtin_amdgcn_readfirstlane(byte_at(buf, E - 1)) == '\r';
        }
        // every read of the current slot happens before the next prefetch is issued (an LDS
        // read after it would make the compiler wait for the LDS-DMA)
        const uint32_t sep_w = gt_head && t8 + 2 < wend ? wbyte((int)(t8 + 2 - A)) : 0u;
        // the next window (the next line's head, and bytes E - 1 and E): issued right after
        // the sweep's first loads (issued before them, the sweep loop's head wait would
        // hold its loads back until the window landed)
        const int nxt = cur ^ 1;
        int64_t An = std::max<int64_t>(E - 1, 0) & ~(int64_t)15;
        bool pending = true;  // the prefetch for An is still to be issued
        auto pre = [&]() {
            prefetch_window(buf, An, hi, win[wv][nxt]);
            pending = false;
        };
        // ---- 3. kind (head_meta) and the sweep
        uint8_t st = 0, kind = 0, sep = 0;
        uint32_t alt = 0, tot = 0, aux = 0, rowpre = 0;
        int64_t S = 0;
        bool ok = false;
        // DoseHeadOp: a predicted GT-only record is not swept (k_dose_fmt checks its bytes)
        bool skip = std::is_same<Op, DoseHeadOp>::value && predicted;
        // the carried wave-steps are this record's only if its sweep is the first af_fixed_x call
        // since they were issued (any other record or a re-sweep drops them)
        int64_t xuse = xvb;
        xvb = -1;
        auto sweep = [&]() {
            if constexpr (kGF) {
              if (gf) {  // gt_first from the sample start: the counts and the record end
                S = t8 + 1;
                Op op = R::make(buf, hi);
                int64_t Eo = hi;
                uint8_t cro = 0;
                auto pre_e = [&](int64_t e) {
                    An = std::max<int64_t>(e - 1, 0) & ~(int64_t)15;
                    pre();
                };
                if constexpr (std::is_same<Op, AfOp>::value && kGfFlags)
                    ok = gt_first_af<kGfUnroll>(buf, S, hi, strip_cr, op, pre_e, Eo, cro);
                else
                    ok = gt_first<kWalkUnroll>(buf, S, hi, strip_cr, op, pre_e, Eo, cro);
                E = Eo;
                cr = cro;
                const int64_t ae = E - cr;
                kind = t8 < ae ? kMetaGt : kMetaFull;
                ok = ok && kind == kMetaGt;
                if (kind == kMetaGt) {
                    rowpre = (uint32_t)(t4 - L + 1);
                    sep = t8 + 2 >= ae ? 0
                          : t8 + 2 < wend ? (uint8_t)sep_w
                                          : (uint8_t)__builtin_amdgcn_readfirstlane(byte_at(buf, t8 + 2));
                    R::out(op, alt, tot, aux);
                }
                return;
              }
            }
            const int64_t ae = E - cr;
            if (ae <= L) kind = kMetaEmpty;
            else if (first == '#') kind = kMetaHeader;
            else if (gt_head && t8 < ae) kind = kMetaGt;
            else kind = kMetaFull;
            ok = false;
            if (kind == kMetaGt) {
                S = t8 + 1;
                rowpre = (uint32_t)(t4 - L + 1);
                sep = t8 + 2 >= ae ? 0
                      : t8 + 2 < wend ? (uint8_t)sep_w
                                      : (uint8_t)__builtin_amdgcn_readfirstlane(byte_at(buf, t8 + 2));
                Op op = R::make(buf, ae);
                if constexpr (kCc) op.max_allele = cc_max;
                if constexpr (kXrec) {
                    const int64_t use = xuse >= 0 && xuse <= S ? xuse : -1;
                    xuse = -1;
                    const int64_t nb = E + 1 < ce2 ? (E + 1) & ~(int64_t)15 : -1;  // this walker's next line
                    int64_t vbo;
                    ok = af_fixed_x<kWalkUnroll>(buf, S, ae, hi, op, sep, pre, xv, use, nb, vbo);
                    xvb = vbo;
                } else if constexpr (kEarly) {
                    // the early batch is this sweep's first when it covers S's block (a re-sweep
                    // after a failed prediction loads its own)
                    const bool mine = eA >= 0 && eA <= S;
                    ok = af_fixed<kWalkUnroll>(buf, S, ae, op, sep, pre, mine ? ev : nullptr, mine ? eA : -1);
                    eA = -1;
                } else if constexpr (std::is_same<Op, AfOp>::value)
                    ok = af_fixed < kGF ? kGfUnroll : kDepth, kRoll > (buf, S, ae, op, sep, pre);
                else if constexpr (std::is_same<Op, DoseHeadOp>::value) {
                    if (skip) {  // samples (ae - S + 1) / 4, none "NA" (checked by k_dose_fmt)
                        ok = (sep == '/' || sep == '|') && ae - S >= 3 && ((ae - S + 1) & 3) == 0;
                        op.ns = ok ? (uint32_t)((ae - S + 1) >> 2) : 0u;
                        op.na = 0;
                    } else {
                        ok = gt_fast<kWalkUnroll>(buf, S, ae, op, sep, pre);
                    }
                } else ok = gt_fast < std::is_same<Op, HweOp>::value ? kHweUnroll : kCc ? kCcUnroll : kWalkUnroll > (buf, S, ae, op, sep, pre);
                R::out(op, alt, tot, aux);
            }
        };
        sweep();
        if (pending) pre();  // (no sweep ran)
        if (predicted) {
            // the prediction holds iff the sweep accepted every byte of [S, ae) and the end
            // bytes are the '\n' (or the input end) and the predicted '\r' state
            const uint4 *nw = win[wv][nxt];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t be = slot_byte(nw, (int)(E - An)), be1 = slot_byte(nw, (int)(E - 1 - An));
            const bool endok = (E < hi ? be == '\n' : true) && ((strip_cr && be1 == '\r') == (cr != 0));
            if (!(ok && endok)) {
                const int64_t Et = scan_nl(buf, wend, hi);
                if (Et != E || !endok) {  // the line again with its true bounds
                    skip = false;
                    E = Et;
                    cr = strip_cr && E > L && __builtin_amdgcn_readfirstlane(byte_at(buf, E - 1)) == '\r';
                    An = std::max<int64_t>(E - 1, 0) & ~(int64_t)15;
                    pending = true;
                    sweep();
                    if (pending) pre();
                }
                // else: true bounds, not fixed-stride
            }
        }
        // DoseHeadOp: a record taken on its predicted end without a sweep (its interior bytes are
        // unread: the consumer checks them, k_dose_fmt / k_ph_lines)
        if constexpr (std::is_same<Op, DoseHeadOp>::value)
            if (skip && kind == kMetaGt) hflags |= kWalkUnswept;
        if (kind == kMetaGt) {
            if (ok) {
                st = 1;
                span = E - S;
                cr_prev = cr;
            } else {
                st = kAfPending;  // not fixed-stride: k_af_complex runs the general sweep
            }
        }
        // ---- 4. results into lane n & 63
        if ((uint32_t)lane() == (uint32_t)(n & 63)) {
            r_le = (uint64_t)E;
            r_S = (uint64_t)S;
            r_alt = alt;
            r_tot = tot;
            r_aux = aux;
            r_h = hflags;
            r_pre = rowpre;
            r_k = (uint32_t)kind | ((uint32_t)sep << 8) | ((uint32_t)cr << 16) | ((uint32_t)st << 24);
        }
        if constexpr (std::is_same<Op, AfOp>::value) {
            // the row's text into the walker's stage (lanes = bytes): CHROM..ALT and its tab from
            // the head window, which still holds the line (the next window went to the other slot),
            // then the frequency; a line left to k_af_cx (or a stage too small) marks the walker
            if (tail.stage && !(VCFXG_AF_EXPT & 1)) {
                if (kind == kMetaGt && ok && wtext + rowpre + 7u <= std::min<uint32_t>(tail.stage_cap, kStgCap)) {
                    uint32_t flo = 0x30303030u, fhi = 0x0A3030u;
                    if (!(VCFXG_AF_EXPT & 2)) af_freq_text(mode, (int32_t)alt, (int32_t)tot, flo, fhi);
                    auto *dst = reinterpret_cast<__attribute__((address_space(3))) char *>(
                                    reinterpret_cast<__attribute__((address_space(3))) char *>(
                                        (__attribute__((address_space(3))) void *)stg[kStageLds ? wv : 0])) +
                                wtext;
                    const unsigned char *src = reinterpret_cast<const unsigned char *>(cw) + (L - A);
                    for (uint32_t j0 = 0; j0 < rowpre + 7u; j0 += kWave) {
                        const uint32_t j = j0 + (uint32_t)lane();
                        if (j < rowpre) dst[j] = (char)src[j];
                        else if (j < rowpre + 7u) {
                            const uint32_t q = j - rowpre;
                            dst[j] = (char)((q < 4u ? flo >> (8u * q) : fhi >> (8u * (q - 4u))) & 0xFFu);
                        }
                    }
                } else if (kind == kMetaGt || kind == kMetaFull) {
                    dirty = true;
                }
            }
        }
        ngt += kind == kMetaGt ? 1u : 0u;
        if constexpr (kGF) ngf += gf && kind == kMetaGt && ok ? 1u : 0u;
        if (tail.wtext) {
            // the row (CHROM..ALT + "\t" + 4 digits... "x.xxxx\n") of a GT line; lines off the
            // fixed-stride sweep go to the leftover list (rare: one atomic each)
            if (kind == kMetaGt) wtext += (uint64_t)rowpre + 7u;
            if (kind == kMetaFull || (kind == kMetaGt && !ok)) {
                if (lane() == 0) {
                    const unsigned long long e = atomicAdd(tail.cx_n, 1ull);
                    if (e < tail.cx_cap) tail.cx_list[e] = base + n;
                }
            }
        }
        n++;
        if ((n & 63) == 0) flush(n - 64, 64);
        L = E + 1;
        A = An;
        cur = nxt;
    }
    if (n & 63) flush(n & ~(uint64_t)63, (uint32_t)(n & 63));
    if constexpr (kStageLds) {
        if (tail.stage && wtext) {  // the walker's rows to its global stage, 16 B stores
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t wt = (uint32_t)std::min<uint64_t>(wtext, kStgCap);
            char *gs = tail.stage + (uint64_t)wk * tail.stage_cap;
            for (uint32_t o = (uint32_t)lane() * 16u; o < wt; o += kWave * 16u)
                *reinterpret_cast<uint4 *>(gs + o) = *reinterpret_cast<const uint4 *>(stg[wv] + o);
        }
    }
    if (lane() == 0) {
        wcount[wk] = n;
        if (tail.wtext) {
            tail.wtext[wk] = wtext;
            tail.wstart[wk] = (uint64_t)L0;
        }
        wgt[wk] = ngt | (ngf << 16);
        if (tail.wdirty) tail.wdirty[wk] = dirty || n >= cap_w ? 1 : 0;
    }
}

}  // namespace vcfxg
