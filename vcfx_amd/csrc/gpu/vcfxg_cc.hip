// vcfxg_cc.hip -- VCFX_cross_sample_concordance's per-record pass: how many distinct
// (normalised) genotypes the selected samples of a record carry.
//
// Long fixed-stride records are counted on the record walk (vcfxg_af_walk.hip with CcOp,
// vcfxg_gt.h: a 55-bit key set and a count per lane, reduced over the wave) in the one HBM pass
// that also finds the lines; k_cc_lines then takes the lines the walk left, or every line on the
// schedule for short records.  It gives a wave to a line.  The wave finds the first five fields (CHROM..ALT, the
// row's prefix and numAlt), then sweeps the line 1 KiB a step: every lane numbers the tabs of
// its 16 bytes, and the field after a tab whose column is selected is parsed by that lane as
// parseGenotypeToId does (VCFX_cross_sample_concordance.cpp:130-167), multi-digit alleles
// included.  A valid key (a1 <= a2 <= 127) sets its bit in the wave's LDS bitset over all
// 128 x 128 keys; the lane whose atomic OR finds the bit clear counts a distinct key.  The
// wave sums the valid calls (weighted by the column's multiplicity) and the distinct keys.
// k_cc_chrom lists the "#CHROM" lines for the host.  k_cc_rowlen maps a data line to its place
// in the output (the reference's per-thread blocks in file mode) and stores the row's length
// there, a scan gives the offsets, and k_cc_format writes every row at its final place.
#include "vcfx_gpu.h"
#include "vcfxg_af_walk_kernel.h"

namespace vcfxg {

constexpr int kCcThreads = 256;
constexpr int kCcWaves = kCcThreads / kWave;
constexpr int kCcSetWords = 128 * 128 / 32;  // one bit per key (a1 << 7) | a2
constexpr uint32_t kCcInvalid = ~0u, kCcEnd = 0x100u;

// parseGenotypeToId (:130-167) on the field that starts at p: its GT ends at the first ':' or
// '\t' or at ae.  The key (lo << 7) | hi of the sorted alleles, or kCcInvalid.  (A digit run
// that overflows int is undefined in the reference; here it saturates, which is invalid.)
__device__ __forceinline__ uint32_t cc_parse(const char *__restrict__ buf, int64_t p, int64_t ae, uint32_t max_allele) {
    auto at = [&](int64_t q) -> uint32_t {
        if (q >= ae) return kCcEnd;
        const uint32_t c = byte_at(buf, q);
        return c == ':' || c == '\t' ? kCcEnd : c;
    };
    uint32_t c = at(p);
    if (c == kCcEnd || c == '.') return kCcInvalid;
    uint32_t a1 = 0, a2 = 0;
    while (c - '0' < 10u) {
        a1 = a1 * 10u + (c - '0');
        if (a1 > 1000u) a1 = 1000u;
        c = at(++p);
    }
    if (c != '/' && c != '|') return kCcInvalid;
    c = at(++p);
    if (c == kCcEnd || c == '.') return kCcInvalid;
    while (c - '0' < 10u) {
        a2 = a2 * 10u + (c - '0');
        if (a2 > 1000u) a2 = 1000u;
        c = at(++p);
    }
    if (a1 > max_allele || a2 > max_allele || a1 > 127u || a2 > 127u) return kCcInvalid;
    const uint32_t lo = a1 < a2 ? a1 : a2, hi = a1 < a2 ? a2 : a1;
    return (lo << 7) | hi;
}

// One line [ls, le).  data = the line counts among the collected data lines (non-empty after
// the file mode's '\r' strip, not a '#' line); st = 0 no row, else kCc*.  File mode
// (processVariantLine :229-319): fields as the tab loop makes them (a trailing tab opens no
// field), >= 5 of them and a non-empty CHROM, selected columns past the line skipped.  Stdin
// mode (:649-716): no '\r' strip, split_tabs fields, >= max(8, 9 + ns) of them.
__device__ __forceinline__ void cc_line(const char *__restrict__ buf, int64_t ls, int64_t le, int mode, uint32_t ns,
                                        const uint32_t *__restrict__ mult, uint32_t n_mult, int64_t *lds,
                                        uint32_t *set, bool &data, uint8_t &st, uint32_t &N, uint32_t &U,
                                        uint32_t &rowpre) {
    data = false;
    st = 0;
    N = U = rowpre = 0;
    int64_t ae = le;
    if (mode == VCFXG_MODE_FILE && ae > ls && byte_at(buf, ae - 1) == '\r') ae--;
    if (ae <= ls || byte_at(buf, ls) == '#') return;
    data = true;
    int64_t t[5];
    const int nt5 = head_tabs(buf, ls, ae, 5, t, lds);
    if (nt5 < 4) return;  // fewer than 5 fields in either mode
    if (mode == VCFXG_MODE_FILE) {
        if (nt5 == 4 && t[3] + 1 >= ae) return;  // "a\tb\tc\td\t": four fields
        if (t[0] == ls) return;                  // empty CHROM
    }
    const int64_t alt_s = t[3] + 1, alt_e = nt5 >= 5 ? t[4] : ae;
    // countAltAlleles :170-178
    uint32_t max_allele = 0;
    if (alt_e > alt_s && byte_at(buf, alt_s) != '.') {
        max_allele = 1;
        for (int64_t w = alt_s; w < alt_e; w += kWave) {
            const int64_t p = w + lane();
            max_allele += (uint32_t)__popcll(__ballot(p < alt_e && byte_at(buf, p) == ','));
        }
    }
    uint32_t n_valid = 0, n_new = 0, tabs = 0;
    for (int64_t w = ls & ~(int64_t)15; w < ae; w += kWaveStep) {
        const int64_t blk = w + (int64_t)lane() * kBlockBytes;
        uint32_t m = 0;
        if (blk < ae) m = eq_mask16(load16(buf, blk), kRepTab) & range_mask16(blk, ls, ae);
        const uint32_t c = (uint32_t)__popc(m);
        const uint32_t incl = wave_incl_scan(c);
        uint32_t k = tabs + incl - c;  // the number of this lane's first tab
        tabs += wave_bcast(incl, kWave - 1);
        while (m) {
            const int j = __builtin_ctz(m);
            m &= m - 1u;
            const uint32_t col = k + 1;  // the field that starts after tab k
            k++;
            if (col < 9) continue;
            const uint32_t s = col - 9;
            const uint32_t mu = mult ? (s < n_mult ? mult[s] : 0u) : (s < ns ? 1u : 0u);
            if (!mu) continue;
            const uint32_t key = cc_parse(buf, blk + j + 1, ae, max_allele);
            if (key == kCcInvalid) continue;
            n_valid += mu;
            const uint32_t bit = 1u << (key & 31u);
            if (!(atomicOr(&set[key >> 5], bit) & bit)) n_new++;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int k = lane(); k < kCcSetWords; k += kWave) set[k] = 0u;  // the set is empty for the next line
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (mode == VCFXG_MODE_STDIN) {
        const uint32_t need = ns + 9u > 8u ? ns + 9u : 8u;
        if (tabs + 1u < need) return;
    }
    N = wave_sum(n_valid);
    U = wave_sum(n_new);
    st = N == 0 ? kCcNoGt : (U == 1 ? kCcSame : kCcDiff);
    rowpre = (uint32_t)(alt_e - ls);
}

// A wave takes 64 lines a step, a lane each for the triage, then the wave runs cc_line on those
// that need it, one after the other.  meta == nullptr: every line (the schedule for short
// records).  Else the lines the walk left: kMetaFull lines, kMetaGt lines its fixed-stride sweep
// refused (kAfPending) or whose sample count is not ns (the sweep counts every sample once: right
// only when exactly the header's columns are there, each selected once); the walk's other kMetaGt
// lines keep its N and U (n_o / u_o) and get their status here, '#' and empty lines none.
// counters: [0] concordant, [1] discordant, [2] no-genotype rows, [3] lines cc_line took
__global__ __launch_bounds__(kCcThreads) void k_cc_lines(const char *__restrict__ buf, int64_t data_start,
                                                         const uint64_t *__restrict__ line_end,
                                                         const uint64_t *n_lines_p, int mode, uint32_t ns,
                                                         const uint32_t *__restrict__ mult, uint32_t n_mult,
                                                         const LineMeta *__restrict__ meta, int32_t *__restrict__ n_o,
                                                         int32_t *__restrict__ u_o, uint32_t *__restrict__ rowpre_o,
                                                         uint8_t *__restrict__ status_o, uint32_t *__restrict__ isdata_o,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ int64_t scratch[kCcWaves][16];
    __shared__ uint32_t sets[kCcWaves][kCcSetWords];
    const int wv = threadIdx.x / kWave;
    int64_t *lds = scratch[wv];
    uint32_t *set = sets[wv];
    for (int k = lane(); k < kCcSetWords; k += kWave) set[k] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint64_t n_lines = *n_lines_p;
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    uint32_t cnt[4] = {0, 0, 0, 0};  // (per lane for the walk's lines, lane 0's for cc_line's)
    for (uint64_t l0 = wid * kWave; l0 < n_lines; l0 += nw * kWave) {
        const uint64_t mine = l0 + lane();
        bool todo_me = mine < n_lines;
        if (meta && todo_me) {
            const LineMeta m = meta[mine];
            const uint8_t ws = status_o[mine];
            if (m.kind == kMetaEmpty || m.kind == kMetaHeader) {
                todo_me = false;
                status_o[mine] = 0;
                isdata_o[mine] = 0u;
            } else if (m.kind == kMetaGt && ws == 1) {
                const int64_t ae = (int64_t)line_end[mine] - m.cr;
                if ((uint64_t)(ae - (int64_t)m.S + 1) == 4ull * ns) {
                    todo_me = false;
                    uint8_t st = 0;
                    if (!(mode == VCFXG_MODE_FILE && (m.pad & kCcEmptyChrom))) {
                        const uint32_t N = (uint32_t)n_o[mine], U = (uint32_t)u_o[mine];
                        st = N == 0 ? kCcNoGt : (U == 1 ? kCcSame : kCcDiff);
                        cnt[0] += st == kCcSame;
                        cnt[1] += st == kCcDiff;
                        cnt[2] += st == kCcNoGt;
                    }
                    status_o[mine] = st;
                    rowpre_o[mine] = m.rowpre - 1u;  // (without ALT's tab)
                    isdata_o[mine] = 1u;
                }
            }
        }
        uint64_t todo = __ballot(todo_me);
        while (todo) {
            const int k = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint64_t li = l0 + k;
            const int64_t ls = li ? (int64_t)line_end[li - 1] + 1 : data_start, le = (int64_t)line_end[li];
            bool data;
            uint8_t st;
            uint32_t N, U, rp;
            cc_line(buf, ls, le, mode, ns, mult, n_mult, lds, set, data, st, N, U, rp);
            if (lane() == 0) {
                cnt[0] += st == kCcSame;
                cnt[1] += st == kCcDiff;
                cnt[2] += st == kCcNoGt;
                cnt[3] += data ? 1u : 0u;
                status_o[li] = st;
                n_o[li] = (int32_t)N;
                u_o[li] = (int32_t)U;
                rowpre_o[li] = rp;
                isdata_o[li] = data ? 1u : 0u;
            }
        }
    }
    // one atomic per counter and block (same-address atomics serialise in L2)
    __shared__ uint32_t red[kCcWaves][4];
    for (int k = 0; k < 4; k++) {
        const uint32_t t = wave_sum(cnt[k]);
        if (lane() == 0) red[wv][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t t = 0;
        for (int k = 0; k < kCcWaves; k++) t += red[k][threadIdx.x];
        if (t) atomicAdd(&counters[threadIdx.x], (unsigned long long)t);
    }
}

// the start offsets of the lines that begin with "#CHROM" (any order; *n counts them all)
__global__ void k_cc_chrom(const char *__restrict__ buf, int64_t data_start, const uint64_t *__restrict__ line_end,
                           const uint64_t *n_lines_p, uint64_t *__restrict__ out, uint64_t cap, unsigned long long *n) {
    const uint64_t n_lines = *n_lines_p;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_lines;
         i += gridDim.x * (uint64_t)blockDim.x) {
        const int64_t ls = i ? (int64_t)line_end[i - 1] + 1 : data_start, le = (int64_t)line_end[i];
        if (le - ls < 6 || buf[ls] != '#' || buf[ls + 1] != 'C' || buf[ls + 2] != 'H' || buf[ls + 3] != 'R' ||
            buf[ls + 4] != 'O' || buf[ls + 5] != 'M')
            continue;
        const unsigned long long k = atomicAdd(n, 1ull);
        if (k < cap) out[k] = (uint64_t)ls;
    }
}

__device__ __forceinline__ uint32_t dec_digits(uint32_t v) {
    uint32_t d = 1;
    while (v >= 10u) {
        v /= 10u;
        d++;
    }
    return d;
}

// The output place of data line number o of n (:498-499, :521, :579-581): T workers, clamped to
// [1, n]; worker t takes lines t, t + T, ... and the workers' rows follow one another.  Workers
// below n % T hold one line more.  T == 0: record order.
__device__ __forceinline__ uint64_t cc_rank(uint64_t o, uint64_t n, uint64_t T) {
    if (!T) return o;
    const uint64_t Te = T < n ? T : n, q = n / Te, r = n % Te, t = o % Te;
    return t * q + (t < r ? t : r) + o / Te;
}

// len[rank of line i] = its row's bytes (0: no row); ord = the exclusive scan of isdata
// (n_lines + 1 entries); len was zeroed
__global__ void k_cc_rowlen(const uint64_t *n_lines_p, uint64_t T, const uint64_t *__restrict__ ord,
                            const uint32_t *__restrict__ isdata, const uint8_t *__restrict__ status,
                            const int32_t *__restrict__ nn, const int32_t *__restrict__ uu,
                            const uint32_t *__restrict__ rowpre, uint64_t *__restrict__ len) {
    const uint64_t n_lines = *n_lines_p;
    const uint64_t nd = ord[n_lines];
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_lines;
         i += gridDim.x * (uint64_t)blockDim.x) {
        if (!isdata[i]) continue;
        uint64_t l = 0;
        const uint8_t st = status[i];
        // "\t<N>\t<U>\t" + CONCORDANT / DISCORDANT (10) or NO_GENOTYPES (12) + '\n'
        if (st == kCcNoGt) l = (uint64_t)rowpre[i] + 3u + 2u + 12u + 1u;
        else if (st) l = (uint64_t)rowpre[i] + 3u + dec_digits((uint32_t)nn[i]) + dec_digits((uint32_t)uu[i]) + 10u + 1u;
        len[cc_rank(ord[i], nd, T)] = l;
    }
}

// out[0] = data lines, [1] = text bytes, [2..5] = counters[0..3], [6] = lines, [7] = the walk's
// overflow flag
__global__ void k_cc_summary(const uint64_t *n_lines_p, const uint64_t *__restrict__ ord,
                             const uint64_t *__restrict__ off, const unsigned long long *__restrict__ counters,
                             const unsigned *fail, uint64_t *__restrict__ out) {
    const uint64_t n_lines = *n_lines_p, nd = ord[n_lines];
    out[0] = nd;
    out[1] = off[nd];
    for (int k = 0; k < 4; k++) out[2 + k] = counters[k];
    out[6] = n_lines;
    out[7] = fail ? *fail : 0u;
}

__device__ __forceinline__ char *put_dec(char *o, uint32_t v) {
    const uint32_t d = dec_digits(v);
    for (uint32_t k = d; k-- > 0;) {
        o[k] = (char)('0' + v % 10u);
        v /= 10u;
    }
    return o + d;
}

// one thread per line: its row at off[rank]
__global__ void k_cc_format(const char *__restrict__ buf, int64_t data_start, const uint64_t *__restrict__ line_end,
                            const uint64_t *n_lines_p, uint64_t T, const uint64_t *__restrict__ ord,
                            const uint8_t *__restrict__ status, const int32_t *__restrict__ nn,
                            const int32_t *__restrict__ uu, const uint32_t *__restrict__ rowpre,
                            const uint64_t *__restrict__ off, char *__restrict__ out, uint64_t cap) {
    const uint64_t n_lines = *n_lines_p;
    const uint64_t nd = ord[n_lines];
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_lines;
         i += gridDim.x * (uint64_t)blockDim.x) {
        const uint8_t st = status[i];
        if (!st) continue;
        const int64_t ls = i ? (int64_t)line_end[i - 1] + 1 : data_start;
        const uint64_t rk = cc_rank(ord[i], nd, T);
        if (off[rk + 1] > cap) continue;  // (past the text capacity: formatted again once it has grown)
        char *o = out + off[rk];
        const uint32_t pl = rowpre[i];
        for (uint32_t k = 0; k < pl; k++) o[k] = buf[ls + k];
        o += pl;
        *o++ = '\t';
        o = put_dec(o, st == kCcNoGt ? 0u : (uint32_t)nn[i]);
        *o++ = '\t';
        o = put_dec(o, st == kCcNoGt ? 0u : (uint32_t)uu[i]);
        *o++ = '\t';
        const char *w = st == kCcSame ? "CONCORDANT" : (st == kCcDiff ? "DISCORDANT" : "NO_GENOTYPES");
        while (*w) *o++ = *w++;
        *o = '\n';
    }
}

static unsigned cc_grid(uint64_t n, uint64_t per, unsigned cap) {
    uint64_t g = (n + per - 1) / per;
    if (g < 1) g = 1;
    return (unsigned)(g > cap ? cap : g);
}

hipError_t launch_cc_walk(const char *buf, int64_t lo, int64_t hi, const WalkLayout &lay, int mode, int64_t span0,
                          uint64_t cap_w, uint64_t *le_b, int32_t *alt_b, int32_t *tot_b, uint32_t *rowpre_b,
                          uint8_t *status_b, void *meta_b, uint64_t *wcount, uint32_t *wgt, unsigned *overflow,
                          hipStream_t s) {
    if (!lay.nw || !lay.grid || lay.K1 != kWalkAllRounds) return hipErrorInvalidValue;  // (the uniform layout)
    hipLaunchKernelGGL(k_af_walk<CcOp>, dim3(lay.grid), dim3(kWalkThreads), 0, s, buf, lo, hi, lay, mode, span0, cap_w,
                       le_b, alt_b, tot_b, nullptr, rowpre_b, status_b, static_cast<LineMeta *>(meta_b), wcount, wgt,
                       overflow, WalkTail{});
    return hipGetLastError();
}

hipError_t launch_cc_lines(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                           uint64_t n_lines_host, int mode, uint32_t ns, const uint32_t *mult, uint32_t n_mult,
                           const void *meta, int32_t *n_o, int32_t *u_o, uint32_t *rowpre, uint8_t *status,
                           uint32_t *isdata, unsigned long long *counters, hipStream_t s) {
    if (!n_lines_host) return hipSuccess;
    // a wave takes 64 lines a step: after the walk the triage alone for nearly all of them
    const unsigned grid = cc_grid((n_lines_host + kWave - 1) / kWave, kCcWaves, meta ? 1024 : 8192);
    hipLaunchKernelGGL(k_cc_lines, dim3(grid), dim3(kCcThreads), 0, s, buf, data_start, line_end, n_lines_dev, mode, ns,
                       mult, n_mult, static_cast<const LineMeta *>(meta), n_o, u_o, rowpre, status, isdata, counters);
    return hipGetLastError();
}

hipError_t launch_cc_chrom(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                           uint64_t n_lines_host, uint64_t *out, uint64_t cap, unsigned long long *n, hipStream_t s) {
    if (!n_lines_host) return hipSuccess;
    hipLaunchKernelGGL(k_cc_chrom, dim3(cc_grid(n_lines_host, 256, 1024)), dim3(256), 0, s, buf, data_start, line_end,
                       n_lines_dev, out, cap, n);
    return hipGetLastError();
}

hipError_t launch_cc_rowlen(const uint64_t *n_lines_dev, uint64_t n_lines_host, uint64_t T, const uint64_t *ord,
                            const uint32_t *isdata, const uint8_t *status, const int32_t *nn, const int32_t *uu,
                            const uint32_t *rowpre, uint64_t *len, hipStream_t s) {
    if (!n_lines_host) return hipSuccess;
    hipLaunchKernelGGL(k_cc_rowlen, dim3(cc_grid(n_lines_host, 256, 1024)), dim3(256), 0, s, n_lines_dev, T, ord, isdata,
                       status, nn, uu, rowpre, len);
    return hipGetLastError();
}

hipError_t launch_cc_summary(const uint64_t *n_lines_dev, const uint64_t *ord, const uint64_t *off,
                             const unsigned long long *counters, const unsigned *fail, uint64_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_cc_summary, dim3(1), dim3(1), 0, s, n_lines_dev, ord, off, counters, fail, out);
    return hipGetLastError();
}

hipError_t launch_cc_format(const char *buf, int64_t data_start, const uint64_t *line_end, const uint64_t *n_lines_dev,
                            uint64_t n_lines_host, uint64_t T, const uint64_t *ord, const uint8_t *status,
                            const int32_t *nn, const int32_t *uu, const uint32_t *rowpre, const uint64_t *off, char *out,
                            uint64_t text_cap, hipStream_t s) {
    if (!n_lines_host) return hipSuccess;
    hipLaunchKernelGGL(k_cc_format, dim3(cc_grid(n_lines_host, 256, 4096)), dim3(256), 0, s, buf, data_start, line_end,
                       n_lines_dev, T, ord, status, nn, uu, rowpre, off, out, text_cap);
    return hipGetLastError();
}

}  // namespace vcfxg
