// vcfxg_fa.hip -- VCFX_fasta_converter (VCFX_fasta_converter.cpp: convertVCFtoFastaStreaming
// :291-424, convertVCFtoFasta :433-523, parseGenotype :198-224, parseAlleleBase :180-196): every
// sample's base at every variant as one IUPAC letter, written sample by sample in lines of 60.
// The first kernels here whose output is the input turned on its side: the records are the
// columns of the text, the samples its rows.
//
// Byte model.  A column is a line the mode counts as a variant (file: every line that does not
// start with '#', the empty ones too; stdin: a non-empty line of at least 9 + n_samples fields).
// Column g (counted over the whole input) of sample s is byte
//     row_off[s] + c + c / 60,   c = g - skip[s]
// of the text, followed by '\n' when c % 60 = 59 or c is the row's last column; skip[s] is the
// columns that came before the sample's "#CHROM" line (stdin mode, repeated headers).  A sample
// the line has no field for is the byte 0 (the reference's zero-initialised matrix shows through).
//
// Passes (vcfxg_api_fa.hip):
//   k_fa_scan       a wave per line: status, the sample region, the GT key's index, the REF base
//                   and the bases of ALT alleles 1..15 (FaMeta), the column flag
//   (scan)          hipcub exclusive sum of the flags: each line's column number
//   k_fa_bases      a wave per column line: its n_samples bases, contiguous, into the record-major
//                   matrix (row = column number, pitch = n_samples rounded up to 16).  Fixed-stride
//                   GT-only records through gt_fast, everything else a lane per sample start with
//                   the reference's parse; allele numbers >= 16 walk the ALT text
//   k_fa_transpose  tiles of 64 samples x 240 columns through LDS: read along samples (a wave per
//                   column, a lane per sample), written along columns (a wave per sample).  A tile
//                   that starts on a multiple of 60 with no skip is laid out in LDS as the text it
//                   becomes ('\n' after every 60 bases) and copied out a dword a lane; any other
//                   tile places each byte by the model above
// LDS: the tile's rows are 244 bytes apart (61 dwords: odd), so the 64 lanes of a column write --
// lane s at 61 s dwords + the column -- fall in 32 different banks per half-wave, and the lanes of
// a row read consecutive bytes.
// Outside the domain (as the reference's int): an allele index of more than 9 digits; and a line
// of 2 GiB or more (offsets within a line are 32-bit).
#include <algorithm>

#include "vcfxg_gt.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kFaThreads = 256;
constexpr int kFaWaves = kFaThreads / kWave;
constexpr int kFaRow = kFaTileCols + kFaTileCols / kFaLine;  // a tile row as text: 244 bytes

static_assert(kFaTileSamples == kWave, "a lane per sample of the tile");
static_assert(kFaTileCols % kFaLine == 0 && (kFaRow / 4) % 2 == 1 && kFaRow % 4 == 0, "tile rows: whole lines, odd dwords");
static_assert(kFaRow <= 4 * kWave - 4, "a row is stored by one wave, a dword a lane");

__device__ __forceinline__ void fa_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// parseAlleleBase :180-196 for allele >= 1 over ALT b[as, ae)
__device__ __forceinline__ uint32_t fa_allele_base(const char *__restrict__ b, int32_t as, int32_t ae, uint32_t allele) {
    uint32_t idx = 1;
    int32_t p = as;
    while (p < ae && idx < allele) {
        if (byte_at(b, p) == ',') idx++;
        p++;
    }
    if (idx != allele || p >= ae) return 'N';
    const int32_t s = p;
    while (p < ae && byte_at(b, p) != ',') p++;
    if (p - s != 1) return 'N';
    const uint32_t c = byte_at(b, s);
    return c - 'A' < 26u ? c : c - 'a' < 26u ? c - 32u : (uint32_t)'N';
}

// the table of FaMeta as two 64-bit values (wave-uniform): entry a < 16 by shifts and masks alone
// (a select among the words made the compiler keep the table in memory and index it)
struct FaTab {
    uint64_t lo, hi;
    __device__ __forceinline__ uint32_t at(uint32_t a) const {
        const uint32_t sh = 8u * (a & 7u), m = a < 8u ? 0xFFu : 0u;
        return ((uint32_t)(lo >> sh) & m) | ((uint32_t)(hi >> sh) & (m ^ 0xFFu));
    }
};

__device__ __forceinline__ int fa_base_idx(uint32_t c) {
    c &= ~0x20u;  // (baseIdx :127-135 takes both cases)
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}

// parseGenotype's tail :220-223: the two alleles' bases combined
__device__ __forceinline__ uint32_t fa_combine(uint32_t b1, uint32_t b2) {
    if (b1 == 'N' || b2 == 'N') return 'N';
    if (b1 == b2) return b1;
    const int i1 = fa_base_idx(b1), i2 = fa_base_idx(b2);
    if (i1 < 0 || i2 < 0) return 'N';
    // IUPAC[16] = "AMRWMCSYRSGKWYKT" :125, eight letters a word
    const uint64_t lo = 0x5953434D57524D41ull, hi = 0x544B59574B475352ull;
    const uint32_t k = (uint32_t)(i1 * 4 + i2);
    return (uint32_t)(((k < 8u ? lo : hi) >> (8u * (k & 7u))) & 0xFFu);
}

struct FaLine {
    const char *b;  // the line's first byte
    int32_t alt_s, alt_e, gi;
    FaTab T;
    __device__ __forceinline__ uint32_t allele(uint32_t a) const {
        return a < kFaTable ? T.at(a) : fa_allele_base(b, alt_s, alt_e, a);
    }
};

// parseGenotype :198-224 over extractGT :171-178 for the sample that starts at st (region end E)
__device__ __forceinline__ uint32_t fa_sample(const FaLine &L, int32_t st, int32_t E) {
    const char *__restrict__ b = L.b;
    if (L.gi < 0) return 'N';
    int32_t se = st;
    while (se < E && byte_at(b, se) != '\t') se++;
    int32_t p = st;
    for (int32_t i = 0; i < L.gi && p < se; i++) {
        while (p < se && byte_at(b, p) != ':') p++;
        if (p < se) p++;
    }
    if (p >= se || byte_at(b, p) == '.') return 'N';
    uint32_t a1 = 0, a2 = 0;
    while (p < se && byte_at(b, p) - '0' < 10u) {
        a1 = a1 * 10u + (byte_at(b, p) - '0');
        p++;
    }
    if (p >= se || (byte_at(b, p) != '/' && byte_at(b, p) != '|')) return 'N';
    p++;
    if (p >= se || byte_at(b, p) == '.') return 'N';
    while (p < se && byte_at(b, p) - '0' < 10u) {
        a2 = a2 * 10u + (byte_at(b, p) - '0');
        p++;
    }
    return fa_combine(L.allele(a1), L.allele(a2));
}

// ---- scan -----------------------------------------------------------------------------------------

// per line li = l0 + i: status[li]; flag[i] = it is a column; meta[i] (column lines)
__global__ __launch_bounds__(kFaThreads) void k_fa_scan(const char *__restrict__ buf, int64_t data_start,
                                                        const uint64_t *__restrict__ line_end, uint64_t l0, uint64_t n,
                                                        int stdin_mode, uint32_t n_samples, uint8_t *__restrict__ status,
                                                        uint32_t *__restrict__ flag, FaMeta *__restrict__ meta,
                                                        unsigned long long *__restrict__ counters) {
    __shared__ uint32_t s_t[kFaWaves][12];
    uint32_t *t = s_t[threadIdx.x / kWave];
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t i = wid; i < n; i += nw) {
        const uint64_t li = l0 + i;
        const int64_t ls = li ? (int64_t)line_end[li - 1] + 1 : data_start;
        const int64_t le = (int64_t)line_end[li];
        uint8_t st = stdin_mode ? kFaEmpty : kFaColumn;
        uint32_t S = 0, E = 0, as = 0, ae = 0, base = 'N';
        int32_t gi = -1;
        if (le > ls) {
            if (byte_at(buf, ls) == '#') {
                st = le - ls >= 6 && byte_at(buf, ls + 1) == 'C' && byte_at(buf, ls + 2) == 'H' && byte_at(buf, ls + 3) == 'R' &&
                             byte_at(buf, ls + 4) == 'O' && byte_at(buf, ls + 5) == 'M'
                         ? kFaChrom
                         : kFaHeader;
            } else {
                // file mode strips one '\r' :357; stdin mode keeps it as a byte of the last field
                const int64_t end = le - (!stdin_mode && byte_at(buf, le - 1) == '\r' ? 1 : 0);
                uint32_t nt = 0;  // tabs seen: all of them on stdin (the field count), nine at least else
                for (int64_t w = ls & ~(int64_t)15; w < end && (stdin_mode || nt < 9u); w += kWaveStep) {
                    const int64_t blk = w + (int64_t)lane() * kBlockBytes;
                    uint32_t m = 0;
                    if (blk < end) m = eq_mask16(load16(buf, blk), kRepTab) & range_mask16(blk, ls, end);
                    const uint32_t c = (uint32_t)__popc(m);
                    const uint32_t incl = wave_incl_scan32(c);
                    uint32_t idx = nt + incl - c;
                    for (; m && idx < 9u; m &= m - 1u, idx++) t[idx] = (uint32_t)(blk + __builtin_ctz(m) - ls);
                    nt += lane_last(incl);
                }
                fa_wave_sync();
                st = kFaColumn;
                if (stdin_mode) {  // fields.size() < 9 + numSamples :480 (no field after a final tab :473-478)
                    const uint64_t fields = (uint64_t)nt + 1u - (byte_at(buf, end - 1) == '\t' ? 1u : 0u);
                    if (fields < 9ull + n_samples) st = kFaSkipped;
                }
                if (st == kFaColumn && nt >= 9u) {
                    const int32_t t2 = uniform32((int)t[2]), t3 = uniform32((int)t[3]), t4 = uniform32((int)t[4]),
                                  t7 = uniform32((int)t[7]), t8 = uniform32((int)t[8]);
                    const char *__restrict__ b = buf + ls;
                    S = (uint32_t)t8 + 1u;
                    E = (uint32_t)(end - ls);
                    as = (uint32_t)t3 + 1u;
                    ae = (uint32_t)t4;
                    gi = gt_index(buf, ls + t7 + 1, ls + t8);
                    if (lane() == 0) {  // the REF base :365 (file: as char) / :486 (stdin: toupper)
                        if (t3 - t2 == 2) {
                            const uint32_t c = byte_at(b, t2 + 1);
                            base = stdin_mode ? (c - 'a' < 26u ? c - 32u : c) : (c >= 'a' && c < 0x80u ? c - 32u : c);
                        }
                    } else if (lane() < (int)kFaTable) {
                        base = fa_allele_base(b, (int32_t)as, (int32_t)ae, (uint32_t)lane());
                    }
                }
                fa_wave_sync();
            }
        }
        if (lane() < (int)kFaTable) meta[i].tab[lane()] = (uint8_t)base;
        if (lane() == 0) {
            status[li] = st;
            flag[i] = st == kFaColumn;
            meta[i].S = S;
            meta[i].E = E;
            meta[i].alt_s = as;
            meta[i].alt_e = ae;
            meta[i].gi = gi;
            if (st == kFaChrom) atomicAdd(&counters[1], 1ull);
        }
    }
}

// ---- bases ----------------------------------------------------------------------------------------

// gt_fast's reducer: a fixed-stride sample "a s b" is N unless both are digits (a '.' first :201,
// a '.' second :211), else the two alleles' bases combined; sample k of the region goes to out[k]
struct FaFastOp {
    uint8_t *out;
    int64_t S;
    uint32_t ns;
    FaTab T;
    __device__ void begin(uint32_t, uint32_t) {}
    __device__ bool done() const { return false; }
    __device__ void dword(const DwordView &v) {
        const uint64_t k = (uint64_t)(v.p - S) >> 2;
        if (!v.real || k >= ns) return;
        const uint32_t a = v.f & 0xFFu, b = v.f >> 16;
        out[k] = (uint8_t)(v.dig == 0x01000100u ? fa_combine(T.at(a), T.at(b)) : (uint32_t)'N');
    }
    __device__ void finish() {}
};

// a wave per column line i of the block: M[col[i] * pitch + s] for every s < n_samples
__global__ __launch_bounds__(kFaThreads) void k_fa_bases(const char *__restrict__ buf, int64_t data_start,
                                                         const uint64_t *__restrict__ line_end, uint64_t l0, uint64_t n,
                                                         const uint8_t *__restrict__ status,
                                                         const uint64_t *__restrict__ col, const FaMeta *__restrict__ meta,
                                                         uint32_t n_samples, uint64_t pitch, uint8_t *__restrict__ M,
                                                         unsigned long long *__restrict__ counters) {
    // (a wave per line and no loop: fewer values live across the sweeps)
    const uint64_t i = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    if (i < n && status[l0 + i] == kFaColumn) {
        const uint64_t li = l0 + i;
        const int64_t ls = li ? (int64_t)line_end[li - 1] + 1 : data_start;
        const uint32_t *mw = reinterpret_cast<const uint32_t *>(meta + i);
        FaLine L;
        L.b = buf + ls;
        const int32_t S = uniform32((int)mw[0]), E = uniform32((int)mw[1]);
        L.alt_s = uniform32((int)mw[2]);
        L.alt_e = uniform32((int)mw[3]);
        L.gi = uniform32((int)mw[4]);
        L.T = FaTab{mw[8] | ((uint64_t)mw[9] << 32), mw[10] | ((uint64_t)mw[11] << 32)};
        uint8_t *__restrict__ out = M + (uint64_t)uniform64((int64_t)col[i]) * pitch;
        bool fast = false;
        uint32_t have = 0;  // the samples the line has, up to n_samples
        if (L.gi == 0 && E > S) {
            FaFastOp op{out, ls + S, n_samples, L.T};
            fast = gt_fast<4>(buf, ls + S, ls + E, op);
            have = (uint32_t)std::min<uint64_t>(((uint64_t)(E - S) + 1u) >> 2, n_samples);
            // (the general path below writes every byte again: the fast path's stores land first)
            if (!fast) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
        if (!fast) {
            // a lane per sample start in its 16 B: S, and the byte after every tab, before E; the
            // start's rank among them is the sample's number
            const int64_t Sa = ls + S, Ea = ls + E;
            uint32_t seen = 0;
            for (int64_t w = Sa & ~(int64_t)15; w < Ea && E > S; w += kWaveStep) {  // (an empty region has no start)
                const int64_t blk = w + (int64_t)lane() * kBlockBytes;
                uint32_t starts = 0;
                if (blk < Ea) {
                    const uint32_t tm = eq_mask16(load16(buf, blk), kRepTab);
                    starts = (tm << 1) & 0xFFFFu;
                    if (blk > 0 && byte_at(buf, blk - 1) == '\t') starts |= 1u;
                    starts &= range_mask16(blk, Sa + 1, Ea);
                    if (Sa >= blk && Sa < blk + 16) starts |= 1u << (Sa - blk);
                }
                const uint32_t c = (uint32_t)__popc(starts);
                const uint32_t incl = wave_incl_scan32(c);
                uint32_t k = seen + incl - c;
                for (; starts; starts &= starts - 1u, k++)
                    if (k < n_samples) out[k] = (uint8_t)fa_sample(L, (int32_t)(blk + __builtin_ctz(starts) - ls), E);
                seen += lane_last(incl);
            }
            have = std::min(seen, n_samples);
            if (lane() == 0) atomicAdd(&counters[0], 1ull);
        }
        for (uint32_t k = have + (uint32_t)lane(); k < n_samples; k += kWave) out[k] = 0;  // :342 the zeroed matrix
    }
}

// ---- transpose ------------------------------------------------------------------------------------

// block (x, y): the columns of global tile first_col / 240 + x that this call holds, samples
// [64 y, 64 y + 64).  M row c is column first_col + c.
__global__ __launch_bounds__(kFaThreads) void k_fa_transpose(const uint8_t *__restrict__ M, uint64_t pitch, uint64_t ncols,
                                                             uint32_t n_samples, uint64_t first_col, uint64_t total_cols,
                                                             const uint64_t *__restrict__ row_off,
                                                             const uint64_t *__restrict__ skip, char *__restrict__ text) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kFaTileSamples * kFaRow];
    const uint64_t gt = first_col / kFaTileCols + blockIdx.x;
    const uint64_t g0 = std::max<uint64_t>(first_col, gt * kFaTileCols);
    const uint64_t g1 = std::min<uint64_t>(first_col + ncols, (gt + 1) * kFaTileCols);
    const uint32_t tc = (uint32_t)(g1 - g0);  // 1..240
    const uint64_t c0 = g0 - first_col;
    const uint32_t s0 = blockIdx.y * kFaTileSamples;
    const uint32_t nsb = std::min<uint32_t>(kFaTileSamples, n_samples - s0);
    const bool as_text = !skip && g0 % kFaLine == 0;
    const uint32_t wv = threadIdx.x / kWave, ln = (uint32_t)lane();
    // in: a wave per column, a lane per sample
    for (uint32_t c = wv; c < tc; c += kFaWaves)
        if (ln < nsb) tile[ln * kFaRow + (as_text ? c + c / kFaLine : c)] = M[(c0 + c) * pitch + s0 + ln];
    const bool last = g1 == total_cols;  // the rows end in this tile
    const uint32_t bytes = tc + tc / kFaLine + (last && tc % kFaLine ? 1u : 0u);
    if (as_text) {  // the '\n' after every 60 bases, and after the row's last
        const uint32_t k = wv;  // (tc / 60 <= 4 = the waves)
        if (ln < nsb && k < tc / kFaLine) tile[ln * kFaRow + k * (kFaLine + 1) + kFaLine] = '\n';
        if (ln < nsb && wv == 0 && last && tc % kFaLine) tile[ln * kFaRow + bytes - 1] = '\n';
    }
    __syncthreads();
    // out: a wave per sample
    for (uint32_t s = wv; s < nsb; s += kFaWaves) {
        const uint8_t *__restrict__ row = tile + s * kFaRow;
        if (as_text) {
            char *dst = text + row_off[s0 + s] + (g0 / kFaLine) * (kFaLine + 1);
            const int m = (int)((uintptr_t)dst & 3u);
            const int d = 4 * (int)ln - m;  // the row bytes [d, d + 4) are this lane's aligned dword
            if (d >= 0 && d + 4 <= (int)bytes) {
                const uint32_t v = (uint32_t)row[d] | ((uint32_t)row[d + 1] << 8) | ((uint32_t)row[d + 2] << 16) |
                                   ((uint32_t)row[d + 3] << 24);
                *reinterpret_cast<uint32_t *>(dst + d) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (d + k >= 0 && d + k < (int)bytes) dst[d + k] = (char)row[d + k];
            }
        } else {
            const uint64_t sk = skip ? skip[s0 + s] : 0;
            const uint64_t vs = total_cols - sk;  // the row's columns
            char *dst = text + row_off[s0 + s];
            for (uint32_t c = ln; c < tc; c += kWave) {
                const uint64_t g = g0 + c;
                if (g < sk) continue;
                const uint64_t cc = g - sk, pos = cc + cc / kFaLine;
                dst[pos] = (char)row[c];
                if (cc % kFaLine == kFaLine - 1 || cc == vs - 1) dst[pos + 1] = '\n';
            }
        }
    }
}

static unsigned fa_blocks(uint64_t waves) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((waves + kFaWaves - 1) / kFaWaves, 8192));
}

hipError_t launch_fa_scan(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                          int stdin_mode, uint32_t n_samples, uint8_t *status, uint32_t *flag, FaMeta *meta,
                          unsigned long long *counters, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_fa_scan, dim3(fa_blocks(n)), dim3(kFaThreads), 0, s, buf, data_start, line_end, l0, n, stdin_mode,
                       n_samples, status, flag, meta, counters);
    return hipGetLastError();
}

hipError_t launch_fa_bases(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                           const uint8_t *status, const uint64_t *col, const FaMeta *meta, uint32_t n_samples,
                           uint64_t pitch, uint8_t *M, unsigned long long *counters, hipStream_t s) {
    if (!n || !n_samples) return hipSuccess;
    hipLaunchKernelGGL(k_fa_bases, dim3((unsigned)((n + kFaWaves - 1) / kFaWaves)), dim3(kFaThreads), 0, s, buf, data_start, line_end, l0, n, status, col,
                       meta, n_samples, pitch, M, counters);
    return hipGetLastError();
}

hipError_t launch_fa_transpose(const uint8_t *M, uint64_t pitch, uint64_t ncols, uint32_t n_samples, uint64_t first_col,
                               uint64_t total_cols, const uint64_t *row_off, const uint64_t *skip, char *text,
                               hipStream_t s) {
    if (!ncols || !n_samples) return hipSuccess;
    const uint64_t tiles = (first_col + ncols - 1) / kFaTileCols - first_col / kFaTileCols + 1;
    const uint64_t sy = ((uint64_t)n_samples + kFaTileSamples - 1) / kFaTileSamples;
    if (tiles >= (1ull << 31) || sy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fa_transpose, dim3((unsigned)tiles, (unsigned)sy), dim3(kFaThreads), 0, s, M, pitch, ncols,
                       n_samples, first_col, total_cols, row_off, skip, text);
    return hipGetLastError();
}

}  // namespace vcfxg
