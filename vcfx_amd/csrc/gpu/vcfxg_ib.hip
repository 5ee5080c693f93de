// vcfxg_ib.hip -- VCFX_inbreeding_calculator: one output row per SAMPLE, accumulated over every
// record of the file (the first reduction along the sample axis on the record walk).
//
// Three stages per block of records (DESIGN.md "Inbreeding coefficient"):
//   A. the walk (k_ib_walk: one wave per chunk of the data region, one HBM pass, no line index)
//      or, on the two-sweep schedule, k_ib_lines over the line index: per line a status
//      (kIbSkip / kIbParsed / kIbUsed), altSum, nGood, nparsed and a row of int8 genotype codes
//      (parseGenotypeCode, VCFX_inbreeding_calculator.cpp:296-339: 0, 1, 2 or -1).  A record
//      of "a s b\t" samples takes the fixed-stride sweep (gt_fast with IbOpW: its clean step
//      writes four codes as one dword into the LDS row); any other shape takes the per-field
//      decode (gt_code_win / gt_code_ib) and is counted in general_records;
//   B. k_ib_table: per used record the expected heterozygosity a sample adds, by the sample's
//      own code (excludeSample: three values, global: one), with the boundary flags;
//   C. k_ib_pack regroups the codes per 64 samples and 16 records; k_ib_chain: one lane per sample walks the block's records in file order and adds the
//      table value of its code to sumExp -- the same fp64 operands in the same order as the
//      reference's loop (:596-626 / :748-776), so the sum is bit-identical.  The chain carries
//      (sumExp, obsHet, usedCount, carried code) per sample from block to block.
// k_ib_rows then writes "<name>\t<F>\n" per sample with appendDouble's digits (:230-266).
//
// Record rules.  File mode (calculateInbreedingMmap :536-629): '\r' stripped, empty and '#'
// lines skipped, ALT empty or with a comma skipped, no tenth field skipped; the sample columns
// that START before the line end are parsed, at most n_samples; the code buffer is reused, so
// a sample past the parsed columns keeps the code of the last parsed record (0 before any).
// Stdin mode (calculateInbreedingStdin :689-777): fewer than 10 tab-separated fields skipped,
// ALT with a comma skipped, a sample without a column is -1.
#include "vcfxg_device.h"
#include "vcfxg_gt.h"
#include "vcfxg_kernels.h"
#include "vcfxg_walk.h"

namespace vcfxg {

constexpr int kIbSkip = 0, kIbParsed = 1, kIbUsed = 2;
constexpr uint32_t kRepComma = 0x2C2C2C2Cu;

struct IbMeta {
    int32_t status, alt_sum, n_good, n_parsed;
};

// parseGenotypeCode (:296-339) of the field starting at p (the field ends at the next '\t' or
// at ae): the GT prefix up to the first ':', leading ' ' / '\r' skipped, a digit run, '/' or
// '|', a digit run; whatever follows the second run is ignored.  An allele above 1 or a '.'
// where a digit is wanted gives -1.  (A run's value saturates at 2: "01" is 1, "10" is > 1.)
__device__ __forceinline__ int gt_code_ib(const char *__restrict__ buf, int64_t p, int64_t ae) {
    auto get = [&](int64_t q) -> uint32_t {
        const uint32_t c = q < ae ? byte_at(buf, q) : (uint32_t)'\t';
        return c == ':' ? (uint32_t)'\t' : c;  // the field's end
    };
    uint32_t c = get(p);
    while (c == ' ' || c == '\r') c = get(++p);
    if (c < '0' || c > '9') return -1;
    int a1 = 0;
    while (c >= '0' && c <= '9') {
        a1 = a1 > 1 ? 2 : a1 * 10 + (int)(c - '0');
        c = get(++p);
    }
    if (c != '/' && c != '|') return -1;
    c = get(++p);
    if (c < '0' || c > '9') return -1;
    int a2 = 0;
    while (c >= '0' && c <= '9') {
        a2 = a2 > 1 ? 2 : a2 * 10 + (int)(c - '0');
        c = get(++p);
    }
    if (a1 > 1 || a2 > 1) return -1;
    return a1 + a2;
}

// one line [ls, le) with the whole wave (every lane active): its codes into row[0, ns), its
// meta (lane 0); returns the status (wave-uniform)
// A "a/b" field whose four bytes (two alleles, the separator, the byte after them) are at hand in
// win (byte 0 first): its code, or kIbSlow when the bytes do not settle it.  A field that starts
// with a digit above 1 or a '.' is -1 whatever follows, and so is one whose second allele does.
constexpr int kIbSlow = -2;
__device__ __forceinline__ int gt_code_win(uint32_t win) {
    const uint32_t c0 = win & 0xFFu, c1 = (win >> 8) & 0xFFu, c2 = (win >> 16) & 0xFFu, c3 = win >> 24;
    if (c0 == '.' || (c0 >= '2' && c0 <= '9')) return -1;
    if ((c0 != '0' && c0 != '1') || (c1 != '/' && c1 != '|')) return kIbSlow;
    if (c2 == '.' || (c2 >= '2' && c2 <= '9')) return -1;
    if ((c2 != '0' && c2 != '1') || (c3 >= '0' && c3 <= '9')) return kIbSlow;
    return (int)(c0 - '0') + (int)(c2 - '0');
}

constexpr uint32_t kIbLdsRow = 4096;  // a wave's LDS code row: rows of up to this many bytes are composed there

// The fixed-stride sweep's reducer (gt_fast, vcfxg_gt.h): a record whose samples are all
// "a s b" with one separator, a tab between them.  A clean step -- four samples whose alleles
// are all '0' / '1' (e = dword ^ "0 s 0 \t" has bits 0 and 16 only) -- gives its four codes as
// one dword into the wave's LDS row, as LdOpW::clean_at does; any other sample dword gives
// a + b for alleles 0 / 1 and -1 for a digit above 1 or a '.', which is what parseGenotypeCode
// gives for a field of exactly three bytes.  Another shape fails the sweep (gt_fast returns
// false) and the record takes the per-field decode below.
struct IbOpW {
    __attribute__((address_space(3))) int8_t *row;
    int64_t S;
    uint32_t ns;
    uint32_t asum = 0, ngood = 0;
    __device__ void begin(uint32_t, uint32_t) {}
    __device__ bool done() const { return false; }
    __device__ void finish() {}
    __device__ void sample(int64_t) {}
    __device__ void dword(const DwordView &v) {
        if (!v.real) return;
        const int64_t k = (v.p - S) >> 2;
        if (k >= (int64_t)ns) return;
        const uint32_t a = v.d & 0xFF, b = (v.d >> 16) & 0xFF;
        const int code = ((a - '0') < 2u && (b - '0') < 2u) ? (int)(a - '0' + b - '0') : -1;
        row[k] = (int8_t)code;
        if (code >= 0) {
            asum += (uint32_t)code;
            ngood++;
        }
    }
    __device__ void clean_at(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, int64_t p) {
        const int64_t k = (p - S) >> 2;
        const uint32_t c[4] = {(e0 + (e0 >> 16)) & 3u, (e1 + (e1 >> 16)) & 3u, (e2 + (e2 >> 16)) & 3u,
                               (e3 + (e3 >> 16)) & 3u};
        if (k + 3 < (int64_t)ns) {
            const uint32_t w = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            auto *r = row + k;
            if ((k & 3) == 0) {
                *reinterpret_cast<__attribute__((address_space(3))) uint32_t *>(r) = w;
            } else if ((k & 1) == 0) {
                reinterpret_cast<__attribute__((address_space(3))) uint16_t *>(r)[0] = (uint16_t)w;
                reinterpret_cast<__attribute__((address_space(3))) uint16_t *>(r)[1] = (uint16_t)(w >> 16);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) r[i] = (int8_t)c[i];
            }
            asum += c[0] + c[1] + c[2] + c[3];
            ngood += 4u;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (k + i < (int64_t)ns) {
                    row[k + i] = (int8_t)c[i];
                    asum += c[i];
                    ngood++;
                }
        }
    }
};

// the composed LDS row out with 16 B stores
__device__ __forceinline__ void ib_flush(int8_t *__restrict__ row, const int8_t *lrow, uint32_t ld) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (uint32_t o = 16u * (uint32_t)lane(); o < ld; o += kWaveStep)
        *reinterpret_cast<uint4 *>(row + o) = *reinterpret_cast<const uint4 *>(lrow + o);
}

constexpr int kIbGeneral = 16;  // ib_line's result: the status, + kIbGeneral when the record left the clean step

// lrow: the wave's LDS row (nullptr: the codes go straight to row, and no fixed-stride sweep);
// lds: the wave's scratch of >= 10 offsets (head_tabs)
__device__ __forceinline__ int ib_line(const char *__restrict__ buf, int64_t ls, int64_t le, int mode, uint32_t ns,
                                       uint32_t ld, int8_t *__restrict__ row, IbMeta *__restrict__ meta,
                                       int8_t *lrow, int64_t *lds) {
    int64_t ae = le;
    if (ae > ls && byte_at(buf, ae - 1) == '\r') ae--;
    int status = kIbSkip;
    bool general = false;
    uint32_t asum = 0, ngood = 0, npar = 0;
    bool settled = false;
    if (lrow && ae > ls && byte_at(buf, ls) != '#') {
        // the head: nine tabs, ALT between tabs 3 and 4, the samples from S = tab 8 + 1
        int64_t t[9];
        const int nt = head_tabs(buf, ls, ae, 9, t, lds);
        if (nt == 9) {
            const int64_t S = t[8] + 1;
            bool comma = false;
            for (int64_t q = t[3] + 1; q < t[4]; q += kWave) {
                const int64_t x = q + lane();
                comma = comma || __any(x < t[4] && byte_at(buf, x) == ',');
            }
            const bool file = mode == 0;
            if (comma || (file && (t[4] == t[3] + 1 || S >= ae))) {
                settled = true;  // skipped (:553-564 / :720-723)
            } else if (S < ae) {
                IbOpW op{(__attribute__((address_space(3))) int8_t *)lrow, S, ns};
                if (gt_fast<6>(buf, S, ae, op)) {
                    asum = wave_sum32(op.asum);
                    ngood = wave_sum32(op.ngood);
                    npar = (uint32_t)std::min<int64_t>((int64_t)ns, (ae - S + 1) >> 2);
                    ib_flush(row, lrow, ld);
                    status = ngood >= 2u ? kIbUsed : kIbParsed;
                    settled = true;
                }
            }
        }
    }
    if (!settled && ae > ls && byte_at(buf, ls) != '#') {
        general = true;
        const bool file = mode == 0;
        bool alt_ne = false, comma = false, f9 = false;
        uint32_t running = 0;  // tabs before this step
        for (int64_t w = ls & ~(int64_t)15; w < ae; w += kWaveStep) {
            const int64_t blk = w + (int64_t)lane() * kBlockBytes;
            uint32_t tm = 0, cm = 0, in = 0;
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (blk < ae) {
                v = load16(buf, blk);
                in = range_mask16(blk, ls, ae);
                tm = eq_mask16(v, kRepTab) & in;
                cm = eq_mask16(v, kRepComma) & in;
            }
            const uint32_t nx = (uint32_t)__shfl_down((int)v.x, 1);  // the next lane's first four bytes
            const uint32_t c = (uint32_t)__popc(tm);
            const uint32_t incl = wave_incl_scan32(c);
            const uint32_t excl = running + incl - c;  // tabs before this lane's bytes
            running += lane_last(incl);
            // ALT = field 4: the bytes after tab 3 up to tab 4
            const int k4 = 4 - (int)excl;
            if (k4 >= 0 && k4 <= (int)c) {
                const int s0 = k4 == 0 ? 0 : nth_bit(tm, k4 - 1) + 1;
                const int e0 = k4 < (int)c ? nth_bit(tm, k4) : 16;
                const uint32_t f4 = e0 > s0 ? (((1u << e0) - 1u) & ~((1u << s0) - 1u)) & in : 0u;
                alt_ne = alt_ne || f4 != 0u;
                comma = comma || (f4 & cm) != 0u;
            }
            // tab ti ends field ti; the sample columns are fields 9, 10, ...
            uint32_t mm = tm, ti = excl;
            while (mm) {
                const int j = __builtin_ctz(mm);
                mm &= mm - 1u;
                if (ti >= 8u) {
                    const uint32_t s = ti - 8u;
                    const int64_t pos = blk + j + 1;
                    // file mode: a column that starts at the line end is not there
                    const bool starts = !file || pos < ae;
                    if (ti == 8u && starts) f9 = true;
                    if (starts && s < ns) {
                        // the field's first four bytes out of the registers when they are all in the
                        // line and in this lane's 16 bytes or the next lane's first 4
                        int code = kIbSlow;
                        const int q = j + 1;
                        if (pos + 3 < ae && (q + 3 < 16 || lane() < kWave - 1)) {
                            const int wi = q >> 2;
                            const uint32_t w0 = wi == 0 ? v.x : wi == 1 ? v.y : wi == 2 ? v.z : wi == 3 ? v.w : nx;
                            const uint32_t w1 = wi == 0 ? v.y : wi == 1 ? v.z : wi == 2 ? v.w : nx;
                            code = gt_code_win((uint32_t)(((((uint64_t)w1) << 32) | w0) >> (8 * (q & 3))));
                        }
                        if (code == kIbSlow) code = gt_code_ib(buf, pos, ae);
                        (lrow ? lrow : row)[s] = (int8_t)code;
                        npar++;
                        if (code >= 0) {
                            asum += (uint32_t)code;
                            ngood++;
                        }
                    }
                }
                ti++;
            }
        }
        if (lrow) ib_flush(row, lrow, ld);
        const bool ok = __any(f9) && !__any(comma) && (!file || __any(alt_ne));
        asum = wave_sum32(asum);
        ngood = wave_sum32(ngood);
        npar = wave_sum32(npar);
        status = !ok ? kIbSkip : ngood >= 2u ? kIbUsed : kIbParsed;
        general = ok;
    }
    if (lane() == 0) *meta = IbMeta{status, (int32_t)asum, (int32_t)ngood, (int32_t)npar};
    return status + (general ? kIbGeneral : 0);
}

// a wave's tallies: [0] parsed records, [1] used records, [2] records off the clean step, [3] lines
struct IbTally {
    uint32_t parsed = 0, used = 0, general = 0, lines = 0;
    __device__ void line(int r) {
        const int st = r & (kIbGeneral - 1);
        parsed += st != kIbSkip;
        used += st == kIbUsed;
        general += (r & kIbGeneral) != 0;
        lines++;
    }
    __device__ void flush(unsigned long long *counters) const {
        if (lane() == 0) {
            if (parsed) atomicAdd(&counters[0], (unsigned long long)parsed);
            if (used) atomicAdd(&counters[1], (unsigned long long)used);
            if (general) atomicAdd(&counters[2], (unsigned long long)general);
            if (lines) atomicAdd(&counters[3], (unsigned long long)lines);
        }
    }
};

// A (walk): walker g of this launch takes chunk w0 + g of the data region; its lines go to the
// slots [g * cap_w, g * cap_w + cnt[g]) in file order.  *ovf: a walker ran out of slots.
__global__ __launch_bounds__(kWalkThreads) void k_ib_walk(const char *__restrict__ buf, int64_t lo, int64_t hi,
                                                          int64_t chunk, int64_t w0, int64_t nw, uint32_t G,
                                                          uint32_t cap_w, int mode, uint32_t ns, uint32_t ld,
                                                          int8_t *__restrict__ codes, IbMeta *__restrict__ meta,
                                                          uint32_t *__restrict__ cnt, unsigned *__restrict__ ovf,
                                                          unsigned long long *__restrict__ counters) {
    __shared__ __attribute__((aligned(16))) int8_t lrows[kWalkWaves][kIbLdsRow];
    __shared__ int64_t scratch[kWalkWaves][16];
    int8_t *lrow = ld <= kIbLdsRow ? lrows[threadIdx.x / kWave] : nullptr;
    int64_t *lds = scratch[threadIdx.x / kWave];
    const uint32_t g = (uint32_t)uniform32((int)(blockIdx.x * (uint32_t)kWalkWaves + threadIdx.x / kWave));
    if (g >= G) return;
    const int64_t w = w0 + g;
    uint32_t k = 0;
    IbTally tally;
    if (w < nw) {
        const int64_t cs = lo + w * chunk, ce = std::min<int64_t>(cs + chunk, hi);
        int64_t b0, b1;
        walker_lines(buf, lo, hi, cs, ce, b0, b1, chunk);
        int64_t p = b0;
        while (p < b1) {
            const int64_t e = scan_nl<1>(buf, p, hi);
            if (k >= cap_w) {
                if (lane() == 0) atomicOr(ovf, 1u);
                break;
            }
            const uint64_t slot = (uint64_t)g * cap_w + k;
            tally.line(ib_line(buf, p, e, mode, ns, ld, codes + slot * ld, meta + slot, lrow, lds));
            k++;
            p = e + 1;
        }
    }
    if (lane() == 0) cnt[g] = k;
    tally.flush(counters);
}

// A (two-sweep): indexed lines [l0, l0 + n), a wave per line, slot = line - l0
__global__ __launch_bounds__(256) void k_ib_lines(const char *__restrict__ buf, int64_t data_start,
                                                  const uint64_t *__restrict__ line_end, uint64_t l0, uint32_t n,
                                                  int mode, uint32_t ns, uint32_t ld, int8_t *__restrict__ codes,
                                                  IbMeta *__restrict__ meta, uint32_t *__restrict__ cnt,
                                                  unsigned long long *__restrict__ counters) {
    __shared__ __attribute__((aligned(16))) int8_t lrows[256 / kWave][kIbLdsRow];
    __shared__ int64_t scratch[256 / kWave][16];
    int8_t *lrow = ld <= kIbLdsRow ? lrows[threadIdx.x / kWave] : nullptr;
    int64_t *lds = scratch[threadIdx.x / kWave];
    const uint32_t wid = (uint32_t)uniform32((int)((blockIdx.x * blockDim.x + threadIdx.x) / kWave));
    const uint32_t nwv = (gridDim.x * blockDim.x) / kWave;
    IbTally tally;
    for (uint32_t i = wid; i < n; i += nwv) {
        const uint64_t li = l0 + i;
        const int64_t ls = li ? (int64_t)line_end[li - 1] + 1 : data_start, le = (int64_t)line_end[li];
        tally.line(ib_line(buf, ls, le, mode, ns, ld, codes + (uint64_t)i * ld, meta + i, lrow, lds));
    }
    if (wid == 0 && lane() == 0) cnt[0] = n;
    tally.flush(counters);
}

// B: the block's records in file order.  k_ib_scan turns the groups' counts into offsets
// (offs[G] = the block's records); k_ib_table then writes record j = offs[g] + k of slot
// g cap_w + k: its status, nparsed and slot and, for a used record, the value a sample of code
// 0 / 1 / 2 adds to sumExp with the boundary flags (bit c: freq <= 0 || freq >= 1 for code c).
// :593, :600-620
struct alignas(16) IbRec {
    double e[3];
    uint32_t flags;
    int32_t status;
    uint32_t n_parsed, slot, pad[2];
};

__global__ __launch_bounds__(256) void k_ib_scan(const uint32_t *__restrict__ cnt, uint32_t G,
                                                 uint32_t *__restrict__ offs) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t run;
    if (threadIdx.x == 0) run = 0;
    __syncthreads();
    for (uint32_t g0 = 0; g0 < G; g0 += 256) {
        const uint32_t g = g0 + threadIdx.x;
        part[threadIdx.x] = g < G ? cnt[g] : 0u;
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t k = 0; k < threadIdx.x; k++) before += part[k];
        const uint32_t base = run;
        if (g < G) offs[g] = base + before;
        __syncthreads();
        if (threadIdx.x == 255) run = base + before + part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) offs[G] = run;
}

__global__ __launch_bounds__(256) void k_ib_table(const IbMeta *__restrict__ meta, const uint32_t *__restrict__ cnt,
                                                  const uint32_t *__restrict__ offs, uint32_t G, uint32_t cap_w,
                                                  int global_freq, IbRec *__restrict__ rec) {
    const uint64_t slot = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (slot >= (uint64_t)G * cap_w) return;
    const uint32_t g = (uint32_t)(slot / cap_w), k = (uint32_t)(slot % cap_w);
    if (k >= cnt[g]) return;
    const IbMeta m = meta[slot];
    IbRec r;
    r.e[0] = r.e[1] = r.e[2] = 0.0;
    r.flags = 0;
    r.status = m.status;
    r.n_parsed = (uint32_t)m.n_parsed;
    r.slot = (uint32_t)slot;
    r.pad[0] = r.pad[1] = 0;
    if (m.status == kIbUsed)
        for (int c = 0; c < 3; c++) {
            const double freq = global_freq
                                    ? __ddiv_rn((double)m.alt_sum, __dmul_rn(2.0, (double)m.n_good))
                                    : __ddiv_rn((double)(m.alt_sum - c), __dmul_rn(2.0, (double)(m.n_good - 1)));
            if (freq <= 0.0 || freq >= 1.0) r.flags |= 1u << c;
            r.e[c] = __dmul_rn(__dmul_rn(2.0, freq), __dsub_rn(1.0, freq));
        }
    rec[offs[g] + k] = r;
}

// The block's codes regrouped for the chain: for sample tile t (64 samples) and record group jg
// (16 records in file order) one KiB, lane l's 16 bytes = sample 64 t + l's codes of the 16
// records (kIbNoCol where the record has no such column), so a chain lane takes 16 records
// with one 16 B load from a sequential stream.  ng: the stride in groups (>= the block's).
constexpr int kIbGroup = 16;
constexpr uint32_t kIbNoCol = 0xFEu;  // (-2 as int8)
__global__ __launch_bounds__(256) void k_ib_pack(const int8_t *__restrict__ codes, uint32_t ld,
                                                 const IbRec *__restrict__ rec, const uint32_t *__restrict__ n_rec,
                                                 uint32_t ns, uint32_t ng, uint4 *__restrict__ packed) {
    const uint32_t N = *n_rec, jg = blockIdx.x;
    if (jg * kIbGroup >= N) return;
    const uint32_t t = blockIdx.y * 4u + threadIdx.x / kWave, s = t * kWave + (uint32_t)lane();
    if (t * kWave >= ns) return;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < kIbGroup; u++) {
        const uint32_t j = std::min<uint32_t>(jg * kIbGroup + u, N - 1);
        const IbRec &r = rec[j];
        uint32_t c = kIbNoCol;
        if (s < ns && s < r.n_parsed) c = (uint32_t)(uint8_t)codes[(uint64_t)r.slot * ld + s];
        w[u / 4] |= c << (8 * (u % 4));
    }
    packed[((uint64_t)t * ng + jg) * kWave + lane()] = uint4{w[0], w[1], w[2], w[3]};
}

// C: lane = sample.  The only dependent work per record is the select of the record's value by
// the lane's code and the add.  Each step takes 16 records: their codes are one 16 B load per
// lane, their entries 12 B per lane (the 16 entries' 192 dwords over the 64 lanes, read back
// with v_readlane), both requested kIbAhead steps before they are used, so no memory access is
// on the chain.  The adds stay in file order, one rounding each.
constexpr int kIbAhead = 3;
__global__ __launch_bounds__(kWave) void k_ib_chain(const uint4 *__restrict__ packed, uint32_t ng,
                                                    const IbRec *__restrict__ rec, const uint32_t *__restrict__ n_rec,
                                                    uint32_t ns, int mode, int skip_boundary, int count_boundary,
                                                    double *__restrict__ sum_exp, uint64_t *__restrict__ obs_het,
                                                    uint64_t *__restrict__ used_cnt, int32_t *__restrict__ carried_p) {
    const uint32_t t = blockIdx.x, s = t * kWave + threadIdx.x;
    const bool act = s < ns;
    const uint32_t sc = act ? s : ns - 1;  // (idle lanes of the last wave carry the last sample's state)
    double sum = sum_exp[sc];
    uint32_t obs = 0, used = 0;
    int carried = carried_p[sc];
    const bool file = mode == 0;
    const uint32_t N = *n_rec, nb = (N + kIbGroup - 1) / kIbGroup;
    const uint4 *pk = packed + (uint64_t)t * ng * kWave + lane();
    const uint32_t *rw = reinterpret_cast<const uint32_t *>(rec) + 3 * lane();
    constexpr uint32_t kRecDw = sizeof(IbRec) / 4 * kIbGroup;  // dwords of a step's entries
    static_assert(sizeof(IbRec) == 48 && kRecDw == 3 * kWave, "a step's entries are 3 dwords per lane");
    uint4 cq[kIbAhead + 1];
    uint32_t rq[kIbAhead + 1][3];
    auto fetch = [&](uint32_t b, int q) {
        const uint32_t bb = std::min<uint32_t>(b, nb - 1);
        cq[q] = pk[(uint64_t)bb * kWave];
        const uint32_t *p = rw + (uint64_t)bb * kRecDw;
        rq[q][0] = p[0];
        rq[q][1] = p[1];
        rq[q][2] = p[2];
    };
    if (nb) {
#pragma unroll
        for (int q = 0; q < kIbAhead; q++) fetch((uint32_t)q, q);
    }
    // steps b, b + 1, ... use the ring slots b % (kIbAhead + 1) (the step loop is unrolled by the
    // ring's size, so no slot is ever copied: a copy would wait for the load just issued)
    for (uint32_t b0 = 0; b0 < nb; b0 += kIbAhead + 1) {
#pragma unroll
        for (int q = 0; q <= kIbAhead; q++) {
            const uint32_t b = b0 + q;
            if (b >= nb) break;  // (uniform)
            fetch(b + kIbAhead, (q + kIbAhead) % (kIbAhead + 1));
            const uint32_t cw[4] = {cq[q].x, cq[q].y, cq[q].z, cq[q].w};
#pragma unroll
            for (int u = 0; u < kIbGroup; u++) {
                if (b * kIbGroup + u >= N) break;  // (uniform)
                // entry u's dword d: flat index 12 u + d of the step, lane (12 u + d) / 3, register % 3
                auto dw = [&](int d) { return lane_get(rq[q][(12 * u + d) % 3], (12 * u + d) / 3); };
                const int status = (int)dw(7);
                if (status == kIbSkip) continue;  // (uniform)
                const int raw = (int)(int8_t)((cw[u / 4] >> (8 * (u % 4))) & 0xFFu);
                const int code = raw != (int)(int8_t)kIbNoCol ? raw : file ? carried : -1;
                carried = code;
                if (status != kIbUsed) continue;  // (uniform)
                const double e0 = __hiloint2double((int)dw(1), (int)dw(0)),
                             e1 = __hiloint2double((int)dw(3), (int)dw(2)),
                             e2 = __hiloint2double((int)dw(5), (int)dw(4));
                const uint32_t flags = dw(6);
                const double e = code == 0 ? e0 : code == 1 ? e1 : e2;
                const bool good = code >= 0;
                const bool bnd = skip_boundary && ((flags >> (code & 3)) & 1u);
                const bool take = good && !bnd;
                const double tsum = __dadd_rn(sum, e);
                sum = take ? tsum : sum;  // a sample that is skipped adds nothing
                used += (take || (good && bnd && count_boundary)) ? 1u : 0u;
                obs += (take && code == 1) ? 1u : 0u;
            }
        }
    }
    if (act) {
        sum_exp[s] = sum;
        obs_het[s] += obs;
        used_cnt[s] += used;
        carried_p[s] = carried;
    }
}

// the rows: "<name>\tNA\n", "<name>\t1.000000\n" or "<name>\t<F>\n" (:645-663), F by
// appendDouble (:230-266).  One block; tiles of 256 samples, the rows' offsets by a block scan.
constexpr int kIbRowThreads = 256;
__global__ __launch_bounds__(kIbRowThreads) void k_ib_rows(const double *__restrict__ sum_exp,
                                                           const uint64_t *__restrict__ obs_het,
                                                           const uint64_t *__restrict__ used_cnt, uint32_t ns,
                                                           const char *__restrict__ names,
                                                           const uint64_t *__restrict__ noff, char *__restrict__ out,
                                                           uint64_t *__restrict__ text_bytes) {
    __shared__ uint32_t len[kIbRowThreads];
    __shared__ uint64_t tile_start;
    if (threadIdx.x == 0) tile_start = 0;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < ns; t0 += kIbRowThreads) {
        const uint32_t s = t0 + threadIdx.x;
        char v[48];
        uint32_t vl = 0, nl = 0;
        if (s < ns) {
            nl = (uint32_t)(noff[s + 1] - noff[s]);
            const double e = sum_exp[s];
            if (used_cnt[s] == 0) {
                v[0] = 'N';
                v[1] = 'A';
                vl = 2;
            } else if (e <= 0.0) {
                const char one[8] = {'1', '.', '0', '0', '0', '0', '0', '0'};
                for (int k = 0; k < 8; k++) v[k] = one[k];
                vl = 8;
            } else {
                double val = __dsub_rn(1.0, __ddiv_rn((double)obs_het[s], e));
                if (val < 0) {
                    v[vl++] = '-';
                    val = -val;
                }
                if (!(val < 9.0e18)) val = 9.0e18;  // (the reference's long long cast overflows there)
                long long ip = (long long)val;
                double fr = __dsub_rn(val, (double)ip);
                char ib[20];
                int il = 0;
                if (ip == 0) ib[il++] = '0';
                while (ip > 0) {
                    ib[il++] = (char)('0' + ip % 10);
                    ip /= 10;
                }
                for (int k = il - 1; k >= 0; k--) v[vl++] = ib[k];
                v[vl++] = '.';
                for (int k = 0; k < 6; k++) {
                    fr = __dmul_rn(fr, 10.0);
                    const int d = (int)fr;
                    v[vl++] = (char)('0' + d);
                    fr = __dsub_rn(fr, (double)d);
                }
            }
        }
        len[threadIdx.x] = s < ns ? nl + vl + 2 : 0;
        __syncthreads();
        uint32_t off = 0;  // (the tile's rows are a few KB: every thread sums the lengths before its own)
        for (uint32_t k = 0; k < threadIdx.x; k++) off += len[k];
        const uint64_t ts = tile_start;
        __syncthreads();
        if (threadIdx.x == kIbRowThreads - 1) tile_start = ts + off + len[threadIdx.x];
        if (s < ns) {
            char *o = out + ts + off;
            const char *nm = names + noff[s];
            for (uint32_t k = 0; k < nl; k++) o[k] = nm[k];
            o[nl] = '\t';
            for (uint32_t k = 0; k < vl; k++) o[nl + 1 + k] = v[k];
            o[nl + 1 + vl] = '\n';
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *text_bytes = tile_start;
}

size_t ib_meta_bytes() { return sizeof(IbMeta); }

hipError_t launch_ib_walk(const char *buf, int64_t lo, int64_t hi, int64_t chunk, int64_t w0, int64_t nw, uint32_t G,
                          uint32_t cap_w, int mode, uint32_t ns, uint32_t ld, int8_t *codes, void *meta, uint32_t *cnt,
                          unsigned *ovf, unsigned long long *counters, hipStream_t s) {
    if (!G) return hipSuccess;
    const unsigned grid = (G + kWalkWaves - 1) / kWalkWaves;
    hipLaunchKernelGGL(k_ib_walk, dim3(grid), dim3(kWalkThreads), 0, s, buf, lo, hi, chunk, w0, nw, G, cap_w, mode, ns,
                       ld, codes, static_cast<IbMeta *>(meta), cnt, ovf, counters);
    return hipGetLastError();
}

hipError_t launch_ib_lines(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint32_t n,
                           int mode, uint32_t ns, uint32_t ld, int8_t *codes, void *meta, uint32_t *cnt,
                           unsigned long long *counters, hipStream_t s) {
    if (!n) return hipSuccess;
    const unsigned grid = std::min<unsigned>((n + 3) / 4, 4096);
    hipLaunchKernelGGL(k_ib_lines, dim3(grid), dim3(256), 0, s, buf, data_start, line_end, l0, n, mode, ns, ld, codes,
                       static_cast<IbMeta *>(meta), cnt, counters);
    return hipGetLastError();
}

size_t ib_rec_bytes() { return sizeof(IbRec); }

hipError_t launch_ib_table(const void *meta, const uint32_t *cnt, uint32_t *offs, uint32_t G, uint32_t cap_w,
                           int global_freq, void *rec, hipStream_t s) {
    const uint64_t slots = (uint64_t)G * cap_w;
    if (!slots) return hipSuccess;
    hipLaunchKernelGGL(k_ib_scan, dim3(1), dim3(256), 0, s, cnt, G, offs);
    hipLaunchKernelGGL(k_ib_table, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s,
                       static_cast<const IbMeta *>(meta), cnt, offs, G, cap_w, global_freq, static_cast<IbRec *>(rec));
    return hipGetLastError();
}

size_t ib_packed_bytes(uint64_t slots, uint32_t ns) {
    return (size_t)((ns + kWave - 1) / kWave) * ((slots + kIbGroup - 1) / kIbGroup) * kWave * 16;
}

hipError_t launch_ib_pack(const int8_t *codes, uint32_t ld, const void *rec, const uint32_t *n_rec, uint64_t slots,
                          void *packed, uint32_t ns, hipStream_t s) {
    if (!ns || !slots) return hipSuccess;
    const uint32_t ng = (uint32_t)((slots + kIbGroup - 1) / kIbGroup), tiles = (ns + kWave - 1) / kWave;
    hipLaunchKernelGGL(k_ib_pack, dim3(ng, (tiles + 3) / 4), dim3(256), 0, s, codes, ld, static_cast<const IbRec *>(rec),
                       n_rec, ns, ng, static_cast<uint4 *>(packed));
    return hipGetLastError();
}

hipError_t launch_ib_chain(const void *rec, const uint32_t *n_rec, uint64_t slots, const void *packed, uint32_t ns,
                           int mode, int skip_boundary, int count_boundary, double *sum_exp, uint64_t *obs_het,
                           uint64_t *used, int32_t *carried, hipStream_t s) {
    if (!ns || !slots) return hipSuccess;
    const uint32_t ng = (uint32_t)((slots + kIbGroup - 1) / kIbGroup), tiles = (ns + kWave - 1) / kWave;
    hipLaunchKernelGGL(k_ib_chain, dim3(tiles), dim3(kWave), 0, s, static_cast<const uint4 *>(packed), ng,
                       static_cast<const IbRec *>(rec), n_rec, ns, mode, skip_boundary, count_boundary, sum_exp,
                       obs_het, used, carried);
    return hipGetLastError();
}

hipError_t launch_ib_rows(const double *sum_exp, const uint64_t *obs_het, const uint64_t *used, uint32_t ns,
                          const char *names, const uint64_t *noff, char *out, uint64_t *text_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_ib_rows, dim3(1), dim3(kIbRowThreads), 0, s, sum_exp, obs_het, used, ns, names, noff, out,
                       text_bytes);
    return hipGetLastError();
}

}  // namespace vcfxg
