// vcfxg_srt.hip -- VCFX_sorter (VCFX_sorter.cpp: sortFileMmap :321-459 file mode, sortExternal
// :601-674 stdin mode): the '#' lines in input order, then the kept data lines ordered by
// (CHROM, POS).  Equal keys keep their input order (the reference leaves them as its C++ library's
// unstable sort does: the one documented difference, DESIGN.md "Sorting").
//
// The passes over the indexed lines (the scans and the radix sort between them are hipcub's,
// vcfxg_api_srt.hip):
//   k_srt_key    a lane per line over its first kSrtWindow bytes: the first tab (stdin mode: the
//                first two) from 16 B loads, then POS and the CHROM key from those few bytes.  A
//                line whose tabs are not inside the window is queued for k_srt_key_wave, a wave per
//                line (head_tabs), so a CHROM of any length passes.
//   k_srt_class  file mode's data lines before the first "#CHROM" line (a max-reduction of L - li
//                in the key pass) become PRE; the written flag; the status counts; the longest
//                kept CHROM.
//   k_srt_scatter  (first-pass key, line) of the written lines, compacted in line order.
//   (sort)       natural order: one stable 64-bit sort of (id, POS).  Lexicographic: least
//                significant part first: (CHROM length, POS) in one word, then CHROM's 8-byte
//                words from the last to the first (k_srt_word gathers each through the
//                permutation so far).  A header line's keys are all 0 and a data line's length
//                word is length + 1, so the header block sorts first and keeps its order.
//   k_srt_len    output line j's bytes (with its '\n') and its first input byte; their scan places
//                every line.
//   k_srt_gather the text: every wave owns aligned 16 KiB (short texts: 4 KiB) spans of the output, finds the lines of a
//                span by a search in the offsets (from a proportional guess), and each lane builds 16 output bytes from the
//                pieces of the lines that cover them (two aligned 16 B loads realigned with
//                v_alignbyte_b32 per piece) and writes them with one aligned 16 B store.
//
// chromToId (:43-146) is restated in srt_chrom_id with its 32-bit wrap.
#include <algorithm>

#include "vcfxg_device.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kSrtThreads = 256;
constexpr int kSrtWaves = kSrtThreads / kWave;
// wave-steps of 1 KiB per span, the output bytes a wave takes at a time: 16 for a text of
// kSrtLongText bytes or more (fewer span searches per byte: 2 to 9 % on the bench shard), else 4 (a
// 20 MB text then still makes 5,000 spans: 0.041 ms against 0.091 ms with 16)
constexpr int kSrtSpanSteps = 16, kSrtSpanStepsShort = 4;
constexpr uint64_t kSrtLongText = 64ull << 20;

struct SrtArgs {
    const char *buf;
    int64_t data_start;
    const uint64_t *line_end;
    uint64_t L;
    int stdin_mode, natural;
};

__device__ __forceinline__ int64_t srt_line_start(const uint64_t *line_end, int64_t data_start, uint64_t li) {
    return li ? (int64_t)line_end[li - 1] + 1 : data_start;
}

__device__ __forceinline__ bool srt_digit(uint32_t b) { return b - '0' <= 9u; }
__device__ __forceinline__ uint32_t srt_upper(uint32_t b) { return b - 'a' <= 25u ? b - 32u : b; }

// chromToId(chrom, len, true) :43-146; int arithmetic wraps at 32 bits
__device__ __forceinline__ int32_t srt_chrom_id(const char *__restrict__ buf, int64_t s, int64_t len) {
    if (len == 0) return 999999;
    int64_t p = s, rem = len;
    bool prefix = false;
    uint32_t c0 = byte_at(buf, s), c1 = 0;
    if (rem >= 3) {
        c1 = byte_at(buf, s + 1);
        const uint32_t c2 = byte_at(buf, s + 2);
        if ((c0 == 'c' || c0 == 'C') && (c1 == 'h' || c1 == 'H') && (c2 == 'r' || c2 == 'R')) {
            p += 3;
            rem -= 3;
            prefix = true;
        }
    }
    if (rem == 0) return 999999;
    uint32_t num = 0;
    int64_t nd = 0;
    while (nd < rem && srt_digit(byte_at(buf, p + nd))) {
        num = num * 10u + (byte_at(buf, p + nd) - '0');
        nd++;
    }
    uint32_t sh = 0;
    if (nd < rem) {
        for (int64_t i = nd; i < rem && i < nd + 8; i++) sh = sh * 31u + byte_at(buf, p + i);
        sh = (sh & 0x7FFFu) + 1u;
    }
    uint32_t off = 0, base = 0;
    if (prefix) {
        base = 5000000u;
        off = c0 == 'C' && c1 == 'H' && byte_at(buf, s + 2) == 'R' ? 10000u : c0 == 'C' && c1 == 'h' ? 20000u : 30000u;
    }
    if (nd > 0 && (int32_t)num >= 1 && (int32_t)num <= 22) return (int32_t)(base + num * 100000u + off + sh);
    if (nd == 0) {
        const uint32_t u0 = srt_upper(byte_at(buf, p));
        if (rem >= 2 && u0 == 'M' && srt_upper(byte_at(buf, p + 1)) == 'T') {
            if (rem > 2) {
                sh = 0;
                for (int64_t i = 2; i < rem && i < 10; i++) sh = sh * 31u + byte_at(buf, p + i);
                sh = (sh & 0x7FFFu) + 1u;
            }
            return (int32_t)(base + 2300000u + off + sh);
        }
        if (rem == 1) {
            if (u0 == 'M') return (int32_t)(base + 2300000u + off + sh);
            if (u0 == 'X') return (int32_t)(base + 2400000u + off + sh);
            if (u0 == 'Y') return (int32_t)(base + 2500000u + off + sh);
        }
    }
    uint32_t h = 3000000u;
    for (int64_t i = 0; i < len && i < 16; i++) h = h * 31u + byte_at(buf, s + i);
    return (int32_t)(base + ((h & 0x3FFFFFFFu) + 3000000u));
}

// File mode's POS (parseChromPosFast :249-270): the digits from s on, accumulated in a wrapping int;
// kept unless that is 0.  (The source tests `pos > 0`; the compiled reference keeps a value that
// wrapped negative and sorts it as a negative int, since a sum of digits cannot be negative to its
// compiler.  The recorded cases hold both to that.)
__device__ __forceinline__ bool srt_pos_file(const char *__restrict__ buf, int64_t s, int64_t le, int32_t &pos) {
    uint32_t v = 0, b;
    for (int64_t p = s; p < le && (b = byte_at(buf, p) - '0') <= 9u; p++) v = v * 10u + b;
    pos = (int32_t)v;
    return pos != 0;
}

// Stdin mode's POS (parseChromPos :231-246): std::stoi of the field [s, fe): C white space skipped,
// one sign, digits, the rest ignored; no digits or a value outside int fails.
__device__ __forceinline__ bool srt_pos_stdin(const char *__restrict__ buf, int64_t s, int64_t fe, int32_t &pos) {
    int64_t p = s;
    uint32_t b = 0;
    while (p < fe && ((b = byte_at(buf, p)) == ' ' || (b >= 9u && b <= 13u))) p++;
    bool neg = false;
    if (p < fe && ((b = byte_at(buf, p)) == '-' || b == '+')) {
        neg = b == '-';
        p++;
    }
    const uint64_t lim = neg ? (1ull << 31) : (1ull << 31) - 1u;
    uint64_t v = 0;
    bool any = false, ovf = false;
    while (p < fe && (b = byte_at(buf, p) - '0') <= 9u) {
        any = true;
        if (!ovf) {
            v = v * 10u + b;
            ovf = v > lim;
        }
        p++;
    }
    if (!any || ovf) return false;
    pos = (int32_t)(uint32_t)(neg ? 0u - v : v);
    return true;
}

// CHROM's bytes [8 w, 8 w + 8) big-endian, zero-padded past its end
__device__ __forceinline__ uint64_t srt_chrom_word(const char *__restrict__ buf, int64_t s, int64_t len, uint32_t w) {
    uint64_t x = 0;
    const int64_t a = 8 * (int64_t)w;
#pragma unroll
    for (int i = 0; i < 8; i++) x = (x << 8) | (a + i < len ? (uint64_t)byte_at(buf, s + a + i) : 0ull);
    return x;
}

struct SrtLine {
    uint64_t w0;
    int32_t pos;
    uint32_t aux;
    uint8_t st;
};

// the data line [ls, le) with its first tab at t0 and, in stdin mode, the field's end at t1
// (-1: the line has no such tab)
__device__ __forceinline__ void srt_parse(const SrtArgs &A, int64_t ls, int64_t le, int64_t t0, int64_t t1, SrtLine &o) {
    o.st = kSrtBad;
    if (t0 < 0 || (A.stdin_mode && t1 < 0)) return;
    const bool ok = A.stdin_mode ? srt_pos_stdin(A.buf, t0 + 1, t1, o.pos) : srt_pos_file(A.buf, t0 + 1, le, o.pos);
    if (!ok) return;
    o.st = kSrtKept;
    if (A.natural) {
        o.aux = (uint32_t)srt_chrom_id(A.buf, ls, t0 - ls);
    } else {
        o.aux = (uint32_t)(t0 - ls);
        o.w0 = srt_chrom_word(A.buf, ls, t0 - ls, 0);
    }
}

__device__ __forceinline__ void srt_store(uint64_t li, const SrtLine &o, int natural, uint8_t *status, int32_t *pos,
                                          uint32_t *aux, uint64_t *w0) {
    status[li] = o.st;
    pos[li] = o.pos;
    aux[li] = o.aux;
    if (!natural) w0[li] = o.w0;
}

__device__ __forceinline__ bool srt_is_chrom(const char *__restrict__ buf, int64_t ls, int64_t le) {
    return le - ls >= 6 && byte_at(buf, ls + 1) == 'C' && byte_at(buf, ls + 2) == 'H' && byte_at(buf, ls + 3) == 'R' &&
           byte_at(buf, ls + 4) == 'O' && byte_at(buf, ls + 5) == 'M';
}

// The lane pass; a line it does not settle goes to queue[counters[5]++] for k_srt_key_wave.
__global__ __launch_bounds__(kSrtThreads) void k_srt_key(SrtArgs A, uint8_t *__restrict__ status, int32_t *__restrict__ pos,
                                                         uint32_t *__restrict__ aux, uint64_t *__restrict__ w0,
                                                         uint32_t *__restrict__ queue,
                                                         unsigned long long *__restrict__ counters) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    const int want = A.stdin_mode ? 2 : 1;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < A.L; li += nth) {
        const int64_t ls = srt_line_start(A.line_end, A.data_start, li), le = (int64_t)A.line_end[li];
        SrtLine o;
        o.w0 = 0;
        o.pos = 0;
        o.aux = 0;
        o.st = kSrtEmpty;
        bool have = true;
        if (le > ls) {
            if (byte_at(A.buf, ls) == '#') {
                o.st = kSrtHeader;
                if (srt_is_chrom(A.buf, ls, le)) atomicMax(&counters[6], (unsigned long long)(A.L - li));
            } else {
                const int64_t we = le - ls > kSrtWindow ? ls + kSrtWindow : le;
                int64_t t[2] = {-1, -1};
                int nt = 0;
                for (int64_t a = ls & ~(int64_t)15; a < we && nt < want; a += 16) {
                    uint32_t m = eq_mask16(load16(A.buf, a), kRepTab) & range_mask16(a, ls, we);
                    while (m && nt < want) {
                        t[nt++] = a + __builtin_ctz(m);
                        m &= m - 1u;
                    }
                }
                if (nt < want && we < le) have = false;  // the window ended before the key fields did
                else srt_parse(A, ls, le, t[0], t[1], o);
            }
        }
        if (have) srt_store(li, o, A.natural, status, pos, aux, w0);
        else queue[atomicAdd(&counters[5], 1ull)] = (uint32_t)li;
    }
}

// The wave pass over the queued lines (counters[5] of them), a wave per line: the tabs by the
// whole wave, the fields by every lane alike.
__global__ __launch_bounds__(kSrtThreads) void k_srt_key_wave(SrtArgs A, uint8_t *__restrict__ status,
                                                              int32_t *__restrict__ pos, uint32_t *__restrict__ aux,
                                                              uint64_t *__restrict__ w0, const uint32_t *__restrict__ queue,
                                                              const unsigned long long *__restrict__ counters) {
    __shared__ int64_t s_tabs[kSrtWaves][10];
    const uint64_t nq = counters[5];
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t q = wid; q < nq; q += nw) {
        const uint64_t li = (uint64_t)uniform32((int)queue[q]);
        const int64_t ls = uniform64(srt_line_start(A.line_end, A.data_start, li)), le = uniform64((int64_t)A.line_end[li]);
        int64_t t[2] = {-1, -1};
        const int nt = head_tabs(A.buf, ls, le, A.stdin_mode ? 2 : 1, t, s_tabs[threadIdx.x / kWave]);
        SrtLine o;
        o.w0 = 0;
        o.pos = 0;
        o.aux = 0;
        srt_parse(A, ls, le, nt > 0 ? t[0] : -1, nt > 1 ? t[1] : -1, o);
        if (lane() == 0) srt_store(li, o, A.natural, status, pos, aux, w0);
    }
}

// PRE, the written flag, the status counts (counters[0..4]) and the longest kept CHROM (counters[7])
__global__ __launch_bounds__(kSrtThreads) void k_srt_class(uint64_t L, int stdin_mode, int natural, uint8_t *__restrict__ status,
                                                           const uint32_t *__restrict__ aux, uint32_t *__restrict__ written,
                                                           unsigned long long *__restrict__ counters) {
    __shared__ unsigned int red[6];
    if (threadIdx.x < 6) red[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t first_chrom = L - (uint64_t)counters[6];  // (L without one)
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    uint32_t k[5] = {0, 0, 0, 0, 0}, longest = 0;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < L; li += nth) {
        uint8_t st = status[li];
        if (!stdin_mode && li < first_chrom && (st == kSrtKept || st == kSrtBad)) {
            st = kSrtPre;
            status[li] = st;
        }
        written[li] = st == kSrtHeader || st == kSrtKept || (stdin_mode && st == kSrtEmpty) ? 1u : 0u;
        if (st == kSrtKept && !natural) longest = max(longest, aux[li]);
#pragma unroll
        for (int i = 0; i < 5; i++) k[i] += st == i ? 1u : 0u;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const uint32_t t = wave_sum(k[i]);
        if (lane() == 0 && t) atomicAdd(&red[i], t);
    }
    if (longest) atomicMax(&red[5], longest);
    __syncthreads();
    if (threadIdx.x < 5 && red[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)red[threadIdx.x]);
    if (threadIdx.x == 5 && red[5]) atomicMax(&counters[7], (unsigned long long)red[5]);
}

__device__ __forceinline__ uint32_t srt_flip(int32_t v) { return (uint32_t)v ^ 0x80000000u; }

__global__ __launch_bounds__(kSrtThreads) void k_srt_scatter(uint64_t L, int stdin_mode, int natural,
                                                             const uint8_t *__restrict__ status,
                                                             const uint32_t *__restrict__ written,
                                                             const uint64_t *__restrict__ ord, const int32_t *__restrict__ pos,
                                                             const uint32_t *__restrict__ aux, uint64_t *__restrict__ keys,
                                                             uint32_t *__restrict__ vals) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < L; li += nth) {
        if (!written[li]) continue;
        uint64_t key = 0;
        if (status[li] == kSrtKept) {
            const uint32_t a = aux[li];
            const uint32_t hi = natural ? srt_flip((int32_t)a) : (stdin_mode && a == 0) ? 0xFFFFFFFFu : a + 1u;
            key = ((uint64_t)hi << 32) | srt_flip(pos[li]);
        }
        keys[ord[li]] = key;
        vals[ord[li]] = (uint32_t)li;
    }
}

__global__ __launch_bounds__(kSrtThreads) void k_srt_word(const char *__restrict__ buf, int64_t data_start,
                                                          const uint64_t *__restrict__ line_end, uint64_t nw, int stdin_mode,
                                                          uint32_t w, uint32_t shift, const uint32_t *__restrict__ vals,
                                                          const uint8_t *__restrict__ status, const uint32_t *__restrict__ aux,
                                                          const uint64_t *__restrict__ w0, uint64_t *__restrict__ keys) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= nw) return;
    const uint32_t li = vals[j];
    uint64_t key = 0;
    if (status[li] == kSrtKept) {
        const uint32_t len = aux[li];
        if (stdin_mode && len == 0) key = ~0ull;
        else if (w == 0) key = w0[li];
        else if (8ull * w < len) key = srt_chrom_word(buf, srt_line_start(line_end, data_start, li), len, w);
    }
    keys[j] = key >> shift;
}

__global__ __launch_bounds__(kSrtThreads) void k_srt_len(int64_t data_start, const uint64_t *__restrict__ line_end, uint64_t nw,
                                                         const uint32_t *__restrict__ order, uint64_t *__restrict__ len,
                                                         uint64_t *__restrict__ src) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j > nw) return;
    if (j == nw) {
        len[j] = 0;
        return;
    }
    const uint32_t li = order[j];
    const int64_t ls = srt_line_start(line_end, data_start, li);
    len[j] = (uint64_t)((int64_t)line_end[li] - ls) + 1u;
    src[j] = (uint64_t)ls;
}

// ---- the gather --------------------------------------------------------------------------------

// the last j in [lo, hi] with off[j] <= g (off[lo] <= g)
__device__ __forceinline__ uint64_t srt_find(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t g) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the same from a guess: gallop away from it, then the search in what is left (lines of like
// lengths put the guess within a few lines: a handful of dependent loads, not log2 of all lines)
__device__ __forceinline__ uint64_t srt_find_near(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t g,
                                                  uint64_t guess) {
    uint64_t j = guess < lo ? lo : guess > hi ? hi : guess;
    uint64_t step = 1;
    if (off[j] <= g) {
        while (j + step <= hi && off[j + step] <= g) {
            j += step;
            step <<= 1;
        }
        return srt_find(off, j, j + step < hi ? j + step : hi, g);
    }
    uint64_t top;  // (off[lo] <= g < off[j]: j > lo)
    do {
        top = j - 1;
        j = j - lo > step ? j - step : lo;
        step <<= 1;
    } while (off[j] > g);
    return srt_find(off, j, top, g);
}

template <bool kNt>
__device__ __forceinline__ uint4 srt_load16(const char *buf, int64_t a) {
    const uint4 *p = reinterpret_cast<const uint4 *>(buf + a);
    if (kNt) {
        typedef uint32_t v4 __attribute__((ext_vector_type(4)));
        const v4 v = __builtin_nontemporal_load(reinterpret_cast<const v4 *>(p));
        return uint4{v.x, v.y, v.z, v.w};
    }
    return *p;
}

// the 16 bytes at input offset s (any alignment, s >= 0): two aligned loads, v_alignbyte_b32
template <bool kNt>
__device__ __forceinline__ uint4 srt_bytes16(const char *buf, int64_t s) {
    const int64_t a = s & ~(int64_t)15;
    const uint4 A = srt_load16<kNt>(buf, a);
    const uint32_t sh = (uint32_t)(s & 15);
    if (sh == 0) return A;
    const uint4 B = srt_load16<kNt>(buf, a + 16);
    const uint32_t d = sh >> 2, b = sh & 3u;
    const uint32_t x0 = d == 0 ? A.x : d == 1 ? A.y : d == 2 ? A.z : A.w;
    const uint32_t x1 = d == 0 ? A.y : d == 1 ? A.z : d == 2 ? A.w : B.x;
    const uint32_t x2 = d == 0 ? A.z : d == 1 ? A.w : d == 2 ? B.x : B.y;
    const uint32_t x3 = d == 0 ? A.w : d == 1 ? B.x : d == 2 ? B.y : B.z;
    const uint32_t x4 = d == 0 ? B.x : d == 1 ? B.y : d == 2 ? B.z : B.w;
    return uint4{__builtin_amdgcn_alignbyte(x1, x0, b), __builtin_amdgcn_alignbyte(x2, x1, b),
                 __builtin_amdgcn_alignbyte(x3, x2, b), __builtin_amdgcn_alignbyte(x4, x3, b)};
}

// v's bytes [t0, t1) replaced by c's
__device__ __forceinline__ void srt_merge(uint4 &v, const uint4 &c, int t0, int t1) {
    const uint32_t m = range16(0, t0, t1);
    const uint32_t m0 = nib_bytes(m & 0xFu), m1 = nib_bytes((m >> 4) & 0xFu), m2 = nib_bytes((m >> 8) & 0xFu),
                   m3 = nib_bytes((m >> 12) & 0xFu);
    v.x = (v.x & ~m0) | (c.x & m0);
    v.y = (v.y & ~m1) | (c.y & m1);
    v.z = (v.z & ~m2) | (c.z & m2);
    v.w = (v.w & ~m3) | (c.w & m3);
}

// Output lines [first, first + k) as text bytes [0, bytes): text byte o is output byte base + o,
// base = off[first].  A wave takes spans of `steps` KiB; lane i of step s builds the 16 bytes
// at o = span + 1024 s + 16 i: the line that holds byte o by a search between the span's first and
// last line (found once per span, wave-uniform), then piece after piece (a line's bytes, its '\n') until the 16 are full or the lines
// end.  Every store is one aligned 16 B store; the bytes past `bytes` in the last one are zero.
template <int kNtMode>
__global__ __launch_bounds__(kSrtThreads) void k_srt_gather(const char *__restrict__ buf, const uint64_t *__restrict__ off,
                                                            const uint64_t *__restrict__ src, uint64_t first, uint64_t k,
                                                            uint64_t bytes, int steps, char *__restrict__ text) {
    constexpr bool kNtLoad = (kNtMode & 1) != 0, kNtStore = (kNtMode & 2) != 0;
    const uint64_t last = first + k - 1;  // the block's last line
    const uint64_t base = off[first];
    const uint64_t span = (uint64_t)steps * kWaveStep;
    const uint64_t nspans = (bytes + span - 1) / span;
    const double per_byte = (double)k / (double)bytes;  // lines per output byte: the searches' guess
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nwaves = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t sp = wid; sp < nspans; sp += nwaves) {
        const uint64_t o0 = sp * span;
        const uint64_t o1 = min(o0 + span, bytes);  // (o0 < bytes)
        const uint64_t j0 = (uint64_t)uniform64((int64_t)srt_find_near(off, first, last, base + o0, first + (uint64_t)((double)o0 * per_byte)));
        const uint64_t j1 = (uint64_t)uniform64((int64_t)srt_find_near(off, j0, last, base + o1 - 1, j0 + (uint64_t)((double)(o1 - o0) * per_byte)));
        for (int s = 0; s < steps; s++) {
            const uint64_t o = o0 + (uint64_t)s * kWaveStep + (uint64_t)lane() * 16u;
            if (o >= o1) continue;
            const uint64_t g = base + o;
            uint64_t j = j0 == j1 ? j0 : srt_find(off, j0, j1, g);
            uint4 v = uint4{0u, 0u, 0u, 0u};
            int t = 0;
            while (t < 16 && j <= last) {
                const uint64_t a = off[j], e = off[j + 1];  // output bytes [a, e): the line, then '\n' at e - 1
                const int64_t q = (int64_t)(g + (uint64_t)t - a);  // the piece starts at line byte q
                const int64_t body = (int64_t)(e - 1 - a) - q;   // line bytes from there on (>= 0)
                const int t1 = body < 16 - t ? t + (int)body : 16;
                if (t1 > t) {
                    const int64_t sv = (int64_t)src[j] + q - t;  // text byte t of this chunk = input byte sv + t
                    if (sv >= 0) {
                        srt_merge(v, srt_bytes16<kNtLoad>(buf, sv), t, t1);
                    } else {  // (a line within the input's first 15 bytes)
                        for (int i = t; i < t1; i++) {
                            const uint4 c = uint4{byte_at(buf, sv + i) * 0x01010101u, byte_at(buf, sv + i) * 0x01010101u,
                                                  byte_at(buf, sv + i) * 0x01010101u, byte_at(buf, sv + i) * 0x01010101u};
                            srt_merge(v, c, i, i + 1);
                        }
                    }
                }
                t = t1;
                if (t < 16) {
                    srt_merge(v, uint4{kRepNl, kRepNl, kRepNl, kRepNl}, t, t + 1);
                    t++;
                    j++;
                }
            }
            uint4 *dst = reinterpret_cast<uint4 *>(text + o);
            if (kNtStore) {
                typedef uint32_t v4 __attribute__((ext_vector_type(4)));
                v4 x;
                x.x = v.x, x.y = v.y, x.z = v.z, x.w = v.w;
                __builtin_nontemporal_store(x, reinterpret_cast<v4 *>(dst));
            } else {
                *dst = v;
            }
        }
    }
}

// ---- launchers ---------------------------------------------------------------------------------

static unsigned srt_grid(uint64_t items, uint64_t per_block, unsigned max_blocks) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, max_blocks));
}

hipError_t launch_srt_key(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t L, int stdin_mode,
                          int natural, uint8_t *status, int32_t *pos, uint32_t *aux, uint64_t *w0, uint32_t *queue,
                          unsigned long long *counters, hipStream_t s) {
    if (!L) return hipSuccess;
    const SrtArgs A{buf, data_start, line_end, L, stdin_mode ? 1 : 0, natural ? 1 : 0};
    hipLaunchKernelGGL(k_srt_key, dim3(srt_grid(L, kSrtThreads, 8192)), dim3(kSrtThreads), 0, s, A, status, pos, aux, w0,
                       queue, counters);
    hipLaunchKernelGGL(k_srt_key_wave, dim3(srt_grid(L, kSrtWaves, 2048)), dim3(kSrtThreads), 0, s, A, status, pos, aux, w0,
                       queue, counters);
    return hipGetLastError();
}

hipError_t launch_srt_class(uint64_t L, int stdin_mode, int natural, uint8_t *status, const uint32_t *aux,
                            uint32_t *written, unsigned long long *counters, hipStream_t s) {
    if (!L) return hipSuccess;
    hipLaunchKernelGGL(k_srt_class, dim3(srt_grid(L, kSrtThreads * 4, 1024)), dim3(kSrtThreads), 0, s, L, stdin_mode ? 1 : 0,
                       natural ? 1 : 0, status, aux, written, counters);
    return hipGetLastError();
}

hipError_t launch_srt_scatter(uint64_t L, int stdin_mode, int natural, const uint8_t *status, const uint32_t *written,
                              const uint64_t *ord, const int32_t *pos, const uint32_t *aux, uint64_t *keys,
                              uint32_t *vals, hipStream_t s) {
    if (!L) return hipSuccess;
    hipLaunchKernelGGL(k_srt_scatter, dim3(srt_grid(L, kSrtThreads, 8192)), dim3(kSrtThreads), 0, s, L, stdin_mode ? 1 : 0,
                       natural ? 1 : 0, status, written, ord, pos, aux, keys, vals);
    return hipGetLastError();
}

hipError_t launch_srt_word(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t nw, int stdin_mode,
                           uint32_t w, uint32_t shift, const uint32_t *vals, const uint8_t *status, const uint32_t *aux,
                           const uint64_t *w0, uint64_t *keys, hipStream_t s) {
    if (!nw) return hipSuccess;
    hipLaunchKernelGGL(k_srt_word, dim3((unsigned)((nw + kSrtThreads - 1) / kSrtThreads)), dim3(kSrtThreads), 0, s, buf,
                       data_start, line_end, nw, stdin_mode ? 1 : 0, w, shift, vals, status, aux, w0, keys);
    return hipGetLastError();
}

hipError_t launch_srt_len(int64_t data_start, const uint64_t *line_end, uint64_t nw, const uint32_t *order,
                          uint64_t *len, uint64_t *src, hipStream_t s) {
    hipLaunchKernelGGL(k_srt_len, dim3((unsigned)((nw + 1 + kSrtThreads - 1) / kSrtThreads)), dim3(kSrtThreads), 0, s,
                       data_start, line_end, nw, order, len, src);
    return hipGetLastError();
}

hipError_t launch_srt_gather(const char *buf, const uint64_t *off, const uint64_t *src, uint64_t first, uint64_t k,
                             uint64_t bytes, int nt, char *text, hipStream_t s) {
    if (!k || !bytes) return hipSuccess;
    const int steps = bytes >= kSrtLongText ? kSrtSpanSteps : kSrtSpanStepsShort;
    const uint64_t spans = (bytes + (uint64_t)steps * kWaveStep - 1) / ((uint64_t)steps * kWaveStep);
    const dim3 grid(srt_grid(spans, kSrtWaves, 4096)), block(kSrtThreads);
    switch (nt & 3) {
        case 1: hipLaunchKernelGGL(k_srt_gather<1>, grid, block, 0, s, buf, off, src, first, k, bytes, steps, text); break;
        case 2: hipLaunchKernelGGL(k_srt_gather<2>, grid, block, 0, s, buf, off, src, first, k, bytes, steps, text); break;
        case 3: hipLaunchKernelGGL(k_srt_gather<3>, grid, block, 0, s, buf, off, src, first, k, bytes, steps, text); break;
        default: hipLaunchKernelGGL(k_srt_gather<0>, grid, block, 0, s, buf, off, src, first, k, bytes, steps, text); break;
    }
    return hipGetLastError();
}

}  // namespace vcfxg
