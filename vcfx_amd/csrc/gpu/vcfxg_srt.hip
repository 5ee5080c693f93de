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
//   The output lines are placed and gathered by vcfxg_gather.hip (launch_line_len, launch_text_gather).
//
// chromToId (:43-146) is restated in srt_chrom_id with its 32-bit wrap.  The leaf functions the keyed
// tools share (line_start, key_word, window_tabs, parse_c_integer, tally_status) are vcfxg_keyed.h's.
#include "vcfxg_keyed.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kSrtThreads = 256;
constexpr int kSrtWaves = kSrtThreads / kWave;

struct SrtArgs {
    const char *buf;
    int64_t data_start;
    const uint64_t *line_end;
    uint64_t L;
    int stdin_mode, natural;
};

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
    const CInteger v = parse_c_integer(buf, s, fe);
    if (!v.any || !v.fits_int()) return false;
    pos = (int32_t)(uint32_t)v.bits();
    return true;
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
        o.w0 = key_word(A.buf, ls, t0 - ls, 0);
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
        const int64_t ls = line_start(A.line_end, A.data_start, li), le = (int64_t)A.line_end[li];
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
                int64_t t[2] = {-1, -1};
                const int nt = window_tabs<2>(A.buf, ls, le, kSrtWindow, t, want);
                if (nt < want && le - ls > kSrtWindow) have = false;  // the window ended before the key fields did
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
        const int64_t ls = uniform64(line_start(A.line_end, A.data_start, li)), le = uniform64((int64_t)A.line_end[li]);
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
    if (longest) atomicMax(&red[5], longest);
    tally_status(k, red, counters);
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
        else if (8ull * w < len) key = key_word(buf, line_start(line_end, data_start, li), len, w);
    }
    keys[j] = key >> shift;
}

// ---- launchers ---------------------------------------------------------------------------------

hipError_t launch_srt_key(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t L, int stdin_mode,
                          int natural, uint8_t *status, int32_t *pos, uint32_t *aux, uint64_t *w0, uint32_t *queue,
                          unsigned long long *counters, hipStream_t s) {
    if (!L) return hipSuccess;
    const SrtArgs A{buf, data_start, line_end, L, stdin_mode ? 1 : 0, natural ? 1 : 0};
    hipLaunchKernelGGL(k_srt_key, dim3(grid_for(L, kSrtThreads, 8192)), dim3(kSrtThreads), 0, s, A, status, pos, aux, w0,
                       queue, counters);
    hipLaunchKernelGGL(k_srt_key_wave, dim3(grid_for(L, kSrtWaves, 2048)), dim3(kSrtThreads), 0, s, A, status, pos, aux, w0,
                       queue, counters);
    return hipGetLastError();
}

hipError_t launch_srt_class(uint64_t L, int stdin_mode, int natural, uint8_t *status, const uint32_t *aux,
                            uint32_t *written, unsigned long long *counters, hipStream_t s) {
    if (!L) return hipSuccess;
    hipLaunchKernelGGL(k_srt_class, dim3(grid_for(L, kSrtThreads * 4, 1024)), dim3(kSrtThreads), 0, s, L, stdin_mode ? 1 : 0,
                       natural ? 1 : 0, status, aux, written, counters);
    return hipGetLastError();
}

hipError_t launch_srt_scatter(uint64_t L, int stdin_mode, int natural, const uint8_t *status, const uint32_t *written,
                              const uint64_t *ord, const int32_t *pos, const uint32_t *aux, uint64_t *keys,
                              uint32_t *vals, hipStream_t s) {
    if (!L) return hipSuccess;
    hipLaunchKernelGGL(k_srt_scatter, dim3(grid_for(L, kSrtThreads, 8192)), dim3(kSrtThreads), 0, s, L, stdin_mode ? 1 : 0,
                       natural ? 1 : 0, status, written, ord, pos, aux, keys, vals);
    return hipGetLastError();
}

hipError_t launch_srt_word(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t nw, int stdin_mode,
                           uint32_t w, uint32_t shift, const uint32_t *vals, const uint8_t *status, const uint32_t *aux,
                           const uint64_t *w0, uint64_t *keys, hipStream_t s) {
    if (!nw) return hipSuccess;
    hipLaunchKernelGGL(k_srt_word, flat_grid(nw, kSrtThreads), dim3(kSrtThreads), 0, s, buf,
                       data_start, line_end, nw, stdin_mode ? 1 : 0, w, shift, vals, status, aux, w0, keys);
    return hipGetLastError();
}

}  // namespace vcfxg
