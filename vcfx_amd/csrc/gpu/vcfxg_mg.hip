// vcfxg_mg.hip -- VCFX_merger (VCFX_merger.cpp: parseChromPos :77-92, parseChromNat :43-74, the
// comparators :17-40 and :223-248, mergeVCFInMemory :176-254, mergeVCFStreaming :257-345): the lines
// of K files, joined into one indexed text, in key order.  Equal keys come out in (file list order,
// line order) (the reference leaves them to std::sort and to its heap: the one documented
// difference, DESIGN.md "Merge").
//
// The passes (the scans and the radix sort between them are hipcub's, vcfxg_api_mg.hip):
//   k_mg_cut     per file the first line that starts at or after the file's first byte.
//   k_mg_key     a lane per line over its first kMgWindow bytes: its file (a search in the first
//                lines), the two tabs from 16 B loads, then POS by std::stol's rule with the exact
//                64-bit overflow test, and the key string's descriptor: where it starts, its length
//                and its first eight bytes big-endian (CHROM; with -n the suffix after the "chr"
//                prefix and the digit run, with the prefix word and the run's value beside it).  A
//                line whose second tab is not inside the window (and that is longer than it) is
//                queued for k_mg_key_wave, a wave per line (head_tabs), so a CHROM and a run of
//                zeros of any length pass.  Each file's first '#' line and first line that is
//                neither empty nor '#' are min-reduced (only a line whose predecessor is of another
//                class tries).
//   k_mg_hdr     the first file that has a header candidate under the mode's rule.
//   k_mg_class   every '#' line HEADER (written) or DROPPED; the written flag; the status counts,
//                BAD per file, the longest key string of a kept line.
//   mg_cmp       the comparator over two lines' descriptors; it reads input bytes only past the
//                cached word (cmp_bytes from byte 8; vcfxg_keyed.h, with line_start, key_word,
//                window_tabs, parse_c_integer and tally_status).
//   sort path    k_mg_scatter: the written lines compacted in line order; k_mg_part: one part of the
//                key per stable LSD pass: POS (sign flipped), the key string's length + 1, its
//                8-byte words from the last to the first; with -n then the digit run's value and
//                (prefix word, numeric class).  A header line's parts are all 0: the header block
//                sorts first and keeps its order.
//   walk path    (-s with a file out of order: k_mg_ordered) k_mg_walk is the reference's heap
//                process run by one wave: lanes stride the files, each keeps the least head of its
//                files in registers, a butterfly takes the wave-wide least (the lowest file among
//                equals), the owner appends the line and advances.  A bounded number of steps a
//                launch; the K cursors and the output count live in device memory between launches.
//   The output lines are placed and gathered by vcfxg_gather.hip (launch_line_len, launch_text_gather).
#include "vcfxg_keyed.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kMgThreads = 256;
constexpr int kMgWaves = kMgThreads / kWave;
constexpr uint32_t kMgNone = 0xFFFFFFFFu;

// the file of line li: the last f in [0, K) with first_line[f] <= li (first_line[0] = 0)
__device__ __forceinline__ uint32_t mg_file_of(const MgLines &M, uint64_t li) {
    uint32_t lo = 0, hi = M.K - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (M.first_line[mid] <= li) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

struct MgLine {
    uint64_t w0, ks, kl, num;
    int64_t pos;
    uint32_t pn;
    uint8_t st;
};

// std::stol of the field [s, fe) (:87): C's integer grammar; no digit or a value outside long fails
__device__ __forceinline__ bool mg_stol(const char *__restrict__ buf, int64_t s, int64_t fe, int64_t &pos) {
    const CInteger v = parse_c_integer(buf, s, fe);
    if (!v.any || v.overflow64) return false;
    pos = (int64_t)v.bits();
    return true;
}

// the data line that starts at ls with its first two tabs at t0 and t1
__device__ __forceinline__ void mg_parse(const char *__restrict__ buf, int natural, int64_t ls, int64_t t0, int64_t t1, MgLine &o) {
    o.st = kMgBad;
    if (!mg_stol(buf, t0 + 1, t1, o.pos)) return;
    o.st = kMgKept;
    int64_t p = ls;
    if (natural) {  // parseChromNat :43-74
        uint32_t pw = 0;
        if (t0 - ls >= 3) {
            const uint32_t c0 = byte_at(buf, ls), c1 = byte_at(buf, ls + 1), c2 = byte_at(buf, ls + 2);
            if ((c0 | 0x20u) == 'c' && (c1 | 0x20u) == 'h' && (c2 | 0x20u) == 'r') {
                pw = (1u << 24) | (c0 << 16) | (c1 << 8) | c2;  // the three bytes as written; any prefix after none
                p += 3;
            }
        }
        uint64_t v = 0;
        const int64_t d0 = p;
        uint32_t d;
        while (p < t0 && (d = byte_at(buf, p) - '0') <= 9u) {
            v = v * 10u + d;  // (more than 18 digits: outside the domain)
            p++;
        }
        o.num = v;
        o.pn = (pw << 1) | (p > d0 ? 0u : 1u);  // numeric names before the others
    }
    o.ks = (uint64_t)p;
    o.kl = (uint64_t)(t0 - p);
    o.w0 = key_word(buf, p, (int64_t)o.kl, 0);
}

__device__ __forceinline__ void mg_clear(MgLine &o) {
    o.w0 = o.ks = o.kl = o.num = 0;
    o.pos = 0;
    o.pn = 0;
    o.st = kMgEmpty;
}

__device__ __forceinline__ void mg_store(const MgLines &M, uint64_t li, const MgLine &o) {
    M.status[li] = o.st;
    if (o.st != kMgKept) return;
    M.pos[li] = o.pos;
    M.w0[li] = o.w0;
    M.ks[li] = o.ks;
    M.kl[li] = o.kl;
    if (M.natural) {
        M.pn[li] = o.pn;
        M.num[li] = o.num;
    }
}

// first_line[f] = the first line that starts at or after file f's first byte (f = K: L); the
// per-file reductions start at L (none) and 0
__global__ __launch_bounds__(kMgThreads) void k_mg_cut(MgLines M) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t f = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; f <= M.K; f += nth) {
        const uint64_t start = M.file_start[f];
        uint64_t lo = 0, hi = M.L;  // line li starts at line_end[li - 1] + 1: non-decreasing
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((uint64_t)line_start(M.line_end, 0, mid) >= start) hi = mid;
            else lo = mid + 1;
        }
        M.first_line[f] = lo;
        if (f < M.K) {
            M.first_hash[f] = M.L;
            M.first_data[f] = M.L;
            M.bad[f] = 0;
        }
    }
}

// 0 an empty line, 1 a '#' line, 2 any other
__device__ __forceinline__ int mg_class_of(const char *__restrict__ buf, int64_t ls, int64_t le) {
    return le <= ls ? 0 : byte_at(buf, ls) == '#' ? 1 : 2;
}

// The lane pass; a line it does not settle goes to queue[counters[5]++] for k_mg_key_wave.
__global__ __launch_bounds__(kMgThreads) void k_mg_key(MgLines M, uint32_t *__restrict__ queue,
                                                       unsigned long long *__restrict__ counters) {
    const char *__restrict__ buf = M.buf;
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < M.L; li += nth) {
        const int64_t ls = line_start(M.line_end, 0, li), le = (int64_t)M.line_end[li];
        const uint32_t f = mg_file_of(M, li);
        M.file[li] = f;
        MgLine o;
        mg_clear(o);
        const int cls = mg_class_of(buf, ls, le);
        if (cls == 0) {
            M.status[li] = kMgEmpty;
            continue;
        }
        // a file's first line of a class follows the file's start or a line of another class
        const int prev = li == M.first_line[f] ? 0 : mg_class_of(buf, line_start(M.line_end, 0, li - 1), ls - 1);
        if (prev != cls) atomicMin((unsigned long long *)(cls == 1 ? M.first_hash : M.first_data) + f, (unsigned long long)li);
        if (cls == 1) {
            M.status[li] = kMgHeader;  // (k_mg_class decides: written or dropped)
            continue;
        }
        int64_t t[2] = {-1, -1};
        const int nt = window_tabs<2>(buf, ls, le, kMgWindow, t);
        if (nt < 2 && le - ls > kMgWindow) {  // the window ended before the key fields did
            queue[atomicAdd(&counters[5], 1ull)] = (uint32_t)li;
            continue;
        }
        if (nt < 2) o.st = kMgBad;
        else mg_parse(buf, M.natural, ls, t[0], t[1], o);
        mg_store(M, li, o);
    }
}

// The wave pass over the queued lines (counters[5] of them), a wave per line: the tabs by the whole
// wave, the fields by every lane alike.
__global__ __launch_bounds__(kMgThreads) void k_mg_key_wave(MgLines M, const uint32_t *__restrict__ queue,
                                                            const unsigned long long *__restrict__ counters) {
    __shared__ int64_t s_tabs[kMgWaves][10];
    const uint64_t nq = counters[5];
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t q = wid; q < nq; q += nw) {
        const uint64_t li = (uint64_t)uniform32((int)queue[q]);
        const int64_t ls = uniform64(line_start(M.line_end, 0, li)), le = uniform64((int64_t)M.line_end[li]);
        int64_t t[2] = {-1, -1};
        const int nt = head_tabs(M.buf, ls, le, 2, t, s_tabs[threadIdx.x / kWave]);
        MgLine o;
        mg_clear(o);
        if (nt < 2) o.st = kMgBad;
        else mg_parse(M.buf, M.natural, ls, uniform64(t[0]), uniform64(t[1]), o);
        if (lane() == 0) mg_store(M, li, o);
    }
}

// counters[7] = the first file with a header candidate (K: none): default mode any '#' line, -s a
// '#' line before the file's first line that is neither empty nor '#'.  One wave.
__global__ __launch_bounds__(kWave) void k_mg_hdr(MgLines M, unsigned long long *__restrict__ counters) {
    uint32_t best = M.K;
    for (uint32_t f = (uint32_t)lane(); f < M.K; f += kWave) {
        const bool has = M.sorted ? M.first_hash[f] < M.first_data[f] : M.first_hash[f] < M.L;
        if (has && f < best) best = f;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o));
    if (lane() == 0) counters[7] = best;
}

// every '#' line HEADER or DROPPED, the written flag, the status counts (counters[0..4]), BAD per
// file, the longest key string of a kept line (counters[6])
__global__ __launch_bounds__(kMgThreads) void k_mg_class(MgLines M, uint32_t *__restrict__ written,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ unsigned int red[5];
    __shared__ unsigned long long longest_s;
    if (threadIdx.x < 5) red[threadIdx.x] = 0;
    if (threadIdx.x == 5) longest_s = 0;
    __syncthreads();
    const uint32_t hdr = (uint32_t)counters[7];
    const uint64_t hdr_end = hdr < M.K ? (M.sorted ? M.first_data[hdr] : M.L) : 0;
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    uint32_t k[5] = {0, 0, 0, 0, 0};
    uint64_t longest = 0;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < M.L; li += nth) {
        uint8_t st = M.status[li];
        if (st == kMgHeader && !(M.file[li] == hdr && li < hdr_end)) {
            st = kMgDropped;
            M.status[li] = st;
        }
        written[li] = st == kMgHeader || st == kMgKept ? 1u : 0u;
        if (st == kMgKept) longest = max(longest, M.kl[li]);
        if (st == kMgBad) atomicAdd((unsigned long long *)M.bad + M.file[li], 1ull);
#pragma unroll
        for (int i = 0; i < 5; i++) k[i] += st == i ? 1u : 0u;
    }
    if (longest) atomicMax(&longest_s, (unsigned long long)longest);
    tally_status(k, red, counters);
    if (threadIdx.x == 5 && longest_s) atomicMax(&counters[6], longest_s);
}

// ---- the comparator ----------------------------------------------------------------------------

struct MgHead {
    uint64_t num, w0, kl, ks;
    int64_t pos;
    uint32_t pn, line, file;
};

__device__ __forceinline__ MgHead mg_head(const MgLines &M, uint32_t li, uint32_t f) {
    MgHead h;
    h.pos = M.pos[li];
    h.w0 = M.w0[li];
    h.kl = M.kl[li];
    h.ks = M.ks[li];
    h.pn = M.natural ? M.pn[li] : 0u;
    h.num = M.natural ? M.num[li] : 0ull;
    h.line = li;
    h.file = f;
    return h;
}

// The order of two kept lines (:17-40, :223-248): with -n the prefix bytes and the numeric class,
// then the digit run's value; the key string as unsigned bytes, a prefix before its extensions
// (the cached first word, then the input bytes); POS.
__device__ __forceinline__ int mg_cmp(const char *__restrict__ buf, const MgHead &a, const MgHead &b) {
    if (a.pn != b.pn) return a.pn < b.pn ? -1 : 1;
    if (a.num != b.num) return a.num < b.num ? -1 : 1;
    if (a.w0 != b.w0) return a.w0 < b.w0 ? -1 : 1;
    const int c = cmp_bytes(buf, (int64_t)a.ks, (int64_t)a.kl, (int64_t)b.ks, (int64_t)b.kl, 8);
    if (c) return c;
    return a.pos < b.pos ? -1 : a.pos > b.pos ? 1 : 0;
}

// counters[8] = 1 when a kept line compares greater than the next kept line of its file (line: the
// written lines in line order)
__global__ __launch_bounds__(kMgThreads) void k_mg_ordered(MgLines M, uint64_t nw, const uint32_t *__restrict__ line,
                                                           unsigned long long *__restrict__ counters) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j + 1 >= nw) return;
    const uint32_t x = line[j], y = line[j + 1];
    if (M.status[x] != kMgKept || M.status[y] != kMgKept || M.file[x] != M.file[y]) return;
    if (mg_cmp(M.buf, mg_head(M, x, 0), mg_head(M, y, 0)) > 0) counters[8] = 1ull;
}

// ---- the sort path -----------------------------------------------------------------------------

__global__ __launch_bounds__(kMgThreads) void k_mg_scatter(uint64_t L, const uint32_t *__restrict__ written,
                                                           const uint64_t *__restrict__ ord, uint32_t *__restrict__ vals) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < L; li += nth)
        if (written[li]) vals[ord[li]] = (uint32_t)li;
}

// keys[j] = one part of the key of line vals[j] (0 for a header line): kMgPartPos POS with its sign
// flipped, kMgPartLen the key string's length + 1, kMgPartWord its word w shifted right by `shift`,
// kMgPartNum the digit run's value, kMgPartPrefix (prefix word, numeric class) + 1
__global__ __launch_bounds__(kMgThreads) void k_mg_part(MgLines M, uint64_t nw, int part, uint64_t w, uint32_t shift,
                                                        const uint32_t *__restrict__ vals, uint64_t *__restrict__ keys) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= nw) return;
    const uint32_t li = vals[j];
    uint64_t key = 0;
    if (M.status[li] == kMgKept) {
        if (part == kMgPartPos) key = (uint64_t)M.pos[li] ^ (1ull << 63);
        else if (part == kMgPartLen) key = M.kl[li] + 1u;
        else if (part == kMgPartNum) key = M.num[li];
        else if (part == kMgPartPrefix) key = (uint64_t)M.pn[li] + 1u;
        else if (w == 0) key = M.w0[li] >> shift;
        else if (8u * w < M.kl[li]) key = key_word(M.buf, (int64_t)M.ks[li], (int64_t)M.kl[li], w) >> shift;
    }
    keys[j] = key;
}

// ---- the walk path -----------------------------------------------------------------------------

// The header block (the header file's written lines before its first data line) to out[0 ..), its
// size to state[0] (zeroed before); every file's cursor and end in the written lines.
__global__ __launch_bounds__(kMgThreads) void k_mg_walk_init(MgLines M, const uint64_t *__restrict__ ord,
                                                             const uint32_t *__restrict__ line, uint32_t *__restrict__ out,
                                                             const unsigned long long *__restrict__ counters,
                                                             uint64_t *__restrict__ state) {
    const uint32_t hdr = (uint32_t)counters[7];
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t f = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; f < M.K; f += nth) {
        uint64_t lo = ord[M.first_line[f]];
        const uint64_t hi = ord[M.first_line[f + 1]];
        if (f == hdr) {
            const uint64_t fd = M.first_data[f] < M.first_line[f + 1] ? M.first_data[f] : M.first_line[f + 1];
            const uint64_t lo2 = ord[fd];
            for (uint64_t j = lo; j < lo2; j++) out[j - lo] = line[j];
            state[0] = lo2 - lo;
            lo = lo2;
        }
        M.cur[f] = lo;
        M.end[f] = hi;
    }
}

__device__ __forceinline__ MgHead mg_shfl_xor(const MgHead &h, int o) {
    MgHead r;
    r.num = __shfl_xor((unsigned long long)h.num, o);
    r.w0 = __shfl_xor((unsigned long long)h.w0, o);
    r.kl = __shfl_xor((unsigned long long)h.kl, o);
    r.ks = __shfl_xor((unsigned long long)h.ks, o);
    r.pos = (int64_t)__shfl_xor((unsigned long long)h.pos, o);
    r.pn = (uint32_t)__shfl_xor((int)h.pn, o);
    r.line = (uint32_t)__shfl_xor((int)h.line, o);
    r.file = (uint32_t)__shfl_xor((int)h.file, o);
    return r;
}

// the least head among the lane's files f = lane, lane + 64, ... (file kMgNone: none left); the
// earliest file among equals
__device__ __forceinline__ MgHead mg_refill(const MgLines &M, const uint32_t *__restrict__ line) {
    MgHead best;
    best.num = best.w0 = best.kl = best.ks = 0;
    best.pos = 0;
    best.pn = best.line = 0;
    best.file = kMgNone;
    for (uint32_t f = (uint32_t)lane(); f < M.K; f += kWave) {
        const uint64_t j = M.cur[f];
        if (j >= M.end[f]) continue;
        const MgHead h = mg_head(M, line[j], f);
        if (best.file == kMgNone || mg_cmp(M.buf, h, best) < 0) best = h;
    }
    return best;
}

// The heap process (:325-344) from the cursors and state[0] (the lines written so far), at most
// `steps` steps: one wave.
__global__ __launch_bounds__(kWave) void k_mg_walk(MgLines M, const uint32_t *__restrict__ line, uint32_t *__restrict__ out,
                                                   uint64_t steps, uint64_t *__restrict__ state) {
    if (blockIdx.x) return;
    uint64_t n = state[0];
    MgHead best = mg_refill(M, line);
    for (uint64_t s = 0; s < steps; s++) {
        MgHead w = best;
#pragma unroll 1
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const MgHead x = mg_shfl_xor(w, o);
            if (x.file == kMgNone) continue;
            bool take = w.file == kMgNone;
            if (!take) {
                const int c = mg_cmp(M.buf, x, w);
                take = c < 0 || (c == 0 && x.file < w.file);
            }
            if (take) w = x;
        }
        const uint32_t wf = (uint32_t)uniform32((int)w.file);  // (every lane holds the same least)
        if (wf == kMgNone) break;
        if ((wf & (kWave - 1u)) == (uint32_t)lane()) {
            out[n] = w.line;
            M.cur[wf] = M.cur[wf] + 1u;
            best = mg_refill(M, line);
        }
        n++;
    }
    if (lane() == 0) state[0] = n;
}

// ---- launchers ---------------------------------------------------------------------------------

hipError_t launch_mg_cut(const MgLines &M, hipStream_t s) {
    hipLaunchKernelGGL(k_mg_cut, dim3(grid_for((uint64_t)M.K + 1, kMgThreads, 1024)), dim3(kMgThreads), 0, s, M);
    return hipGetLastError();
}

hipError_t launch_mg_key(const MgLines &M, uint32_t *queue, unsigned long long *counters, hipStream_t s) {
    if (!M.L) return hipSuccess;
    hipLaunchKernelGGL(k_mg_key, dim3(grid_for(M.L, kMgThreads, 8192)), dim3(kMgThreads), 0, s, M, queue, counters);
    hipLaunchKernelGGL(k_mg_key_wave, dim3(grid_for(M.L, kMgWaves, 2048)), dim3(kMgThreads), 0, s, M, queue, counters);
    return hipGetLastError();
}

hipError_t launch_mg_class(const MgLines &M, uint32_t *written, unsigned long long *counters, hipStream_t s) {
    if (!M.L) return hipSuccess;
    hipLaunchKernelGGL(k_mg_hdr, dim3(1), dim3(kWave), 0, s, M, counters);
    hipLaunchKernelGGL(k_mg_class, dim3(grid_for(M.L, kMgThreads * 4, 1024)), dim3(kMgThreads), 0, s, M, written, counters);
    return hipGetLastError();
}

hipError_t launch_mg_scatter(uint64_t L, const uint32_t *written, const uint64_t *ord, uint32_t *vals, hipStream_t s) {
    if (!L) return hipSuccess;
    hipLaunchKernelGGL(k_mg_scatter, dim3(grid_for(L, kMgThreads, 8192)), dim3(kMgThreads), 0, s, L, written, ord, vals);
    return hipGetLastError();
}

hipError_t launch_mg_part(const MgLines &M, uint64_t nw, int part, uint64_t w, uint32_t shift, const uint32_t *vals,
                          uint64_t *keys, hipStream_t s) {
    if (!nw) return hipSuccess;
    hipLaunchKernelGGL(k_mg_part, flat_grid(nw, kMgThreads), dim3(kMgThreads), 0, s, M, nw, part, w, shift, vals, keys);
    return hipGetLastError();
}

hipError_t launch_mg_ordered(const MgLines &M, uint64_t nw, const uint32_t *line, unsigned long long *counters,
                             hipStream_t s) {
    if (nw < 2) return hipSuccess;
    hipLaunchKernelGGL(k_mg_ordered, flat_grid(nw, kMgThreads), dim3(kMgThreads), 0, s, M, nw, line, counters);
    return hipGetLastError();
}

hipError_t launch_mg_walk_init(const MgLines &M, const uint64_t *ord, const uint32_t *line, uint32_t *out,
                               const unsigned long long *counters, uint64_t *state, hipStream_t s) {
    hipLaunchKernelGGL(k_mg_walk_init, dim3(grid_for(M.K, kMgThreads, 1024)), dim3(kMgThreads), 0, s, M, ord, line, out,
                       counters, state);
    return hipGetLastError();
}

hipError_t launch_mg_walk(const MgLines &M, const uint32_t *line, uint32_t *out, uint64_t steps, uint64_t *state,
                          hipStream_t s) {
    hipLaunchKernelGGL(k_mg_walk, dim3(1), dim3(kWave), 0, s, M, line, out, steps, state);
    return hipGetLastError();
}

}  // namespace vcfxg
