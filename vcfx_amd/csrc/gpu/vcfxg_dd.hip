// vcfxg_dd.hip -- VCFX_duplicate_remover's keep / drop decision (VCFX_duplicate_remover.cpp:182-214
// stdin mode, :226-382 file mode): a line is kept when no earlier line carries the same
// (CHROM bytes, POS integer, REF bytes, multiset of ALT tokens).
//
// Three passes over the indexed lines (the sort between the first two is hipcub's, vcfxg_api_dd.hip):
//   k_dd_key     a lane per line over the line's first kDdWindow bytes: status, the first five tab
//                offsets (the fifth = ALT's end: the tab or the line's end), POS and the key's
//                64-bit hash, one sequential byte loop on 16 B loads.  The sample columns are never
//                read.  A line whose ALT does not end inside the window, or whose POS is not 1..9
//                digits from its first byte, is queued for k_dd_key_wave, a wave per line (head_tabs,
//                POS by the general strtol restatement, dd_pos over parse_c_integer, CHROM / REF
//                hashed lane-strided, ALT a lane per token), so any line width passes.
//   (sort)       (hash & mask, line) of the data lines, compacted in line order, stable radix sort:
//                inside a run of equal hashes the lines ascend
//   k_dd_heads / k_dd_verify   run heads, (max scan: every element's run head), then a lane per
//                element: a head is kept, another element is compared exactly with its head: equal
//                = duplicate, else it is a true hash collision, left pending
//   k_dd_resolve a wave per run with pending elements walks them in line order, each against the
//                elements of the run kept so far (64 candidates a step): correctness does not
//                depend on the hash.  A run of n equal lines costs n comparisons.
//
// The hash (mix64, hash_byte, hash_field: vcfxg_keyed.h).  byte(b, i) = mix((i << 8 | b) + c0) with i the byte's place in its field or token;
// field(bytes) = mix(sum of byte() ^ (len * c1 + c2)); ALT = the plain sum of field(token) over its
// tokens (commutative: no token order, no sorting) + mix(token count);
// key = mix(mix(mix(mix(field(CHROM) + 1) ^ POS * c3) + field(REF)) ^ ALT).  mix = splitmix64's
// finaliser.  Both schedules compute the same function: equal keys meet in one run whichever path
// took their lines.
//
// Exact comparison (dd_equal): POS integers, CHROM and REF bytes; ALT byte-identical = equal, a
// different token count or total token length = unequal, else each token of one side must occur
// as often in the other (quadratic in the token count, a lane per comparison: ALT fields that
// differ only in order are rare and short).
// Mode: stdin splits ALT at every comma (empty tokens count), file drops empty tokens; POS see dd_pos.
#include "vcfxg_keyed.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kDdThreads = 256;
constexpr int kDdWaves = kDdThreads / kWave;
constexpr uint8_t kDdData = 5;  // a data line not decided yet (never left behind by a call)

struct DdArgs {
    const char *buf;
    int64_t data_start, n;  // the indexed range's first byte; the input's bytes
    const uint64_t *line_end;
    uint64_t L;
    int stdin_mode;
};

__device__ __forceinline__ uint64_t dd_key(uint64_t fc, int32_t pos, uint64_t fr, uint64_t alt, uint64_t ntok) {
    uint64_t h = mix64(fc + 1u);
    h = mix64(h ^ ((uint64_t)(uint32_t)pos * 0xE7037ED1A0B428DBull));
    h = mix64(h + fr);
    return mix64(h ^ (alt + mix64(ntok)));
}

// POS of the field [s, fe).  stdin mode: std::stoi of the field, any exception 0 (:115-119): C
// white space skipped, one sign, digits; no digits or a value outside int = 0.  File mode: strtol
// from the field's first byte, cast to int (:146): the white-space skip crosses tabs and newlines
// (bounded here by the input's end), the value saturates at LONG_MAX / LONG_MIN and loses its
// high 32 bits.
__device__ __forceinline__ int32_t dd_pos(const char *__restrict__ buf, int64_t s, int64_t fe, int64_t n, int stdin_mode) {
    const CInteger v = parse_c_integer(buf, s, stdin_mode ? fe : n);
    if (!v.any) return 0;
    if (stdin_mode) return v.fits_int() ? (int32_t)(uint32_t)v.bits() : 0;
    if (v.overflow64) return v.neg ? 0 : -1;
    return (int32_t)(uint32_t)v.bits();
}

// ---- the key pass ------------------------------------------------------------------------------

struct DdLine {
    uint64_t t0, t1, t2, t3, t4, hash;
    int32_t pos;
    uint8_t st;
};

// The lane's line [ls, le) over its first kDdWindow bytes; false: the wave takes it.
__device__ __forceinline__ bool dd_lane_line(const DdArgs &A, int64_t ls, int64_t le, DdLine &o) {
    const char *__restrict__ buf = A.buf;
    const int64_t we = le - ls > kDdWindow ? ls + kDdWindow : le;
    uint32_t nt = 0, pv = 0, nd = 0;
    bool pos_open = true, pos_ok = false, done = false;
    uint64_t sum = 0, idx = 0, fc = 0, fr = 0, asum = 0, ntok = 0;
    for (int64_t a = ls & ~(int64_t)15; a < we && !done; a += 16) {
        const uint4 v = load16(buf, a);
        const uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
        const int j0 = a < ls ? (int)(ls - a) : 0, j1 = we - a < 16 ? (int)(we - a) : 16;
        for (int j = j0; j < j1; j++) {
            const uint32_t b = (uint32_t)((j < 8 ? lo : hi) >> (8 * (j & 7))) & 0xFFu;
            const int64_t p = a + j;
            if (b == '\t') {
                if (nt == 0) {
                    fc = hash_field(sum, idx);
                    o.t0 = (uint64_t)p;
                } else if (nt == 1) {
                    o.t1 = (uint64_t)p;
                } else if (nt == 2) {
                    o.t2 = (uint64_t)p;
                } else if (nt == 3) {
                    fr = hash_field(sum, idx);
                    o.t3 = (uint64_t)p;
                } else {
                    if (A.stdin_mode || idx) {
                        asum += hash_field(sum, idx);
                        ntok++;
                    }
                    o.t4 = (uint64_t)p;
                    done = true;
                    break;
                }
                nt++;
                sum = 0;
                idx = 0;
            } else if (nt == 1) {
                const uint32_t d = b - '0';
                if (pos_open && d <= 9u && nd < 9u) {
                    pv = pv * 10u + d;
                    nd++;
                    pos_ok = true;
                } else {
                    if (pos_open && (d <= 9u || !nd)) pos_ok = false;  // a tenth digit; no digit first
                    pos_open = false;
                }
            } else if (nt == 4 && b == ',') {
                if (A.stdin_mode || idx) {
                    asum += hash_field(sum, idx);
                    ntok++;
                }
                sum = 0;
                idx = 0;
            } else if (nt != 2) {
                sum += hash_byte(b, idx);
                idx++;
            }
        }
    }
    if (!done) {
        if (we < le) return false;  // the window ended inside the key fields
        if (nt < 4) {
            o.st = kDdShort;
            return true;
        }
        if (A.stdin_mode || idx) {  // ALT runs to the line's end
            asum += hash_field(sum, idx);
            ntok++;
        }
        o.t4 = (uint64_t)le;
    }
    if (!pos_ok) return false;
    o.pos = (int32_t)pv;
    o.hash = dd_key(fc, o.pos, fr, asum, ntok);
    o.st = kDdData;
    return true;
}

__device__ __forceinline__ uint64_t dd_wave_sum64(uint64_t x) {
    return (uint64_t)wave_sum<unsigned long long>((unsigned long long)x);
}

// field(bytes of [s, e)) by the whole wave
__device__ __forceinline__ uint64_t dd_wave_field(const char *__restrict__ buf, int64_t s, int64_t e) {
    uint64_t sum = 0;
    for (int64_t p = s + lane(); p < e; p += kWave) sum += hash_byte(byte_at(buf, p), (uint64_t)(p - s));
    return hash_field(dd_wave_sum64(sum), (uint64_t)(e - s));
}

// The wave's line [ls, le) (uniform; every lane active): any width.
__device__ __forceinline__ void dd_wave_line(const DdArgs &A, int64_t ls, int64_t le, int64_t *lds, DdLine &o) {
    const char *__restrict__ buf = A.buf;
    int64_t t[5];
    const int nt = head_tabs(buf, ls, le, 5, t, lds);
    if (nt < 4) {
        o.st = kDdShort;
        return;
    }
    const int64_t t4 = nt == 5 ? t[4] : le;
    o.t0 = (uint64_t)t[0], o.t1 = (uint64_t)t[1], o.t2 = (uint64_t)t[2], o.t3 = (uint64_t)t[3], o.t4 = (uint64_t)t4;
    o.pos = dd_pos(buf, t[0] + 1, t[1], A.n, A.stdin_mode);
    const uint64_t fc = dd_wave_field(buf, ls, t[0]), fr = dd_wave_field(buf, t[2] + 1, t[3]);
    // ALT [s, e): a token starts at s and after every comma (so possibly at e: an empty last token)
    const int64_t s = t[3] + 1, e = t4;
    uint64_t asum = 0;
    uint32_t ntok = 0;
    for (int64_t w = s; w <= e; w += kWave) {
        const int64_t p = w + lane();
        if (p <= e && (p == s || byte_at(buf, p - 1) == ',')) {
            uint64_t sum = 0;
            int64_t q = p;
            uint32_t b;
            while (q < e && (b = byte_at(buf, q)) != ',') {
                sum += hash_byte(b, (uint64_t)(q - p));
                q++;
            }
            if (A.stdin_mode || q > p) {
                asum += hash_field(sum, (uint64_t)(q - p));
                ntok++;
            }
        }
    }
    o.hash = dd_key(fc, o.pos, fr, dd_wave_sum64(asum), (uint64_t)wave_sum32(ntok));
    o.st = kDdData;
}

__device__ __forceinline__ void dd_store(uint64_t li, const DdLine &o, uint8_t *status, uint32_t *isdata, uint64_t *tabs,
                                         int32_t *pos, uint64_t *hash) {
    status[li] = o.st;
    isdata[li] = o.st == kDdData ? 1u : 0u;
    if (o.st == kDdData) {
        uint64_t *t = tabs + 5 * li;
        t[0] = o.t0, t[1] = o.t1, t[2] = o.t2, t[3] = o.t3, t[4] = o.t4;
        pos[li] = o.pos;
        hash[li] = o.hash;
    }
}

// The lane pass; a line it does not settle goes to queue[counters[5]++] for k_dd_key_wave.
__global__ __launch_bounds__(kDdThreads) void k_dd_key(DdArgs A, uint8_t *__restrict__ status, uint32_t *__restrict__ isdata,
                                                       uint64_t *__restrict__ tabs, int32_t *__restrict__ pos,
                                                       uint64_t *__restrict__ hash, uint32_t *__restrict__ queue,
                                                       unsigned long long *__restrict__ counters) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < A.L; li += nth) {
        const int64_t ls = line_start(A.line_end, A.data_start, li), le = (int64_t)A.line_end[li];
        DdLine o;
        o.t0 = o.t1 = o.t2 = o.t3 = o.t4 = o.hash = 0;
        o.pos = 0;
        o.st = kDdEmpty;
        bool have = true;
        if (le > ls) {
            if (byte_at(A.buf, ls) == '#') o.st = kDdHeader;
            else have = dd_lane_line(A, ls, le, o);
        }
        if (have) dd_store(li, o, status, isdata, tabs, pos, hash);
        else queue[atomicAdd(&counters[5], 1ull)] = (uint32_t)li;
    }
}

// The wave pass over the queued lines (counters[5] of them), a wave per line.
__global__ __launch_bounds__(kDdThreads) void k_dd_key_wave(DdArgs A, uint8_t *__restrict__ status, uint32_t *__restrict__ isdata,
                                                            uint64_t *__restrict__ tabs, int32_t *__restrict__ pos,
                                                            uint64_t *__restrict__ hash, const uint32_t *__restrict__ queue,
                                                            const unsigned long long *__restrict__ counters) {
    __shared__ int64_t s_tabs[kDdWaves][10];
    const uint64_t nq = counters[5];
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t q = wid; q < nq; q += nw) {
        const uint64_t li = (uint64_t)uniform32((int)queue[q]);
        const int64_t ls = uniform64(line_start(A.line_end, A.data_start, li)), le = uniform64((int64_t)A.line_end[li]);
        DdLine o;
        o.t0 = o.t1 = o.t2 = o.t3 = o.t4 = o.hash = 0;
        o.pos = 0;
        dd_wave_line(A, ls, le, s_tabs[threadIdx.x / kWave], o);
        if (lane() == 0) dd_store(li, o, status, isdata, tabs, pos, hash);
    }
}

// (hash & mask, line) of the data lines at their ordinals (ord = the exclusive scan of isdata)
__global__ __launch_bounds__(kDdThreads) void k_dd_gather(uint64_t L, const uint32_t *__restrict__ isdata,
                                                          const uint64_t *__restrict__ ord, const uint64_t *__restrict__ hash,
                                                          uint64_t mask, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < L; li += nth)
        if (isdata[li]) {
            keys[ord[li]] = hash[li] & mask;
            vals[ord[li]] = (uint32_t)li;
        }
}

// ---- the verify pass ---------------------------------------------------------------------------

struct DdCmp {
    const char *buf;
    const uint64_t *line_end, *tabs;
    const int32_t *pos;
    int64_t data_start;
    int stdin_mode;
};

__device__ __forceinline__ bool dd_bytes_equal(const char *__restrict__ buf, int64_t a, int64_t b, int64_t n) {
    for (int64_t i = 0; i < n; i++)
        if (byte_at(buf, a + i) != byte_at(buf, b + i)) return false;
    return true;
}
// tokens (empty ones only in stdin mode) and their bytes of the ALT field [s, e)
__device__ __forceinline__ void dd_alt_shape(const char *__restrict__ buf, int64_t s, int64_t e, int stdin_mode,
                                             uint64_t &count, uint64_t &bytes) {
    uint64_t commas = 0, empty = 0;
    int64_t ts = s;
    for (int64_t p = s; p <= e; p++)
        if (p == e || byte_at(buf, p) == ',') {
            if (p < e) commas++;
            if (p == ts) empty++;
            ts = p + 1;
        }
    bytes = (uint64_t)(e - s) - commas;
    count = commas + 1u - (stdin_mode ? 0u : empty);
}
// how often the token [ts, te) occurs among the tokens of [s, e)
__device__ __forceinline__ uint64_t dd_occurs(const char *__restrict__ buf, int64_t ts, int64_t te, int64_t s, int64_t e) {
    uint64_t k = 0;
    int64_t a = s;
    for (int64_t p = s; p <= e; p++)
        if (p == e || byte_at(buf, p) == ',') {
            if (p - a == te - ts && dd_bytes_equal(buf, a, ts, te - ts)) k++;
            a = p + 1;
        }
    return k;
}
// the keys of lines x and y are equal
__device__ __forceinline__ bool dd_equal(const DdCmp &C, uint32_t x, uint32_t y) {
    if (C.pos[x] != C.pos[y]) return false;
    const char *__restrict__ buf = C.buf;
    const uint64_t *tx = C.tabs + 5 * (uint64_t)x, *ty = C.tabs + 5 * (uint64_t)y;
    const int64_t xs = line_start(C.line_end, C.data_start, x), ys = line_start(C.line_end, C.data_start, y);
    const int64_t cl = (int64_t)tx[0] - xs;
    if (cl != (int64_t)ty[0] - ys || !dd_bytes_equal(buf, xs, ys, cl)) return false;
    const int64_t xr = (int64_t)tx[2] + 1, yr = (int64_t)ty[2] + 1, rl = (int64_t)tx[3] - xr;
    if (rl != (int64_t)ty[3] - yr || !dd_bytes_equal(buf, xr, yr, rl)) return false;
    const int64_t xa = (int64_t)tx[3] + 1, xe = (int64_t)tx[4], ya = (int64_t)ty[3] + 1, ye = (int64_t)ty[4];
    if (xe - xa == ye - ya && dd_bytes_equal(buf, xa, ya, xe - xa)) return true;
    uint64_t cx, bx, cy, by;
    dd_alt_shape(buf, xa, xe, C.stdin_mode, cx, bx);
    dd_alt_shape(buf, ya, ye, C.stdin_mode, cy, by);
    if (cx != cy || bx != by) return false;
    // the same number of tokens: equal multisets when every token of x is as frequent in y
    int64_t a = xa;
    for (int64_t p = xa; p <= xe; p++)
        if (p == xe || byte_at(buf, p) == ',') {
            if ((C.stdin_mode || p > a) && dd_occurs(buf, a, p, xa, xe) != dd_occurs(buf, a, p, ya, ye)) return false;
            a = p + 1;
        }
    return true;
}

// hp[j] = j where a run of equal keys begins, else 0 (its inclusive max scan = each element's head)
__global__ __launch_bounds__(kDdThreads) void k_dd_heads(uint64_t nd, const uint64_t *__restrict__ keys, uint32_t *__restrict__ hp) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j < nd) hp[j] = j && keys[j] != keys[j - 1] ? (uint32_t)j : 0u;
}

// a head is kept; another element equal to its head is a duplicate, else pending (left[head] = 1,
// counters[6] counts them)
__global__ __launch_bounds__(kDdThreads) void k_dd_verify(DdCmp C, uint64_t nd, const uint32_t *__restrict__ vals,
                                                          const uint32_t *__restrict__ head, uint8_t *__restrict__ status,
                                                          uint8_t *__restrict__ left, unsigned long long *__restrict__ counters) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= nd) return;
    const uint32_t h = head[j];
    if (h == j) {
        status[vals[j]] = kDdKept;
    } else if (dd_equal(C, vals[j], vals[h])) {
        status[vals[j]] = kDdDup;
    } else {
        left[h] = 1;
        atomicAdd(&counters[6], 1ull);
    }
}

__device__ __forceinline__ uint8_t dd_status_load(const uint8_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A wave per run that has pending elements: in line order each one against the run's elements
// kept so far (the head excepted: it differs), 64 candidates a step.
__global__ __launch_bounds__(kDdThreads) void k_dd_resolve(DdCmp C, uint64_t nd, const uint64_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ vals, const uint8_t *__restrict__ left,
                                                           uint8_t *status, const unsigned long long *__restrict__ counters) {
    if (counters[6] == 0) return;
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t h = wid; h < nd; h += nw) {
        if (!left[h]) continue;
        const uint64_t key = keys[h];
        for (uint64_t e = h + 1; e < nd && keys[e] == key; e++) {
            // (loaded per lane: as a scalar value, the offsets dd_equal derives from it overflow the
            // scalar registers)
            const uint32_t le = vals[e + (uint64_t)(lane() >> 6)];
            if (dd_status_load(status + uniform32((int)le)) != kDdData) continue;
            bool found = false;
            for (uint64_t base = h + 1; base < e && !found; base += kWave) {
                const uint64_t c = base + (uint64_t)lane();
                bool hit = false;
                if (c < e) {
                    const uint32_t lc = vals[c];
                    hit = dd_status_load(status + lc) == kDdKept && dd_equal(C, le, lc);
                }
                found = __ballot(hit) != 0ull;
            }
            if (lane() == 0) __hip_atomic_store(status + le, found ? kDdDup : kDdKept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
}

// counters[st] += the lines of each final status (0..4)
__global__ __launch_bounds__(kDdThreads) void k_dd_count(uint64_t L, const uint8_t *__restrict__ status,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ unsigned int red[5];
    if (threadIdx.x < 5) red[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    uint32_t k[5] = {0, 0, 0, 0, 0};
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < L; li += nth) {
        const uint8_t st = status[li];
#pragma unroll
        for (int i = 0; i < 5; i++) k[i] += st == i ? 1u : 0u;
    }
    tally_status(k, red, counters);
}

// ---- launchers ---------------------------------------------------------------------------------

hipError_t launch_dd_key(const char *buf, int64_t data_start, int64_t n, const uint64_t *line_end, uint64_t L,
                         int stdin_mode, uint8_t *status, uint32_t *isdata, uint64_t *tabs, int32_t *pos, uint64_t *hash,
                         uint32_t *queue, unsigned long long *counters, hipStream_t s) {
    if (!L) return hipSuccess;
    const DdArgs A{buf, data_start, n, line_end, L, stdin_mode ? 1 : 0};
    hipLaunchKernelGGL(k_dd_key, dim3(grid_for(L, kDdThreads, 8192)), dim3(kDdThreads), 0, s, A, status, isdata, tabs, pos,
                       hash, queue, counters);
    hipLaunchKernelGGL(k_dd_key_wave, dim3(grid_for(L, kDdWaves, 2048)), dim3(kDdThreads), 0, s, A, status, isdata, tabs, pos,
                       hash, queue, counters);
    return hipGetLastError();
}

hipError_t launch_dd_gather(uint64_t L, const uint32_t *isdata, const uint64_t *ord, const uint64_t *hash,
                            uint32_t hash_bits, uint64_t *keys, uint32_t *vals, hipStream_t s) {
    if (!L) return hipSuccess;
    const uint64_t mask = hash_bits && hash_bits < 64u ? (1ull << hash_bits) - 1u : ~0ull;
    hipLaunchKernelGGL(k_dd_gather, dim3(grid_for(L, kDdThreads, 8192)), dim3(kDdThreads), 0, s, L, isdata, ord, hash, mask,
                       keys, vals);
    return hipGetLastError();
}

hipError_t launch_dd_heads(uint64_t nd, const uint64_t *keys, uint32_t *hp, hipStream_t s) {
    if (!nd) return hipSuccess;
    hipLaunchKernelGGL(k_dd_heads, flat_grid(nd, kDdThreads), dim3(kDdThreads), 0, s, nd, keys, hp);
    return hipGetLastError();
}

hipError_t launch_dd_verify(const char *buf, int64_t data_start, const uint64_t *line_end, int stdin_mode,
                            const uint64_t *tabs, const int32_t *pos, uint64_t nd, const uint64_t *keys, const uint32_t *vals,
                            const uint32_t *head, uint8_t *status, uint8_t *left, unsigned long long *counters,
                            hipStream_t s) {
    if (!nd) return hipSuccess;
    const DdCmp C{buf, line_end, tabs, pos, data_start, stdin_mode ? 1 : 0};
    hipLaunchKernelGGL(k_dd_verify, flat_grid(nd, kDdThreads), dim3(kDdThreads), 0, s, C, nd, vals,
                       head, status, left, counters);
    hipLaunchKernelGGL(k_dd_resolve, dim3(grid_for(nd, kDdWaves, 2048)), dim3(kDdThreads), 0, s, C, nd, keys, vals, left,
                       status, counters);
    return hipGetLastError();
}

hipError_t launch_dd_count(uint64_t L, const uint8_t *status, unsigned long long *counters, hipStream_t s) {
    if (!L) return hipSuccess;
    hipLaunchKernelGGL(k_dd_count, dim3(grid_for(L, kDdThreads * 16, 1024)), dim3(kDdThreads), 0, s, L, status, counters);
    return hipGetLastError();
}

}  // namespace vcfxg
