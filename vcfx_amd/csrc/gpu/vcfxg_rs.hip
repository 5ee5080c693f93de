// vcfxg_rs.hip -- VCFX_region_subsampler (VCFX_region_subsampler.cpp: loadRegions :344-381,
// sortAndMergeIntervals :383-404, processVCFMmap :427-517 file mode, processVCF :519-564 stdin mode):
// a data line is kept when its CHROM bytes name a chromosome of the BED and its POS lies in the union
// of that chromosome's intervals.  The first join of the records against a side table.
//
// The table (built once per vcfxg_regions_load; the sort between k_rs_keys and k_rs_sorted is the
// keyed tools' radix sort, vcfxg_api_rs.hip):
//   k_rs_keys      (name id << 32 | start, interval) pairs
//   k_rs_sorted    the sorted intervals' id and start, and the scan key (id << 32 | end)
//   k_rs_tile_max / k_rs_carry / k_rs_reach   the inclusive running maximum of the scan keys: each
//                  block's tile maximum, one block that turns the tile maxima into every tile's
//                  carry-in (the maximum of all earlier tiles), and the tiles scanned again on top
//                  of their carry.  The ids ascend along the table, so a key of an earlier name is
//                  below every key of the current one: the plain maximum is already segmented, and
//                  reach[j] = its low word = the furthest end among the intervals of j's name that
//                  start at or before start[j].
//   k_rs_bounds    per name its [first, last) in the table; open[j] = a merged interval begins at j
//                  (the name's first, or start > reach before + 1 in 64 bits)
//   k_rs_rows      the merged intervals (the reference's table) at the scan of open: a row's end is
//                  the reach of its last element
//   k_rs_dict      the names into an open-addressing table (slot = id + 1) over hash_field of their
//                  bytes, masked to hash_bits; linear probing, at most half full
// The per-line pass (vcfxg_region_filter):
//   k_rs_class     a lane per line over its first kRsWindow bytes, one byte loop on 16 B loads: the
//                  first two tabs, CHROM's hash, POS in the mode's grammar (file: every digit byte of
//                  the field accumulated modulo 2^32, parseIntFast :190-198; stdin: std::stoi), then in
//                  stdin mode the tabs up to the seventh counted from the byte masks; the look-up
//                  (rs_lookup: the dictionary probe, every hit confirmed byte by byte, then a binary
//                  search of the name's range for the last start <= POS: inside when the reach
//                  there is >= POS).  The sample columns are never read.  A line whose two (stdin:
//                  seven) tabs do not lie inside the window while the line goes on past it is queued
//                  for k_rs_class_wave, a wave per line (head_tabs, CHROM hashed lane-strided).
//                  A line that starts with "#CHROM" lowers first_chrom to its index (atomic minimum).
//   k_rs_finish    a data line before first_chrom becomes kRsEarly (that check precedes the others
//                  in the reference); the lines of each status are tallied (tally_status).
#include "vcfxg_keyed.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kRsThreads = 256;
constexpr int kRsWaves = kRsThreads / kWave;
constexpr int kRsItems = 4;                        // scan: elements per thread
constexpr int kRsTile = kRsThreads * kRsItems;     // ... and per block

// ---- the table ---------------------------------------------------------------------------------

__global__ __launch_bounds__(kRsThreads) void k_rs_keys(uint64_t n, const uint32_t *__restrict__ id,
                                                        const int32_t *__restrict__ start, uint64_t *__restrict__ keys,
                                                        uint32_t *__restrict__ vals) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    keys[j] = ((uint64_t)id[j] << 32) | (uint32_t)start[j];
    vals[j] = (uint32_t)j;
}

__global__ __launch_bounds__(kRsThreads) void k_rs_sorted(uint64_t n, const uint64_t *__restrict__ keys,
                                                          const uint32_t *__restrict__ vals, const int32_t *__restrict__ end,
                                                          uint32_t *__restrict__ sid, int32_t *__restrict__ sstart,
                                                          uint64_t *__restrict__ scan_key) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t k = keys[j];
    sid[j] = (uint32_t)(k >> 32);
    sstart[j] = (int32_t)(uint32_t)k;
    scan_key[j] = (k & 0xFFFFFFFF00000000ull) | (uint32_t)end[vals[j]];
}

__device__ __forceinline__ uint64_t rs_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t rs_shfl_up(uint64_t v, int o) {
    return (uint64_t)__shfl_up((unsigned long long)v, o);
}
// the inclusive running maximum over the block's threads (every thread calls it); *total = the block's
__device__ __forceinline__ uint64_t rs_block_incl_max(uint64_t v, uint64_t *s_wave, uint64_t *total) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint64_t t = rs_shfl_up(v, o);
        if (lane() >= o) v = rs_max(v, t);
    }
    const int w = threadIdx.x / kWave;
    if (lane() == kWave - 1) s_wave[w] = v;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kRsWaves; i++) {
        const uint64_t t = s_wave[i];
        if (i < w) before = rs_max(before, t);
        all = rs_max(all, t);
    }
    __syncthreads();  // (s_wave is free for the caller's next round)
    *total = all;
    return rs_max(v, before);
}

// tile_max[b] = the maximum of tile b
__global__ __launch_bounds__(kRsThreads) void k_rs_tile_max(uint64_t n, const uint64_t *__restrict__ key,
                                                            uint64_t *__restrict__ tile_max) {
    __shared__ uint64_t s_wave[kRsWaves];
    const uint64_t base = blockIdx.x * (uint64_t)kRsTile + threadIdx.x * (uint64_t)kRsItems;
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < kRsItems; i++)
        if (base + i < n) m = rs_max(m, key[base + i]);
    uint64_t total;
    rs_block_incl_max(m, s_wave, &total);
    if (threadIdx.x == 0) tile_max[blockIdx.x] = total;
}

// tile_max[b] -> the maximum of the tiles before b (0 for the first): one block walks the nb values
// kRsThreads at a time, the running maximum carried from round to round
__global__ __launch_bounds__(kRsThreads) void k_rs_carry(uint64_t nb, uint64_t *__restrict__ tile_max) {
    __shared__ uint64_t s_wave[kRsWaves], s_last[kRsWaves];
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += kRsThreads) {
        const uint64_t b = b0 + threadIdx.x;
        const uint64_t v = b < nb ? tile_max[b] : 0;
        uint64_t total;
        const uint64_t incl = rs_max(rs_block_incl_max(v, s_wave, &total), carry);
        // exclusive: the thread before this one, or the carry
        uint64_t prev = rs_shfl_up(incl, 1);
        if (lane() == kWave - 1) s_last[threadIdx.x / kWave] = incl;
        __syncthreads();
        if (lane() == 0) prev = threadIdx.x ? s_last[threadIdx.x / kWave - 1] : carry;
        if (b < nb) tile_max[b] = prev;
        carry = rs_max(carry, total);
        __syncthreads();
    }
}

// reach[j] = the low word of the inclusive running maximum at j
__global__ __launch_bounds__(kRsThreads) void k_rs_reach(uint64_t n, const uint64_t *__restrict__ key,
                                                         const uint64_t *__restrict__ carry, int32_t *__restrict__ reach) {
    __shared__ uint64_t s_wave[kRsWaves], s_last[kRsWaves];
    const uint64_t base = blockIdx.x * (uint64_t)kRsTile + threadIdx.x * (uint64_t)kRsItems;
    uint64_t v[kRsItems], m = 0;
#pragma unroll
    for (int i = 0; i < kRsItems; i++) {
        v[i] = base + i < n ? key[base + i] : 0;
        m = rs_max(m, v[i]);
        v[i] = m;  // the running maximum inside the thread
    }
    uint64_t total;
    const uint64_t incl = rs_block_incl_max(m, s_wave, &total);
    // everything before this thread: the threads before it in the block and the tile's carry-in
    uint64_t before = rs_shfl_up(incl, 1);
    if (lane() == kWave - 1) s_last[threadIdx.x / kWave] = incl;
    __syncthreads();
    if (lane() == 0) before = threadIdx.x ? s_last[threadIdx.x / kWave - 1] : 0;
    before = rs_max(before, carry[blockIdx.x]);
#pragma unroll
    for (int i = 0; i < kRsItems; i++)
        if (base + i < n) reach[base + i] = (int32_t)(uint32_t)rs_max(v[i], before);
}

// per name its [first, last) (zeroed beforehand: a name without intervals keeps [0, 0)); open[j] = 1
// where a merged interval begins (open[n] zeroed beforehand)
__global__ __launch_bounds__(kRsThreads) void k_rs_bounds(uint64_t n, const uint32_t *__restrict__ sid,
                                                          const int32_t *__restrict__ sstart, const int32_t *__restrict__ reach,
                                                          uint32_t *__restrict__ first, uint32_t *__restrict__ last,
                                                          uint32_t *__restrict__ open) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t id = sid[j];
    const bool head = j == 0 || sid[j - 1] != id;
    if (head) first[id] = (uint32_t)j;
    if (j + 1 == n || sid[j + 1] != id) last[id] = (uint32_t)(j + 1);
    open[j] = head || (int64_t)sstart[j] > (int64_t)reach[j - 1] + 1 ? 1u : 0u;
}

// the merged intervals: row ord[j] opens at j; the row of j ends at j when the next element opens one
__global__ __launch_bounds__(kRsThreads) void k_rs_rows(uint64_t n, const uint32_t *__restrict__ sid,
                                                        const int32_t *__restrict__ sstart, const int32_t *__restrict__ reach,
                                                        const uint32_t *__restrict__ open, const uint64_t *__restrict__ ord,
                                                        uint32_t *__restrict__ m_id, int32_t *__restrict__ m_start,
                                                        int32_t *__restrict__ m_end) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t row = ord[j] + open[j] - 1u;  // (element 0 opens a row: never -1)
    if (open[j]) {
        m_id[row] = sid[j];
        m_start[row] = sstart[j];
    }
    if (j + 1 == n || open[j + 1]) m_end[row] = reach[j];
}

using RsTable = RsTableArgs;  // (read through a pointer: by value its nine fields spill scalar registers)

__device__ __forceinline__ uint64_t rs_wave_sum64(uint64_t x) {
    return (uint64_t)wave_sum<unsigned long long>((unsigned long long)x);
}

__global__ __launch_bounds__(kRsThreads) void k_rs_dict(uint32_t n_chrom, const char *__restrict__ names,
                                                        const uint64_t *__restrict__ name_off, uint64_t hash_mask,
                                                        uint32_t dict_mask, uint32_t *dict) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_chrom) return;
    const int64_t s = (int64_t)name_off[id], e = (int64_t)name_off[id + 1];
    uint64_t sum = 0;
    for (int64_t p = s; p < e; p++) sum += hash_byte(byte_at(names, p), (uint64_t)(p - s));
    uint32_t slot = (uint32_t)(hash_field(sum, (uint64_t)(e - s)) & hash_mask) & dict_mask;
    while (atomicCAS(&dict[slot], 0u, id + 1u) != 0u) slot = (slot + 1u) & dict_mask;
}

// ---- the per-line pass -------------------------------------------------------------------------

struct RsArgs {
    const char *buf;
    int64_t data_start;
    const uint64_t *line_end;
    uint64_t L;
    int stdin_mode;
};

// CHROM = buf[cs, cs + clen) with the field hash fc: its id's range searched for POS
__device__ __forceinline__ uint8_t rs_lookup(const RsTable *__restrict__ T, const char *__restrict__ buf, int64_t cs, int64_t clen,
                                             uint64_t fc, int32_t pos) {
    uint32_t slot = (uint32_t)(fc & T->hash_mask) & T->dict_mask;
    for (;;) {
        const uint32_t e = T->dict[slot];
        if (!e) return kRsOut;  // the name is not in the BED
        const int64_t ns = (int64_t)T->name_off[e - 1u], nn = (int64_t)T->name_off[e] - ns;
        if (nn == clen && cmp_bytes(buf, cs, clen, T->names, ns, nn) == 0) {
            const uint32_t f = T->first[e - 1u];
            uint32_t lo = f, hi = T->last[e - 1u];
            while (lo < hi) {  // the first start > pos
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (T->start[mid] <= pos) lo = mid + 1u;
                else hi = mid;
            }
            return lo > f && T->reach[lo - 1u] >= pos ? kRsIn : kRsOut;
        }
        slot = (slot + 1u) & T->dict_mask;
    }
}

// std::stoi's verdict on a field read byte by byte: C white space, one sign, digits
struct RsStoi {
    uint32_t state = 0;  // 0 leading white space, 1 digits, 2 the rest (ignored)
    bool any = false, neg = false, big = false;
    uint64_t mag = 0;
    __device__ __forceinline__ void byte(uint32_t b) {
        if (state == 0) {
            if (b == ' ' || (b >= 9u && b <= 13u)) return;
            state = 1;
            if (b == '-' || b == '+') {
                neg = b == '-';
                return;
            }
        }
        if (state == 1) {
            const uint32_t d = b - '0';
            if (d <= 9u) {
                any = true;
                if (mag > (1ull << 31)) big = true;  // (stays outside int whatever follows)
                else mag = mag * 10u + d;
            } else {
                state = 2;
            }
        }
    }
    __device__ __forceinline__ bool ok() const { return any && !big && mag <= (neg ? (1ull << 31) : (1ull << 31) - 1u); }
    __device__ __forceinline__ int32_t value() const { return (int32_t)(uint32_t)(neg ? 0ull - mag : mag); }
};

// The lane's line [ls, le) over its first kRsWindow bytes; false: the wave takes it.
__device__ __forceinline__ bool rs_lane_line(const RsArgs &A, const RsTable *__restrict__ T, int64_t ls, int64_t le, uint8_t &st) {
    const char *__restrict__ buf = A.buf;
    const int64_t we = le - ls > kRsWindow ? ls + kRsWindow : le;
    uint32_t nt = 0, pv = 0;
    uint64_t sum = 0, idx = 0, fc = 0;
    int64_t t0 = 0, t1 = -1;
    RsStoi sp;
    int64_t a = ls & ~(int64_t)15;
    uint4 v = uint4{0, 0, 0, 0};
    for (; a < we && t1 < 0; a += 16) {
        v = load16(buf, a);
        const uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
        const int j0 = a < ls ? (int)(ls - a) : 0, j1 = we - a < 16 ? (int)(we - a) : 16;
        for (int j = j0; j < j1; j++) {
            const uint32_t b = (uint32_t)((j < 8 ? lo : hi) >> (8 * (j & 7))) & 0xFFu;
            if (b == '\t') {
                if (nt == 0) {
                    fc = hash_field(sum, idx);
                    t0 = a + j;
                    nt = 1;
                } else {
                    t1 = a + j;
                    nt = 2;
                    break;
                }
            } else if (nt == 0) {
                sum += hash_byte(b, idx);
                idx++;
            } else if (A.stdin_mode) {
                sp.byte(b);
            } else {
                const uint32_t d = b - '0';
                if (d <= 9u) pv = pv * 10u + d;  // (modulo 2^32: the reference's int wraps)
            }
        }
    }
    // (after the loop `a` is one block past the last one loaded, `v`)
    if (nt < 2 && we < le) return false;  // CHROM or POS may go on past the window
    int32_t pos;
    if (!A.stdin_mode) {
        const int64_t pe = nt == 2 ? t1 : le;
        if (nt == 0 || t0 == ls || pe == t0 + 1) {
            st = kRsShort;
            return true;
        }
        pos = (int32_t)pv;
    } else {
        // five more tabs after the second, from the byte masks
        uint32_t more = 0;
        if (nt == 2) {
            more = (uint32_t)__popc(eq_mask16(v, kRepTab) & range_mask16(a - 16, t1 + 1, we));
            for (; a < we && more < 5u; a += 16) more += (uint32_t)__popc(eq_mask16(load16(buf, a), kRepTab) & range_mask16(a, ls, we));
        }
        if (nt < 2 || more < 5u) {
            if (we < le) return false;  // the seventh tab may lie past the window
            st = kRsShort;
            return true;
        }
        if (!sp.ok()) {
            st = kRsBadPos;
            return true;
        }
        pos = sp.value();
    }
    st = rs_lookup(T, buf, ls, t0 - ls, fc, pos);
    return true;
}

// The wave's line [ls, le) (uniform; every lane active): any width.
__device__ __forceinline__ uint8_t rs_wave_line(const RsArgs &A, const RsTable *__restrict__ T, int64_t ls, int64_t le, int64_t *lds) {
    const char *__restrict__ buf = A.buf;
    int64_t t[7];
    const int want = A.stdin_mode ? 7 : 2;
    const int nt = head_tabs(buf, ls, le, want, t, lds);
    int32_t pos;
    if (A.stdin_mode) {
        if (nt < 7) return kRsShort;
        const CInteger c = parse_c_integer(buf, t[0] + 1, t[1]);
        if (!c.any || !c.fits_int()) return kRsBadPos;
        pos = (int32_t)(uint32_t)c.bits();
    } else {
        const int64_t pe = nt == 2 ? t[1] : le;
        if (nt == 0 || t[0] == ls || pe == t[0] + 1) return kRsShort;
        uint32_t pv = 0;
        for (int64_t p = t[0] + 1; p < pe; p++) {  // (every lane the same bytes: POS fields are short)
            const uint32_t d = byte_at(buf, p) - '0';
            if (d <= 9u) pv = pv * 10u + d;
        }
        pos = (int32_t)pv;
    }
    uint64_t sum = 0;
    for (int64_t p = ls + lane(); p < t[0]; p += kWave) sum += hash_byte(byte_at(buf, p), (uint64_t)(p - ls));
    const uint64_t fc = hash_field(rs_wave_sum64(sum), (uint64_t)(t[0] - ls));
    return rs_lookup(T, buf, ls, t[0] - ls, fc, pos);
}

// counters[7]: the queued lines; counters[8]: the index of the first line that starts with "#CHROM"
// (set to L beforehand)
__global__ __launch_bounds__(kRsThreads) void k_rs_class(RsArgs A, const RsTable *__restrict__ T, uint8_t *__restrict__ status,
                                                         uint32_t *__restrict__ queue, unsigned long long *__restrict__ counters) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < A.L; li += nth) {
        const int64_t ls = line_start(A.line_end, A.data_start, li), le = (int64_t)A.line_end[li];
        uint8_t st = kRsEmpty;
        bool have = true;
        if (le > ls) {
            if (byte_at(A.buf, ls) == '#') {
                st = kRsHeader;
                if (le - ls >= 6 && byte_at(A.buf, ls + 1) == 'C' && byte_at(A.buf, ls + 2) == 'H' && byte_at(A.buf, ls + 3) == 'R' &&
                    byte_at(A.buf, ls + 4) == 'O' && byte_at(A.buf, ls + 5) == 'M')
                    atomicMin(&counters[8], (unsigned long long)li);
            } else {
                have = rs_lane_line(A, T, ls, le, st);
            }
        }
        if (have) status[li] = st;
        else queue[atomicAdd(&counters[7], 1ull)] = (uint32_t)li;
    }
}

__global__ __launch_bounds__(kRsThreads) void k_rs_class_wave(RsArgs A, const RsTable *__restrict__ T, uint8_t *__restrict__ status,
                                                              const uint32_t *__restrict__ queue,
                                                              const unsigned long long *__restrict__ counters) {
    __shared__ int64_t s_tabs[kRsWaves][10];
    const uint64_t nq = counters[7];
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t q = wid; q < nq; q += nw) {
        const uint64_t li = (uint64_t)uniform32((int)queue[q]);
        const int64_t ls = uniform64(line_start(A.line_end, A.data_start, li)), le = uniform64((int64_t)A.line_end[li]);
        const uint8_t st = rs_wave_line(A, T, ls, le, s_tabs[threadIdx.x / kWave]);
        if (lane() == 0) status[li] = st;
    }
}

// a data line before the first "#CHROM" line is kRsEarly; counters[st] += the lines of each status
__global__ __launch_bounds__(kRsThreads) void k_rs_finish(uint64_t L, uint8_t *__restrict__ status,
                                                          unsigned long long *__restrict__ counters) {
    __shared__ unsigned int red[7];
    if (threadIdx.x < 7) red[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t first_chrom = counters[8];
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    uint32_t k[7] = {0, 0, 0, 0, 0, 0, 0};
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < L; li += nth) {
        uint8_t st = status[li];
        if (st >= kRsIn && li < first_chrom) {
            st = kRsEarly;
            status[li] = st;
        }
#pragma unroll
        for (int i = 0; i < 7; i++) k[i] += st == i ? 1u : 0u;
    }
    tally_status(k, red, counters);
}

// ---- launchers ---------------------------------------------------------------------------------

hipError_t launch_rs_keys(uint64_t n, const uint32_t *id, const int32_t *start, uint64_t *keys, uint32_t *vals, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rs_keys, flat_grid(n, kRsThreads), dim3(kRsThreads), 0, s, n, id, start, keys, vals);
    return hipGetLastError();
}

uint64_t rs_scan_tiles(uint64_t n) { return (n + kRsTile - 1) / kRsTile; }

hipError_t launch_rs_table(uint64_t n, const uint64_t *keys, const uint32_t *vals, const int32_t *end, uint32_t *sid,
                           int32_t *sstart, uint64_t *scan_key, uint64_t *tile_max, int32_t *reach, uint32_t *first,
                           uint32_t *last, uint32_t *open, hipStream_t s) {
    if (!n) return hipSuccess;
    const dim3 flat = flat_grid(n, kRsThreads), tiles((unsigned)rs_scan_tiles(n));
    hipLaunchKernelGGL(k_rs_sorted, flat, dim3(kRsThreads), 0, s, n, keys, vals, end, sid, sstart, scan_key);
    hipLaunchKernelGGL(k_rs_tile_max, tiles, dim3(kRsThreads), 0, s, n, scan_key, tile_max);
    hipLaunchKernelGGL(k_rs_carry, dim3(1), dim3(kRsThreads), 0, s, rs_scan_tiles(n), tile_max);
    hipLaunchKernelGGL(k_rs_reach, tiles, dim3(kRsThreads), 0, s, n, scan_key, tile_max, reach);
    hipLaunchKernelGGL(k_rs_bounds, flat, dim3(kRsThreads), 0, s, n, sid, sstart, reach, first, last, open);
    return hipGetLastError();
}

hipError_t launch_rs_rows(uint64_t n, const uint32_t *sid, const int32_t *sstart, const int32_t *reach, const uint32_t *open,
                          const uint64_t *ord, uint32_t *m_id, int32_t *m_start, int32_t *m_end, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rs_rows, flat_grid(n, kRsThreads), dim3(kRsThreads), 0, s, n, sid, sstart, reach, open, ord, m_id,
                       m_start, m_end);
    return hipGetLastError();
}

hipError_t launch_rs_dict(uint32_t n_chrom, const char *names, const uint64_t *name_off, uint32_t hash_bits,
                          uint32_t dict_mask, uint32_t *dict, hipStream_t s) {
    if (!n_chrom) return hipSuccess;
    hipLaunchKernelGGL(k_rs_dict, flat_grid(n_chrom, kRsThreads), dim3(kRsThreads), 0, s, n_chrom, names, name_off,
                       rs_hash_mask(hash_bits), dict_mask, dict);
    return hipGetLastError();
}

hipError_t launch_rs_class(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t L, int stdin_mode,
                           const RsTableArgs *T, uint8_t *status, uint32_t *queue, unsigned long long *counters,
                           hipStream_t s) {
    if (!L) return hipSuccess;
    const RsArgs A{buf, data_start, line_end, L, stdin_mode ? 1 : 0};
    hipLaunchKernelGGL(k_rs_class, dim3(grid_for(L, kRsThreads, 8192)), dim3(kRsThreads), 0, s, A, T, status, queue, counters);
    hipLaunchKernelGGL(k_rs_class_wave, dim3(grid_for(L, kRsWaves, 2048)), dim3(kRsThreads), 0, s, A, T, status, queue,
                       counters);
    hipLaunchKernelGGL(k_rs_finish, dim3(grid_for(L, kRsThreads * 16, 1024)), dim3(kRsThreads), 0, s, L, status, counters);
    return hipGetLastError();
}

}  // namespace vcfxg
