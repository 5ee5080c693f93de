// vcfxg_sx.hip -- VCFX_sample_extractor's column selection (VCFX_sample_extractor.cpp:206-335
// file mode, :458-539 stdin mode): a text rewrite whose output is a byte-granular selection of
// the input.
//
// Byte model.  Number the fields of a line from 0 and give a tab the number of the field it
// precedes.  A written data line is: every byte numbered 0..8, every byte whose number is a kept
// column (so a kept field comes with the tab in front of it), "\t." for each kept column the
// line lacks (all of them past the line's last field, so the order holds), and one '\n'.  The
// kept numbers are one bitmask (bits 0..8 always set) of last-kept-column + 1 bits, in LDS when it
// fits kSxMaskLds bytes and in global memory otherwise.  An empty line is "\n"; a '#' line is
// copied ('\r' stripped in file mode) by the same walk with every byte kept.
//
// Two passes over the indexed lines, one wave per line, 16 B per lane per step (1 KiB a step):
//   k_sx_len    the line's status and output bytes: tab masks from the loaded bytes, the running
//               tab count carried across the lanes by a DPP scan and across the steps in a
//               scalar register, 32 mask bits fetched at the lane's first field number, the kept
//               bytes counted.  The walk stops at the step that ends the last kept column.
//   (scan)      hipcub exclusive sum of the lengths: each line's output offset
//   k_sx_write  the same walk; each lane's runs of kept bytes go to the wave's LDS ring at the
//               position the scan of the kept counts gives (dword stores inside a run, byte stores
//               at its ragged ends), and every complete 16 B piece of the ring is flushed with
//               one aligned 16 B store.  Ring position q is output byte G0 + q with G0 the
//               line's output offset rounded down to 16, so only a line's first and last piece
//               (shared with the neighbouring lines, written by other waves) use byte stores.
//               The ring is drained every step, so a line of any width passes through it: the tab
//               count, the ring position and the output offset are the carried state.
#include <type_traits>

#include "vcfxg_device.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kSxThreads = 256;
constexpr int kSxWaves = kSxThreads / kWave;
constexpr uint32_t kSxStage = 2048;  // ring bytes per wave: a step's 1 KiB + the < 16 B not yet flushed, a power of two
constexpr uint32_t kSxRing = kSxStage - 1;
constexpr uint32_t kSxMaskLds = 32768;  // mask bytes kept in LDS (262,144 columns); larger: global loads

struct SxArgs {
    const uint32_t *mask;  // nwords + 2 words: bit f = field f is kept (0..8 set), two zero words behind
    uint32_t nwords;
    uint32_t lastk;        // the largest kept field number (8 without a kept column)
    uint32_t m;            // kept columns
    int stdin_mode;        // VCFXG_MODE_STDIN: no '\r' strip, '#CHROM' lines flagged, 8-field lines skipped
    int seen;              // a '#CHROM' line precedes the range
};

struct SxMaskLds {
    const uint32_t *w;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return w[i]; }
};
struct SxMaskGlobal {
    const uint32_t *__restrict__ w;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return __ldg(w + i); }
};

// The walk over [ls, le): sink.step(v, km) per 1 KiB step with the lane's 16 bytes and the mask
// of its kept bytes (every lane of the wave calls it).  all: every byte is kept and no tab is
// counted.  Returns the tabs seen, exact up to lastk and at least lastk + 1 past it.
template <typename Mask, typename Sink>
__device__ __forceinline__ uint32_t sx_walk(const char *__restrict__ buf, int64_t ls, int64_t le, bool all,
                                            const SxArgs &A, const Mask &M, Sink &sink) {
    uint32_t carry = 0;  // tabs before this step (wave-uniform)
    for (int64_t w = ls & ~(int64_t)15; w < le; w += kWaveStep) {
        const int64_t blk = w + (int64_t)lane() * kBlockBytes;
        uint4 v{0u, 0u, 0u, 0u};
        uint32_t rm = 0;
        if (blk < le) {
            v = load16(buf, blk);
            rm = range_mask16(blk, ls, le);
        }
        uint32_t km = rm;
        if (!all) {
            const uint32_t tm = eq_mask16(v, kRepTab) & rm;
            const uint32_t c = (uint32_t)__popc(tm);
            const uint32_t incl = wave_incl_scan32(c);
            const uint32_t base = carry + incl - c;  // the field number of the lane's first byte
            carry += lane_last(incl);
            // mask bits [base, base + 32): the lane's 16 bytes span at most 17 fields
            const uint32_t i0 = min(base >> 5, A.nwords), i1 = min(i0 + 1u, A.nwords + 1u);
            uint32_t kb = (uint32_t)((((uint64_t)M(i1) << 32) | M(i0)) >> (base & 31u));
            km = 0;
            uint32_t t = tm, prev = 0;
            for (;;) {  // the bytes before the first tab, then from each tab (inclusive) to the next
                const uint32_t p = t ? (uint32_t)__builtin_ctz(t) : 16u;
                if (kb & 1u) km |= ((1u << p) - 1u) & ~((1u << prev) - 1u);
                if (!t) break;
                t &= t - 1u;
                prev = p;
                kb >>= 1;
            }
            km &= rm;
        }
        sink.step(v, km);
        if (!all && carry > A.lastk) break;
    }
    return carry;
}

// kept columns the line lacks: mask bits at or past max(nf, 9)
template <typename Mask>
__device__ __forceinline__ uint32_t sx_missing(const SxArgs &A, const Mask &M, uint32_t nf) {
    if (A.m == 0 || nf > A.lastk) return 0;
    const uint32_t lo = nf < 9u ? 9u : nf;
    uint32_t cnt = 0;
    for (uint32_t wi = lo / 32u + (uint32_t)lane(); wi < A.nwords; wi += kWave) {
        uint32_t x = M(wi);
        if (wi * 32u < lo) x &= ~0u << (lo - wi * 32u);
        cnt += (uint32_t)__popc(x);
    }
    return wave_sum32(cnt);
}

struct SxLenSink {
    uint32_t cnt = 0;
    __device__ __forceinline__ void step(const uint4 &, uint32_t km) { cnt += (uint32_t)__popc(km); }
};

__device__ __forceinline__ bool sx_is_chrom(const char *__restrict__ buf, int64_t ls, int64_t le) {
    return le - ls >= 6 && byte_at(buf, ls + 1) == 'C' && byte_at(buf, ls + 2) == 'H' && byte_at(buf, ls + 3) == 'R' &&
           byte_at(buf, ls + 4) == 'O' && byte_at(buf, ls + 5) == 'M';
}

// the mask into LDS (kLds) by the whole block
template <bool kLds>
__device__ __forceinline__ void sx_load_mask(const SxArgs &A, uint32_t *s_mask) {
    if (kLds) {
        for (uint32_t i = threadIdx.x; i < A.nwords + 2u; i += blockDim.x) s_mask[i] = A.mask[i];
        __syncthreads();
    }
}

template <bool kLds>
__global__ __launch_bounds__(kSxThreads) void k_sx_len(const char *__restrict__ buf, int64_t data_start,
                                                       const uint64_t *__restrict__ line_end, uint64_t l0, uint64_t l1,
                                                       SxArgs A, uint8_t *__restrict__ status, uint64_t *__restrict__ len,
                                                       unsigned long long *__restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mask[];
    __shared__ unsigned long long red[4][kSxWaves];
    sx_load_mask<kLds>(A, s_mask);
    const typename std::conditional<kLds, SxMaskLds, SxMaskGlobal>::type M{kLds ? s_mask : A.mask};
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    uint32_t rows = 0, data = 0, warn = 0, chrom = 0;  // (wave-uniform)
    for (uint64_t li = l0 + wid; li < l1; li += nw) {
        const int64_t ls = li ? (int64_t)line_end[li - 1] + 1 : data_start;
        int64_t le = (int64_t)line_end[li];
        if (!A.stdin_mode && le > ls && byte_at(buf, le - 1) == '\r') le--;
        uint8_t st = kSxEmpty;
        uint64_t L = 1;
        if (le > ls) {
            if (byte_at(buf, ls) == '#') {
                if (A.stdin_mode && sx_is_chrom(buf, ls, le)) {
                    st = kSxChrom;
                    L = 0;
                    chrom++;
                } else {
                    st = kSxHeader;
                    L = (uint64_t)(le - ls) + 1u;
                }
            } else {
                data++;
                L = 0;
                if (!A.seen) {
                    st = kSxPre;
                    warn++;
                } else {
                    SxLenSink sink;
                    const uint32_t nf = sx_walk(buf, ls, le, false, A, M, sink) + 1u;
                    const uint64_t kept = wave_sum32(sink.cnt);
                    if (nf < 8u) {
                        st = kSxShort;
                        warn++;
                    } else if (nf == 8u && A.stdin_mode) {
                        st = kSxNoSample;
                        warn++;
                    } else {
                        st = kSxRow;
                        rows++;
                        L = kept + 2ull * sx_missing(A, M, nf) + 1u;
                    }
                }
            }
        }
        if (lane() == 0) {
            status[li] = st;
            len[li - l0] = L;
        }
    }
    if (lane() == 0) {
        red[0][threadIdx.x / kWave] = rows;
        red[1][threadIdx.x / kWave] = data;
        red[2][threadIdx.x / kWave] = warn;
        red[3][threadIdx.x / kWave] = chrom;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long t = 0;
        for (int k = 0; k < kSxWaves; k++) t += red[threadIdx.x][k];
        if (t) atomicAdd(&counters[threadIdx.x], t);
    }
}

// the wave's LDS accesses before this point are complete and visible to its other lanes
__device__ __forceinline__ void sx_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the 4 bytes at byte s (0..15) of v, zeros past its end
__device__ __forceinline__ uint32_t sx_dword(const uint4 &v, uint32_t s) {
    const uint32_t i = s >> 2;
    const uint32_t lo = i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
    const uint32_t hi = i == 0 ? v.y : i == 1 ? v.z : i == 2 ? v.w : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, s & 3u);
}

// The wave's output stream through its LDS ring.  Ring position q is output byte G0 + q; the
// line's bytes are positions [q0, ...), q0 = its output offset mod 16.
struct SxWriteSink {
    char *ring;             // kSxStage bytes, 16 B aligned
    char *__restrict__ out;
    uint64_t G0;            // output offset of ring position 0 (a multiple of 16)
    uint32_t q0;
    uint64_t fill;          // the next position to write
    uint64_t done;          // 16 B pieces flushed

    // bytes [a, a + n) of v to positions [q, q + n)
    __device__ __forceinline__ void put(uint32_t q, const uint4 &v, uint32_t a, uint32_t n) {
        uint32_t s = a, d = q;
        const uint32_t e = q + n;
        while (d != e && (d & 3u)) {
            ring[d & kSxRing] = (char)sx_dword(v, s);
            d++, s++;
        }
        while (e - d >= 4u) {
            *reinterpret_cast<uint32_t *>(ring + (d & kSxRing)) = sx_dword(v, s);
            d += 4, s += 4;
        }
        while (d != e) {
            ring[d & kSxRing] = (char)sx_dword(v, s);
            d++, s++;
        }
    }
    // every complete piece out, as aligned 16 B stores (the line's first piece, when the line
    // starts inside it, byte by byte: its first bytes are the previous line's)
    __device__ __forceinline__ void flush() {
        sx_wave_sync();
        const uint64_t c1 = fill >> 4;
        for (uint64_t c = done + (uint64_t)lane(); c < c1; c += kWave) {
            const uint32_t r = (uint32_t)(c << 4) & kSxRing;
            if (c == 0 && q0) {
                for (uint32_t j = q0; j < 16u; j++) out[G0 + j] = ring[j];
            } else {
                *reinterpret_cast<uint4 *>(out + G0 + (c << 4)) = *reinterpret_cast<const uint4 *>(ring + r);
            }
        }
        done = c1;
        sx_wave_sync();
    }
    __device__ __forceinline__ void step(const uint4 &v, uint32_t km) {
        const uint32_t n = (uint32_t)__popc(km);
        const uint32_t incl = wave_incl_scan32(n);
        uint32_t q = (uint32_t)fill + incl - n;
        uint32_t k = km;
        while (k) {  // the runs of kept bytes
            const uint32_t a = (uint32_t)__builtin_ctz(k);
            const uint32_t r = (uint32_t)__builtin_ctz(~(k >> a));
            put(q, v, a, r);
            q += r;
            k &= ~(((1u << r) - 1u) << a);
        }
        fill += lane_last(incl);
        flush();
    }
    // `pairs` times "\t." (at most 512 a step)
    __device__ __forceinline__ void dots(uint64_t pairs) {
        while (pairs) {
            const uint32_t k = (uint32_t)(pairs < 512u ? pairs : 512u);
            for (uint32_t i = (uint32_t)lane(); i < k; i += kWave) {
                const uint32_t q = (uint32_t)fill + 2u * i;
                ring[q & kSxRing] = '\t';
                ring[(q + 1u) & kSxRing] = '.';
            }
            fill += 2u * k;
            pairs -= k;
            flush();
        }
    }
    // the closing '\n' and the bytes of the last, incomplete piece
    __device__ __forceinline__ void finish() {
        if (lane() == 0) ring[(uint32_t)fill & kSxRing] = '\n';
        fill++;
        flush();
        const uint64_t from = (done << 4) > q0 ? (done << 4) : (uint64_t)q0;
        for (uint64_t p = from + (uint64_t)lane(); p < fill; p += kWave) out[G0 + p] = ring[(uint32_t)p & kSxRing];
        sx_wave_sync();
    }
};

template <bool kLds>
__global__ __launch_bounds__(kSxThreads) void k_sx_write(const char *__restrict__ buf, int64_t data_start,
                                                         const uint64_t *__restrict__ line_end, uint64_t l0, uint64_t l1,
                                                         SxArgs A, const uint8_t *__restrict__ status,
                                                         const uint64_t *__restrict__ off, char *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mask[];
    __shared__ __attribute__((aligned(16))) char ring_all[kSxWaves][kSxStage];
    sx_load_mask<kLds>(A, s_mask);
    const typename std::conditional<kLds, SxMaskLds, SxMaskGlobal>::type M{kLds ? s_mask : A.mask};
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t li = l0 + wid; li < l1; li += nw) {
        const uint8_t st = status[li];
        if (st != kSxEmpty && st != kSxHeader && st != kSxRow) continue;
        const int64_t ls = li ? (int64_t)line_end[li - 1] + 1 : data_start;
        int64_t le = (int64_t)line_end[li];
        if (!A.stdin_mode && le > ls && byte_at(buf, le - 1) == '\r') le--;
        const uint64_t o = off[li - l0], total = off[li - l0 + 1] - o;
        SxWriteSink sink{ring_all[threadIdx.x / kWave], out, o & ~15ull, (uint32_t)(o & 15u), o & 15u, 0};
        if (st != kSxEmpty) {
            sx_walk(buf, ls, le, st == kSxHeader, A, M, sink);
            const uint64_t kept = sink.fill - sink.q0;  // (+ 2 per lacking column + the '\n' = total)
            if (st == kSxRow && kept + 1u < total) sink.dots((total - 1u - kept) / 2u);
        }
        sink.finish();
    }
}

static SxArgs sx_args(const uint32_t *mask, uint32_t nwords, uint32_t lastk, uint32_t m, int stdin_mode, int seen) {
    SxArgs A;
    A.mask = mask;
    A.nwords = nwords;
    A.lastk = lastk;
    A.m = m;
    A.stdin_mode = stdin_mode;
    A.seen = seen;
    return A;
}

hipError_t launch_sx_len(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t l1,
                         unsigned blocks, const uint32_t *mask, uint32_t nwords, uint32_t lastk, uint32_t m,
                         int stdin_mode, int seen, uint8_t *status, uint64_t *len, unsigned long long *counters,
                         hipStream_t s) {
    if (l1 <= l0) return hipSuccess;
    const SxArgs A = sx_args(mask, nwords, lastk, m, stdin_mode, seen);
    const size_t mb = 4 * ((size_t)nwords + 2);
    if (mb <= kSxMaskLds)
        hipLaunchKernelGGL(k_sx_len<true>, dim3(blocks), dim3(kSxThreads), mb, s, buf, data_start, line_end, l0, l1, A,
                           status, len, counters);
    else
        hipLaunchKernelGGL(k_sx_len<false>, dim3(blocks), dim3(kSxThreads), 0, s, buf, data_start, line_end, l0, l1, A,
                           status, len, counters);
    return hipGetLastError();
}

hipError_t launch_sx_write(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t l1,
                           unsigned blocks, const uint32_t *mask, uint32_t nwords, uint32_t lastk, uint32_t m,
                           int stdin_mode, int seen, const uint8_t *status, const uint64_t *off, char *out,
                           hipStream_t s) {
    if (l1 <= l0) return hipSuccess;
    const SxArgs A = sx_args(mask, nwords, lastk, m, stdin_mode, seen);
    const size_t mb = 4 * ((size_t)nwords + 2);
    if (mb <= kSxMaskLds)
        hipLaunchKernelGGL(k_sx_write<true>, dim3(blocks), dim3(kSxThreads), mb, s, buf, data_start, line_end, l0, l1,
                           A, status, off, out);
    else
        hipLaunchKernelGGL(k_sx_write<false>, dim3(blocks), dim3(kSxThreads), 0, s, buf, data_start, line_end, l0, l1,
                           A, status, off, out);
    return hipGetLastError();
}

int sx_threads() { return kSxThreads; }
uint32_t sx_stage_bytes() { return kSxStage; }

}  // namespace vcfxg
