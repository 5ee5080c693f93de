// vcfxg_gather.hip -- the ordered-text stage of the keyed line tools (VCFX_sorter, VCFX_merger,
// VCFX_diff_tool): lines of a resident text, in a given order, copied into one contiguous text.
//   k_line_len    output line j's bytes (with its '\n') and its first input byte; their scan places
//                 every line.
//   k_text_gather the text: every wave owns aligned 16 KiB (short texts: 4 KiB) spans of the output, finds the lines of a
//                 span by a search in the offsets (from a proportional guess), and each lane builds 16 output bytes from the
//                 pieces of the lines that cover them (two aligned 16 B loads realigned with
//                 v_alignbyte_b32 per piece) and writes them with one aligned 16 B store.
#include "vcfxg_keyed.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kGatherThreads = 256;
constexpr int kGatherWaves = kGatherThreads / kWave;
// wave-steps of 1 KiB per span, the output bytes a wave takes at a time: 16 for a text of
// kGatherLongText bytes or more (fewer span searches per byte: 2 to 9 % on the bench shard), else 4 (a
// 20 MB text then still makes 5,000 spans: 0.041 ms against 0.091 ms with 16)
constexpr int kGatherSpanSteps = 16, kGatherSpanStepsShort = 4;
constexpr uint64_t kGatherLongText = 64ull << 20;

__global__ __launch_bounds__(kGatherThreads) void k_line_len(int64_t data_start, const uint64_t *__restrict__ line_end, uint64_t nw,
                                                             const uint32_t *__restrict__ order, uint64_t *__restrict__ len,
                                                             uint64_t *__restrict__ src) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j > nw) return;
    if (j == nw) {
        len[j] = 0;
        return;
    }
    const uint32_t li = order[j];
    const int64_t ls = line_start(line_end, data_start, li);
    len[j] = (uint64_t)((int64_t)line_end[li] - ls) + 1u;
    src[j] = (uint64_t)ls;
}

// the last j in [lo, hi] with off[j] <= g (off[lo] <= g)
__device__ __forceinline__ uint64_t gather_find(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t g) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the same from a guess: gallop away from it, then the search in what is left (lines of like
// lengths put the guess within a few lines: a handful of dependent loads, not log2 of all lines)
__device__ __forceinline__ uint64_t gather_find_near(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t g,
                                                     uint64_t guess) {
    uint64_t j = guess < lo ? lo : guess > hi ? hi : guess;
    uint64_t step = 1;
    if (off[j] <= g) {
        while (j + step <= hi && off[j + step] <= g) {
            j += step;
            step <<= 1;
        }
        return gather_find(off, j, j + step < hi ? j + step : hi, g);
    }
    uint64_t top;  // (off[lo] <= g < off[j]: j > lo)
    do {
        top = j - 1;
        j = j - lo > step ? j - step : lo;
        step <<= 1;
    } while (off[j] > g);
    return gather_find(off, j, top, g);
}

template <bool kNt>
__device__ __forceinline__ uint4 gather_load16(const char *buf, int64_t a) {
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
__device__ __forceinline__ uint4 gather_bytes16(const char *buf, int64_t s) {
    const int64_t a = s & ~(int64_t)15;
    const uint4 A = gather_load16<kNt>(buf, a);
    const uint32_t sh = (uint32_t)(s & 15);
    if (sh == 0) return A;
    const uint4 B = gather_load16<kNt>(buf, a + 16);
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
__device__ __forceinline__ void gather_merge(uint4 &v, const uint4 &c, int t0, int t1) {
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
__global__ __launch_bounds__(kGatherThreads) void k_text_gather(const char *__restrict__ buf, const uint64_t *__restrict__ off,
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
        const uint64_t j0 = (uint64_t)uniform64((int64_t)gather_find_near(off, first, last, base + o0, first + (uint64_t)((double)o0 * per_byte)));
        const uint64_t j1 = (uint64_t)uniform64((int64_t)gather_find_near(off, j0, last, base + o1 - 1, j0 + (uint64_t)((double)(o1 - o0) * per_byte)));
        for (int s = 0; s < steps; s++) {
            const uint64_t o = o0 + (uint64_t)s * kWaveStep + (uint64_t)lane() * 16u;
            if (o >= o1) continue;
            const uint64_t g = base + o;
            uint64_t j = j0 == j1 ? j0 : gather_find(off, j0, j1, g);
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
                        gather_merge(v, gather_bytes16<kNtLoad>(buf, sv), t, t1);
                    } else {  // (a line within the input's first 15 bytes)
                        for (int i = t; i < t1; i++) {
                            const uint4 c = uint4{byte_at(buf, sv + i) * 0x01010101u, byte_at(buf, sv + i) * 0x01010101u,
                                                  byte_at(buf, sv + i) * 0x01010101u, byte_at(buf, sv + i) * 0x01010101u};
                            gather_merge(v, c, i, i + 1);
                        }
                    }
                }
                t = t1;
                if (t < 16) {
                    gather_merge(v, uint4{kRepNl, kRepNl, kRepNl, kRepNl}, t, t + 1);
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

hipError_t launch_line_len(int64_t data_start, const uint64_t *line_end, uint64_t nw, const uint32_t *order, uint64_t *len,
                           uint64_t *src, hipStream_t s) {
    hipLaunchKernelGGL(k_line_len, flat_grid(nw + 1, kGatherThreads), dim3(kGatherThreads), 0, s, data_start, line_end, nw,
                       order, len, src);
    return hipGetLastError();
}

hipError_t launch_text_gather(const char *buf, const uint64_t *off, const uint64_t *src, uint64_t first, uint64_t k,
                              uint64_t bytes, int nt, char *text, hipStream_t s) {
    if (!k || !bytes) return hipSuccess;
    const int steps = bytes >= kGatherLongText ? kGatherSpanSteps : kGatherSpanStepsShort;
    const uint64_t spans = (bytes + (uint64_t)steps * kWaveStep - 1) / ((uint64_t)steps * kWaveStep);
    const dim3 grid(grid_for(spans, kGatherWaves, 4096)), block(kGatherThreads);
    switch (nt & 3) {
        case 1: hipLaunchKernelGGL(k_text_gather<1>, grid, block, 0, s, buf, off, src, first, k, bytes, steps, text); break;
        case 2: hipLaunchKernelGGL(k_text_gather<2>, grid, block, 0, s, buf, off, src, first, k, bytes, steps, text); break;
        case 3: hipLaunchKernelGGL(k_text_gather<3>, grid, block, 0, s, buf, off, src, first, k, bytes, steps, text); break;
        default: hipLaunchKernelGGL(k_text_gather<0>, grid, block, 0, s, buf, off, src, first, k, bytes, steps, text); break;
    }
    return hipGetLastError();
}

}  // namespace vcfxg
