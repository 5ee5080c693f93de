// vcfxg_keyed.h -- device leaf functions shared by the keyed line tools (vcfxg_dd.hip, vcfxg_srt.hip,
// vcfxg_df.hip, vcfxg_mg.hip, vcfxg_gather.hip): where a line starts, the pieces of a key (its
// 8-byte words, its byte order, its hash), the tabs inside a lane's window, C's integer grammar and
// the per-status block tally.  Free functions only: no state, no kernels, no loops over lines.
#pragma once
#include "vcfxg_device.h"

namespace vcfxg {

// the first byte of indexed line li (line 0 starts at data_start)
__device__ __forceinline__ int64_t line_start(const uint64_t *line_end, int64_t data_start, uint64_t li) {
    return li ? (int64_t)line_end[li - 1] + 1 : data_start;
}

// the bytes [8 w, 8 w + 8) of [s, s + len) big-endian, zero-padded past len
__device__ __forceinline__ uint64_t key_word(const char *__restrict__ buf, int64_t s, int64_t len, uint64_t w) {
    uint64_t x = 0;
    const int64_t a = 8 * (int64_t)w;
#pragma unroll
    for (int i = 0; i < 8; i++) x = (x << 8) | (a + i < len ? (uint64_t)byte_at(buf, s + a + i) : 0ull);
    return x;
}

// the bytes [a, a + an) against [b, b + bn) as unsigned bytes, a prefix before its extensions; the
// first `from` bytes are known to be equal
__device__ __forceinline__ int cmp_bytes(const char *__restrict__ buf, int64_t a, int64_t an, int64_t b, int64_t bn,
                                         int64_t from = 0) {
    const int64_t n = an < bn ? an : bn;
    for (int64_t i = from; i < n; i++) {
        const uint32_t x = byte_at(buf, a + i), y = byte_at(buf, b + i);
        if (x != y) return x < y ? -1 : 1;
    }
    return an < bn ? -1 : an > bn ? 1 : 0;
}

// ... and the bytes [a, a + an) of one buffer against [b, b + bn) of another (a line's field against
// a side table's name)
__device__ __forceinline__ int cmp_bytes(const char *__restrict__ abuf, int64_t a, int64_t an, const char *__restrict__ bbuf,
                                         int64_t b, int64_t bn) {
    const int64_t n = an < bn ? an : bn;
    for (int64_t i = 0; i < n; i++) {
        const uint32_t x = byte_at(abuf, a + i), y = byte_at(bbuf, b + i);
        if (x != y) return x < y ? -1 : 1;
    }
    return an < bn ? -1 : an > bn ? 1 : 0;
}

// The key hashes: a byte's term is mix64((i << 8 | b) + c0), i its place in its field, token or key;
// a field of `len` bytes with the sum of its terms closes as mix64(sum ^ (len * c1 + c2)).  A sum, so
// any lane may add any byte.  mix64 = splitmix64's finaliser.
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__device__ __forceinline__ uint64_t hash_byte(uint32_t b, uint64_t i) { return mix64(((i << 8) | b) + 0x9E3779B97F4A7C15ull); }
__device__ __forceinline__ uint64_t hash_field(uint64_t sum, uint64_t len) {
    return mix64(sum ^ (len * 0xD6E8FEB86659FD93ull + 0xA0761D6478BD642Full));
}

// The first `want` (<= kWant) tabs of the line [ls, le) inside its first `window` bytes, from aligned
// 16 B loads: their offsets to t[0 ..], their number returned.  Fewer than `want` on a line longer
// than the window: the key fields may go on past it (the caller queues the line for its wave pass).
template <int kWant>
__device__ __forceinline__ int window_tabs(const char *__restrict__ buf, int64_t ls, int64_t le, int window, int64_t t[kWant],
                                           int want = kWant) {
    const int64_t we = le - ls > window ? ls + window : le;
    int nt = 0;
    for (int64_t a = ls & ~(int64_t)15; a < we && nt < want; a += 16) {
        uint32_t m = eq_mask16(load16(buf, a), kRepTab) & range_mask16(a, ls, we);
        while (m && nt < want) {
            t[nt++] = a + __builtin_ctz(m);
            m &= m - 1u;
        }
    }
    return nt;
}

// C's strtol front end over [s, end): white space (' ', 9..13) skipped, one sign, decimal digits,
// the rest ignored.  any: a digit was read; overflow64: the value is outside long (the exact test:
// v * 10 + b > lim), magnitude then stops short of it.  Each caller puts its own range and failure
// rule on top.
struct CInteger {
    bool any, neg, overflow64;
    uint64_t magnitude;
    // the value as a two's complement word (|value| <= 2^63)
    __device__ __forceinline__ uint64_t bits() const { return neg ? 0ull - magnitude : magnitude; }
    // ... and whether it lies in int
    __device__ __forceinline__ bool fits_int() const {
        return !overflow64 && magnitude <= (neg ? (1ull << 31) : (1ull << 31) - 1u);
    }
};
__device__ __forceinline__ CInteger parse_c_integer(const char *__restrict__ buf, int64_t s, int64_t end) {
    int64_t p = s;
    uint32_t b = 0;
    while (p < end && ((b = byte_at(buf, p)) == ' ' || (b >= 9u && b <= 13u))) p++;
    CInteger r{false, false, false, 0};
    if (p < end && ((b = byte_at(buf, p)) == '-' || b == '+')) {
        r.neg = b == '-';
        p++;
    }
    const uint64_t lim = r.neg ? (1ull << 63) : (1ull << 63) - 1u;
    while (p < end && (b = byte_at(buf, p) - '0') <= 9u) {
        r.any = true;
        if (!r.overflow64) {
            if (r.magnitude > (lim - b) / 10u) r.overflow64 = true;
            else r.magnitude = r.magnitude * 10u + b;
        }
        p++;
    }
    return r;
}

// The end of a class kernel: the lanes' counts per status k[0 .. kN) summed over the wave, over the
// block (red[0 .. kN): shared, zeroed before the kernel's loop) and added to counters[0 .. kN) with one
// global atomic per status and block.  Every thread of the block calls it (it holds a barrier); a
// block reduction of the kernel's own (the longest CHROM) goes into shared memory before the call
// and is read after it.
template <int kN>
__device__ __forceinline__ void tally_status(const uint32_t (&k)[kN], unsigned int *red, unsigned long long *counters) {
#pragma unroll
    for (int i = 0; i < kN; i++) {
        const uint32_t t = wave_sum(k[i]);
        if (lane() == 0 && t) atomicAdd(&red[i], t);
    }
    __syncthreads();
    if (threadIdx.x < kN && red[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)red[threadIdx.x]);
}

}  // namespace vcfxg
