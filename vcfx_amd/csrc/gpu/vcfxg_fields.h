// vcfxg_fields.h -- "find key K inside a field, hand back its span": the wave-parallel searches the
// INFO and FORMAT tools share (beside vcfxg_keyed.h).  Free functions without state: a wave calls them
// with every lane active on a span [a, b) of the line [ls, le) (offsets from the line's start), and
// they answer through a callback that every lane reaches with the same arguments.
//
// A token sweep walks the span 1 KiB a step, 16 B per lane, every load an aligned load16 of a block
// that holds a byte of the span (so of the line: no byte of another line decides anything).  The
// span's end counts as one more separator, set in the mask and never read.  A token is
// [start, d): start = the byte after the separator before it (the span's first byte for the first
// token), d = the separator that closes it; its key ends at the token's first '=' (INFO) or at d.
// The lane that owns d examines the token.  What it needs from the bytes before its block comes from
// two maximum scans over the lanes and, across the steps, from the carried state TokCarry:
//   last   the position + 1 of the last separator seen (0: none yet, the token starts at a)
//   eq     the position + 1 of the first '=' after it (0: none yet)
//   nsep   the separators seen: the ordinal of the token that is open
// so a token, a key or a value that crosses a step (or many) costs nothing but the carry: there is no
// scalar loop over a span's bytes.  A key is compared with the length test first; only a token of the
// key's length has its bytes compared (re-read with load16 from the cache the sweep just filled).
#pragma once
#include "vcfxg_device.h"

namespace vcfxg {

constexpr uint32_t kFieldNone = 0xFFFFFFFFu;
constexpr uint32_t kRepSemi = 0x3B3B3B3Bu, kRepEq = 0x3D3D3D3Du;

// which tokens a search examines
enum FieldRule : int {
    kTokAll = 0,       // every token, the empty ones too (FORMAT's sub-fields)
    kTokBeforeEnd = 1, // the tokens that start before the span's end (INFO pairs as a memchr walk meets them)
    kTokNonEmpty = 2,  // the tokens that hold a byte (INFO pairs as a map of the non-empty ones holds them)
};

struct TokCarry {
    uint32_t last, eq, nsep;
};

template <typename T>
__device__ __forceinline__ T wave_incl_max(T v) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane() >= o && t > v) v = t;
    }
    return v;
}

// byte j (0..15) of the 16 loaded bytes
__device__ __forceinline__ uint32_t byte16(const uint4 &v, uint32_t j) {
    const uint32_t i = j >> 2;
    const uint32_t w = i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
    return (w >> ((j & 3u) * 8u)) & 0xFFu;
}

// the line's bytes [s, s + K.len(k)) equal key k (K.byte(k, i) = the key's byte i); one lane's work
template <typename Keys>
__device__ __forceinline__ bool span_equals(const char *__restrict__ buf, int64_t ls, uint32_t s, const Keys &K, uint32_t k) {
    const uint32_t n = K.len(k);
    const int64_t p = ls + (int64_t)s;
    uint4 v{0u, 0u, 0u, 0u};
    bool same = true;
    for (uint32_t i = 0; same && i < n; i++) {
        const uint32_t j = (uint32_t)(p + i) & 15u;
        if (i == 0u || j == 0u) v = load16(buf, (p + i) & ~(int64_t)15);  // (holds byte s + i of the token: inside the line)
        same = byte16(v, j) == K.byte(k, i);
    }
    return same;
}

// The token sweep over [a, b) with separator bytes sep_rep (replicated): for each of the nk keys and
// each step in which a token's key equals it, hit(k, start, e, d, ord) with the step's first such
// token (or its last when `last`): key [start, e), token [start, d), e < d where an '=' ended the key,
// ord = the separators before the token.  Tokens come in rising order through the steps, so the first
// call for a key is its first match and the last call its last.  kEq: an '=' ends the key.
template <bool kEq, typename Keys, typename Hit>
__device__ __forceinline__ void find_tokens(const char *__restrict__ buf, int64_t ls, int64_t le, uint32_t a, uint32_t b,
                                            uint32_t sep_rep, int rule, bool last, uint32_t nk, const Keys &K, Hit &hit) {
    TokCarry c{0u, 0u, 0u};
    const int len = (int)(le - ls);
    for (int w = (int)a - (int)((ls + (int64_t)a) & 15); w <= (int)b; w += kWaveStep) {
        const int rb = w + lane() * kBlockBytes;  // the block's first byte, from the line's start (negative before it)
        uint4 v{0u, 0u, 0u, 0u};
        if (rb < (int)b && rb < len) v = load16(buf, ls + (int64_t)rb);
        const uint32_t in = range16(rb, (int)a, (int)b);
        uint32_t S = eq_mask16(v, sep_rep) & in;
        if (rb <= (int)b && (int)b < rb + 16) S |= 1u << ((int)b - rb);  // the span's end closes the last token
        const uint32_t E = kEq ? eq_mask16(v, kRepEq) & in : 0u;
        // the lane's own summary: its last separator, the first '=' after it
        const uint32_t hi = S ? 31u - (uint32_t)__clz((int)S) : 0u;
        const uint32_t lastS = S ? (uint32_t)(rb + (int)hi) + 1u : 0u;
        const uint32_t Em = S ? E & ~((2u << hi) - 1u) : E;
        const uint32_t Qb = Em ? (uint32_t)(rb + __builtin_ctz(Em)) + 1u : 0u;
        // (last separator << 32 | ~first '=' after it): the maximum takes the latest separator, then the earliest '='
        const uint32_t Linc = wave_incl_max(lastS);
        const uint64_t Winc = wave_incl_max(((uint64_t)Linc << 32) | (uint64_t)(Qb ? ~Qb : 0u));
        uint64_t Wex = __shfl_up(Winc, 1);
        if (lane() == 0) Wex = 0;
        uint32_t Lin = (uint32_t)(Wex >> 32), Qin = (uint32_t)Wex ? ~(uint32_t)Wex : 0u;
        if (!Lin) {  // no separator in this step before the lane: the open token came in with the carry
            Lin = c.last;
            if (c.eq) Qin = c.eq;
        }
        const uint32_t cnt = (uint32_t)__popc(S);
        const uint32_t incl = wave_incl_scan32(cnt);
        const uint32_t ord0 = c.nsep + incl - cnt;
        if (__ballot(S != 0u)) {
            for (uint32_t k = 0; k < nk; k++) {
                const uint32_t kl = K.len(k);
                bool found = false;
                uint32_t hs = 0, he = 0, hd = 0, ho = 0;
                uint32_t t = S, start = Lin ? Lin : a, q = Qin, lo = 0, ord = ord0;
                while (t) {
                    const uint32_t j = (uint32_t)__builtin_ctz(t);
                    t &= t - 1u;
                    const uint32_t d = (uint32_t)(rb + (int)j);
                    uint32_t e = d;
                    if (kEq) {
                        const uint32_t Es = E & ((1u << j) - 1u) & ~((1u << lo) - 1u);
                        if (q) e = q - 1u;
                        else if (Es) e = (uint32_t)(rb + __builtin_ctz(Es));
                    }
                    const bool counts = rule == kTokAll || (rule == kTokBeforeEnd ? start < b : d > start);
                    if (counts && e - start == kl && (last || !found) && span_equals(buf, ls, start, K, k)) {
                        found = true;
                        hs = start, he = e, hd = d, ho = ord;
                    }
                    start = d + 1u, q = 0u, lo = j + 1u, ord++;
                }
                const uint64_t m = __ballot(found);
                if (m) {
                    const int src = uniform32(last ? 63 - __builtin_clzll(m) : __builtin_ctzll(m));
                    hit(k, lane_get(hs, src), lane_get(he, src), lane_get(hd, src), lane_get(ho, src));
                }
            }
        }
        const uint64_t Wall = __shfl(Winc, kWave - 1);
        const uint32_t Lall = (uint32_t)(Wall >> 32), Qall = (uint32_t)Wall ? ~(uint32_t)Wall : 0u;
        if (Lall) {
            c.last = Lall;
            c.eq = Qall;
        } else if (!c.eq) {
            c.eq = Qall;
        }
        c.nsep += lane_last(incl);
    }
}

// The INFO search: pairs split at ';', a pair's key ends at its first '='.  hit(k, start, e, d, ord)
// as above: the value is [e + 1, d) when e < d, the pair is a flag when e == d.  last = false with
// kTokBeforeEnd is the first-match walk over every pair, last = true with kTokNonEmpty the map that
// the later pair overwrites.  The caller decides what an INFO of "." or of no byte means.
template <typename Keys, typename Hit>
__device__ __forceinline__ void info_find_keys(const char *__restrict__ buf, int64_t ls, int64_t le, uint32_t a, uint32_t b,
                                               int rule, bool last, uint32_t nk, const Keys &K, Hit &hit) {
    find_tokens<true>(buf, ls, le, a, b, kRepSemi, rule, last, nk, K, hit);
}

// The FORMAT search: sub-fields split at ':', the empty ones too.  The first hit for a key carries
// its index in ord (the count of ':' before it).
template <typename Keys, typename Hit>
__device__ __forceinline__ void format_find_keys(const char *__restrict__ buf, int64_t ls, int64_t le, uint32_t a, uint32_t b,
                                                 uint32_t nk, const Keys &K, Hit &hit) {
    find_tokens<false>(buf, ls, le, a, b, kRepColon, kTokAll, false, nk, K, hit);
}

// The idx-th ':' token of [a, b): false when the span has fewer.  Carried across the steps: the colons
// counted so far; the sweep stops at the step that closes the token.
__device__ __forceinline__ bool nth_colon_token(const char *__restrict__ buf, int64_t ls, int64_t le, uint32_t a, uint32_t b,
                                                uint32_t idx, uint32_t &off, uint32_t &len) {
    uint32_t nc = 0, start = idx ? kFieldNone : a, end = kFieldNone;
    const int line = (int)(le - ls);
    for (int w = (int)a - (int)((ls + (int64_t)a) & 15); w < (int)b; w += kWaveStep) {
        const int rb = w + lane() * kBlockBytes;
        uint4 v{0u, 0u, 0u, 0u};
        if (rb < (int)b && rb < line) v = load16(buf, ls + (int64_t)rb);
        const uint32_t C = eq_mask16(v, kRepColon) & range16(rb, (int)a, (int)b);
        const uint32_t cnt = (uint32_t)__popc(C);
        const uint32_t incl = wave_incl_scan32(cnt);
        const uint32_t base = nc + incl - cnt;  // colons before the lane's block; its own are base + 1 ..
        const bool hs = idx && idx > base && idx <= base + cnt;
        const bool he = idx + 1u > base && idx + 1u <= base + cnt;
        const uint32_t ps = hs ? (uint32_t)(rb + nth_bit(C, (int)(idx - base - 1u))) + 1u : 0u;
        const uint32_t pe = he ? (uint32_t)(rb + nth_bit(C, (int)(idx - base))) : 0u;
        const uint64_t ms = __ballot(hs), me = __ballot(he);
        if (ms) start = lane_get(ps, uniform32(__builtin_ctzll(ms)));
        if (me) end = lane_get(pe, uniform32(__builtin_ctzll(me)));
        nc += lane_last(incl);
        if (nc > idx) break;
    }
    if (start == kFieldNone) return false;
    off = start;
    len = (end == kFieldNone ? b : end) - start;
    return true;
}

}  // namespace vcfxg
