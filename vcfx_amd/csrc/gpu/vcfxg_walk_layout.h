// vcfxg_walk_layout.h -- which bytes of the data region each walker (wave) of k_af_walk owns.
// One function for the kernel, the host's plan (walk_plan) and the CPU test: no HIP headers.
//
// The dispatcher hands hardware block b to XCD x = b mod 8 in round k = b / 8.  In file order the
// blocks are x-major (walk_file_block: each XCD takes one contiguous run of the file, so the two
// walkers either side of a block boundary run on one XCD at about the same time).  The layout has
// two segments keyed on the round: blocks of rounds k < K1 hold walkers of C bytes, blocks of
// rounds k >= K1 walkers of Cs bytes (Cs <= C, both multiples of 16).  The short walkers are
// dispatched last, so the launch's drain is a short chunk's length; their bytes lie at the end
// of each XCD's run.  A block's first byte is
//     base[x] + waves * (min(k, K1) * C + max(k - K1, 0) * Cs),
// base[x] = lo + the bytes of XCDs 0 .. x - 1.  With K1 past the last round that is
// lo + file block * waves * C: walker wk owns [lo + wk * C, lo + (wk + 1) * C), the uniform layout.
#pragma once
#include <algorithm>
#include <cstdint>

#if defined(__HIPCC__)
#define VCFXG_LAYOUT_FN __host__ __device__ inline
#else
#define VCFXG_LAYOUT_FN inline
#endif

// blocks in x-major file order (1, the default) or in hardware order (0, for A/B)
#ifndef VCFXG_WALK_XCD
#define VCFXG_WALK_XCD 1
#endif

namespace vcfxg {

constexpr uint32_t kWalkXcds = 8;
constexpr uint32_t kWalkAllRounds = 0xFFFFFFFFu;  // K1 of the uniform layout

struct WalkLayout {
    int64_t base[kWalkXcds];  // first byte of each XCD's run (x-major order; [0] alone without it)
    int64_t C, Cs;            // a walker's bytes in rounds < K1 / >= K1
    int64_t nw;               // walkers that own bytes: the first nw in file order
    uint32_t K1, grid;        // first short round; blocks
};

// blocks of XCD x in a grid of n blocks
VCFXG_LAYOUT_FN uint32_t walk_xcd_blocks(uint32_t n, uint32_t x) { return n / kWalkXcds + (x < n % kWalkXcds ? 1u : 0u); }
// file-order index of hardware block b (x-major; bijective for any n)
VCFXG_LAYOUT_FN uint32_t walk_file_block(uint32_t b, uint32_t n) {
    const uint32_t q = n / kWalkXcds, r = n % kWalkXcds, x = b % kWalkXcds, k = b / kWalkXcds;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}
// bytes of the first `rounds` blocks of an XCD's run
VCFXG_LAYOUT_FN int64_t walk_run_bytes(const WalkLayout &l, uint32_t rounds, int waves) {
    const uint32_t full = rounds < l.K1 ? rounds : l.K1;
    return (int64_t)waves * ((int64_t)full * l.C + (int64_t)(rounds - full) * l.Cs);
}
// walker wv of hardware block b: its file-order index, its bytes [cs, ce) (clamped to hi; empty
// at the region's end) and its nominal size (C or Cs).  xcd = false: blocks in hardware order
VCFXG_LAYOUT_FN int64_t walk_range(const WalkLayout &l, uint32_t b, uint32_t n, int wv, int waves, int64_t hi, bool xcd,
                                   int64_t &cs, int64_t &ce, int64_t &size) {
    const uint32_t x = xcd ? b % kWalkXcds : 0u, k = xcd ? b / kWalkXcds : b;
    const uint32_t fb = xcd ? walk_file_block(b, n) : b;
    size = k < l.K1 ? l.C : l.Cs;
    cs = l.base[x] + walk_run_bytes(l, k, waves) + (int64_t)wv * size;
    if (cs > hi) cs = hi;
    ce = cs + size < hi ? cs + size : hi;
    return (int64_t)fb * waves + wv;
}

// The layout of [lo, hi) with walkers of C bytes in the first K1 rounds and Cs bytes after them:
// the smallest grid that covers the region (all of it full-size where 8 * K1 blocks already do),
// the XCD bases and the walkers that own bytes (only the last block's walkers can own none)
inline WalkLayout walk_layout_make(int64_t lo, int64_t hi, int64_t C, int64_t Cs, uint32_t K1, int waves, bool xcd) {
    WalkLayout l{};
    l.C = C;
    l.Cs = Cs;
    l.K1 = K1;
    const int64_t R = hi > lo ? hi - lo : 0, FB = (int64_t)waves * C, SB = (int64_t)waves * Cs;
    const int64_t nfull = (int64_t)K1 * kWalkXcds;  // (xcd = false: the rounds are the blocks)
    const int64_t fullcap = xcd ? nfull : (int64_t)K1;
    int64_t blocks;
    if (R <= 0) blocks = 0;
    else if ((R + FB - 1) / FB <= fullcap) blocks = (R + FB - 1) / FB;
    else blocks = fullcap + (R - fullcap * FB + SB - 1) / SB;
    l.grid = (uint32_t)blocks;
    int64_t at = lo;
    for (uint32_t x = 0; x < kWalkXcds; x++) {
        l.base[x] = at;
        at += walk_run_bytes(l, xcd ? walk_xcd_blocks(l.grid, x) : (x == 0 ? l.grid : 0u), waves);
    }
    l.nw = 0;
    if (blocks) {  // the last file-order block: the last hardware block of the last XCD that has one
        const uint32_t xl = !xcd ? 0u : l.grid < kWalkXcds ? l.grid - 1 : kWalkXcds - 1;
        const uint32_t kl = (xcd ? walk_xcd_blocks(l.grid, xl) : l.grid) - 1;
        const int64_t size = kl < K1 ? C : Cs, off = l.base[xl] + walk_run_bytes(l, kl, waves);
        int64_t own = (hi - off + size - 1) / size;
        if (own > waves) own = waves;
        l.nw = (blocks - 1) * waves + own;
    }
    return l;
}

// ---- the plan's choice (host)
// uniform: walkers of C0 bytes, as many as cover the region.
// fit:     with S walkers resident at a time, the walkers fill a whole number G of generations:
//          G = the uniform layout's walkers / S rounded down, C = C0 adjusted upward by the least
//          amount (to a multiple of 16 * div) that lets G * S walkers cover the region.  A region
//          under one generation stays uniform.
// taper:   fit, then the last g generations' worth of bytes go out in walkers of C / div bytes,
//          dispatched last (K1 = the rounds of the G - g full-size generations).
// split:   walkers of C0 bytes in rounds < K1, of C0 / div (rounded down to 16) after (tests)
enum : int { kLayoutDefault = 0, kLayoutUniform, kLayoutFit, kLayoutTaper, kLayoutSplit };
struct WalkLayoutKnob {
    int kind = kLayoutDefault;
    int div = 1;   // taper / split: C / Cs
    int64_t g = 0;  // taper: short generations; split: K1
};

inline WalkLayoutKnob parse_walk_layout(const char *e) {
    WalkLayoutKnob k;
    if (!e) return k;
    auto is = [&](const char *w) {
        size_t i = 0;
        while (w[i] && e[i] == w[i]) i++;
        return !w[i] && (!e[i] || e[i] == ':');
    };
    auto nums = [&](int64_t &a, int64_t &b) {  // ":<a>:<b>", both decimal
        const char *p = e;
        while (*p && *p != ':') p++;
        int64_t v[2] = {-1, -1};
        for (int i = 0; i < 2 && *p == ':'; i++) {
            p++;
            if (*p < '0' || *p > '9') return false;
            v[i] = 0;
            while (*p >= '0' && *p <= '9' && v[i] < (1ll << 40)) v[i] = v[i] * 10 + (*p++ - '0');
        }
        a = v[0];
        b = v[1];
        return !*p && a >= 0 && b >= 0;
    };
    int64_t a = 0, b = 0;
    if (is("uniform") && !e[7]) k.kind = kLayoutUniform;
    else if (is("fit") && !e[3]) k.kind = kLayoutFit;
    else if ((is("taper") || is("split")) && nums(a, b) && a >= 1 && a <= 64 && b <= 0x7FFFFFFF) {
        k.kind = is("taper") ? kLayoutTaper : kLayoutSplit;
        k.div = (int)a;
        k.g = b;
    }
    return k;
}

// the layout of [lo, hi) for `knob` (kLayoutDefault is the caller's to resolve) with S walkers
// resident; *kind: what it came to (a fit or taper that does not apply reports kLayoutUniform)
inline WalkLayout walk_layout_plan(int64_t lo, int64_t hi, int64_t C0, int64_t S, WalkLayoutKnob knob, int waves,
                                   bool xcd, int *kind = nullptr) {
    const int64_t R = hi > lo ? hi - lo : 0;
    int got = kLayoutUniform;
    WalkLayout l = walk_layout_make(lo, hi, C0, C0, kWalkAllRounds, waves, xcd);
    if (knob.kind == kLayoutSplit) {
        const int64_t Cs = std::max<int64_t>(C0 / knob.div & ~(int64_t)15, 16);
        l = walk_layout_make(lo, hi, C0, Cs, (uint32_t)knob.g, waves, xcd);
        got = kLayoutSplit;
    } else if ((knob.kind == kLayoutFit || knob.kind == kLayoutTaper) && S >= waves && R > 0) {
        const int64_t G = l.nw / S;
        if (G >= 1) {
            const int64_t div = knob.kind == kLayoutTaper ? knob.div : 1, unit = 16 * div;
            int64_t C = (R + G * S - 1) / (G * S);
            C = (std::max(C, C0) + unit - 1) / unit * unit;
            const int64_t g = knob.kind == kLayoutTaper ? std::min<int64_t>(knob.g, G) : 0;
            if (g > 0 && div > 1) {
                const int64_t rounds = (G - g) * (S / waves) / (xcd ? (int64_t)kWalkXcds : 1);
                l = walk_layout_make(lo, hi, C, C / div, (uint32_t)std::min<int64_t>(rounds, kWalkAllRounds - 1), waves, xcd);
                got = kLayoutTaper;
            } else {
                l = walk_layout_make(lo, hi, C, C, kWalkAllRounds, waves, xcd);
                got = kLayoutFit;
            }
        }
    }
    if (kind) *kind = got;
    return l;
}

}  // namespace vcfxg
