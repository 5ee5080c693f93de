// vcfxg_df.hip -- VCFX_diff_tool (VCFX_diff_tool.cpp: parseVariantLine :214-264, generateVariantKey
// :168-200, compareChromNatural :269-307, compareKeys :312-328, diffInMemoryMmap :333-404,
// diffStreamingMmap :409-506): the variant keys of two files, and which of them the other file
// lacks.  Both files are one indexed text: file 1's lines, then (from line `cut` on) file 2's.
//
// The passes (the scans and the radix sort between them are hipcub's, vcfxg_api_df.hip):
//   k_df_key     a lane per line over its first kDfWindow bytes: the first five tabs from 16 B
//                loads, then the status, POS (digits only; its value for the sorted mode), ALT's
//                token count, the key's length and CHROM's natural-order parts.  A line whose fifth
//                tab is not inside the window (and that is longer than it) is queued for
//                k_df_key_wave, a wave per line (head_tabs), so a field of any length passes.
//   k_df_text    every data line's key CHROM:POS:REF:ALT' written once at its offset (the scan of
//                the lengths), with the key's hash: a lane per key of up to kDfLaneKey bytes and up
//                to kDfLaneTok ALT tokens, k_df_text_wave for every other key.  ALT' = ALT's tokens
//                in byte order (a prefix before its extensions), joined with ','.  One token is
//                copied; otherwise each token's place is COUNTED: the bytes of the tokens that sort
//                before it (an equal token: that start before it), exact for any count, quadratic
//                in the count.  Only typical counts (one to a few tokens) need to be fast: a lane
//                does them; the wave path gives a token to each lane (200 tokens: four rounds).
//   default mode (diffInMemoryMmap: two sets of key strings): (hash, line) of the data lines sorted
//                stably; k_df_verify compares every element exactly with the head of its run,
//                k_df_resolve settles the ones that differ in line order against the run's class
//                heads (dedup's discipline: the result does not depend on the hash); rep[j] = the
//                first element with j's key.  Inside a run the lines ascend, so a class's file-1
//                lines come first: k_df_first2 finds each class's first file-2 element, k_df_decide
//                gives every line its status: a repeat, or the first of its file with (common) or
//                without (unique) the key in the other file.  Each side's output is in line order,
//                that is IN INPUT ORDER OF THE KEY'S FIRST LINE in its file; the reference prints
//                each side in the iteration order of its C++ library's unordered_set (the one
//                documented difference, DESIGN.md "Diff").
//   sorted mode  (diffStreamingMmap: a two-pointer walk) df_cmp is compareKeys over the descriptors
//                of two lines.  k_df_ordered: is every data line <= the next one of its file?  If
//                so the walk is a multiset difference and k_df_bounds decides each line from three
//                binary searches: it is reported when its occurrence number among its file's equal
//                lines is at least the other file's count of equal lines.  If not, k_df_walk is
//                the loop itself, one lane of one wave, a bounded number of steps a launch with the
//                two pointers kept in device memory; k_df_drain reports what it left.  That is the
//                slow path of inputs that break the tool's own contract.
//   k_df_flag / k_df_place  the unique lines' key text spans, in line order, for the gather (vcfxg_gather.hip).
//
// The hash: sum over the key's bytes of mix((i << 8 | byte) + c0), i the byte's place in the key,
// then mix(sum ^ (length * c1 + c2)); a sum, so any lane may add any byte.  mix = splitmix64's
// finaliser (mix64, hash_byte, hash_field: vcfxg_keyed.h, with the tab scan window_tabs and the byte
// order cmp_bytes).
#include "vcfxg_keyed.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kDfThreads = 256;
constexpr int kDfWaves = kDfThreads / kWave;
constexpr uint64_t kDfLaneKey = 96;  // key bytes and ALT tokens a lane writes; more: a wave
constexpr uint32_t kDfLaneTok = 4;
constexpr uint32_t kDfPending = 0xFFFFFFFFu;

// ---- the key pass ------------------------------------------------------------------------------

struct DfLine {
    uint64_t t0, t1, t2, t3, t4, klen, nsuf;
    int64_t posv, natv;
    uint32_t ntok;
    uint8_t st;
};

// compareChromNatural's view of the CHROM [cs, ce) (:271-290): a prefix of exactly chr / Chr / CHR
// dropped, then the decimal digit prefix: its value (-1: none) and where the rest begins
__device__ __forceinline__ void df_natural(const char *__restrict__ buf, int64_t cs, int64_t ce, int64_t &val, uint64_t &suf) {
    int64_t p = cs;
    if (ce - cs >= 3) {
        const uint32_t c0 = byte_at(buf, cs), c1 = byte_at(buf, cs + 1), c2 = byte_at(buf, cs + 2);
        if ((c0 == 'c' && c1 == 'h' && c2 == 'r') || (c0 == 'C' && c1 == 'h' && c2 == 'r') || (c0 == 'C' && c1 == 'H' && c2 == 'R'))
            p += 3;
    }
    uint64_t v = 0;
    int64_t q = p;
    uint32_t d;
    while (q < ce && (d = byte_at(buf, q) - '0') <= 9u) {
        v = v * 10u + d;
        q++;
    }
    val = q > p ? (int64_t)v : -1;
    suf = (uint64_t)q;
}

// the line's end as parseVariantLine sees it: without one trailing '\r' (le > ls)
__device__ __forceinline__ int64_t df_line_end(const char *__restrict__ buf, int64_t le) {
    return byte_at(buf, le - 1) == '\r' ? le - 1 : le;
}

__device__ __forceinline__ void df_lengths(int64_t ls, int natural, const char *__restrict__ buf, DfLine &o) {
    o.klen = (o.t0 - (uint64_t)ls) + (o.t1 - o.t0 - 1u) + (o.t3 - o.t2 - 1u) + (o.t4 - o.t3 - 1u) + 3u;
    if (natural) df_natural(buf, ls, (int64_t)o.t0, o.natv, o.nsuf);
    o.st = kDfData;
}

// The lane's line [ls, le) (not empty, not '#') over its first kDfWindow bytes; false: the wave takes it.
__device__ __forceinline__ bool df_lane_line(const DfLines &D, int natural, int64_t ls, int64_t le, DfLine &o) {
    const char *__restrict__ buf = D.buf;
    int64_t t[5] = {0, 0, 0, 0, 0};
    const int nt = window_tabs<5>(buf, ls, le, kDfWindow, t);
    if (nt < 5 && le - ls > kDfWindow) return false;  // the window ended before the key fields did
    o.t0 = (uint64_t)t[0], o.t1 = (uint64_t)t[1], o.t2 = (uint64_t)t[2], o.t3 = (uint64_t)t[3], o.t4 = (uint64_t)t[4];
    o.st = kDfSkipped;
    if (nt < 4) return true;  // CHROM, POS, ID and REF each end at a tab (:222-251)
    if (nt == 4) o.t4 = (uint64_t)df_line_end(buf, le);
    uint64_t v = 0;
    for (int64_t p = (int64_t)o.t0 + 1; p < (int64_t)o.t1; p++) {
        const uint32_t d = byte_at(buf, p) - '0';
        if (d > 9u) return true;  // a POS byte outside 0-9 (:235-238)
        v = v * 10u + d;
    }
    o.posv = (int64_t)v;
    uint32_t commas = 0;
    for (int64_t p = (int64_t)o.t3 + 1; p < (int64_t)o.t4; p++) commas += byte_at(buf, p) == ',' ? 1u : 0u;
    o.ntok = commas + 1u;
    df_lengths(ls, natural, buf, o);
    return true;
}

// The wave's line [ls, le) (uniform; every lane active): any width.
__device__ __forceinline__ void df_wave_line(const DfLines &D, int natural, int64_t ls, int64_t le, int64_t *lds, DfLine &o) {
    const char *__restrict__ buf = D.buf;
    int64_t t[5] = {0, 0, 0, 0, 0};
    const int nt = head_tabs(buf, ls, le, 5, t, lds);
    o.st = kDfSkipped;
    if (nt < 4) return;
    o.t0 = (uint64_t)t[0], o.t1 = (uint64_t)t[1], o.t2 = (uint64_t)t[2], o.t3 = (uint64_t)t[3];
    o.t4 = (uint64_t)(nt == 5 ? t[4] : uniform64(df_line_end(buf, le)));
    bool bad = false;
    for (int64_t p = t[0] + 1 + lane(); p < t[1]; p += kWave) bad = bad || byte_at(buf, p) - '0' > 9u;
    if (__ballot(bad) != 0ull) return;
    // (more than 18 digits: outside the sorted mode's domain, and no other mode reads the value)
    uint64_t v = 0;
    for (int64_t p = t[0] + 1; p < t[1] && p < t[0] + 20; p++) v = v * 10u + (byte_at(buf, p) - '0');
    o.posv = (int64_t)v;
    uint32_t commas = 0;
    for (int64_t p = t[3] + 1 + lane(); p < (int64_t)o.t4; p += kWave) commas += byte_at(buf, p) == ',' ? 1u : 0u;
    o.ntok = wave_sum32(commas) + 1u;
    df_lengths(ls, natural, buf, o);
}

__device__ __forceinline__ void df_store(const DfLines &D, uint64_t li, const DfLine &o) {
    D.status[li] = o.st;
    D.isdata[li] = o.st == kDfData ? 1u : 0u;
    D.klen[li] = o.st == kDfData ? o.klen : 0u;
    if (o.st == kDfData) {
        uint64_t *t = D.tabs + 5 * li;
        t[0] = o.t0, t[1] = o.t1, t[2] = o.t2, t[3] = o.t3, t[4] = o.t4;
        D.ntok[li] = o.ntok;
        D.posv[li] = o.posv;
        D.natv[li] = o.natv;
        D.nsuf[li] = o.nsuf;
    }
}

__device__ __forceinline__ void df_clear(DfLine &o) {
    o.t0 = o.t1 = o.t2 = o.t3 = o.t4 = o.klen = o.nsuf = 0;
    o.posv = 0;
    o.natv = -1;
    o.ntok = 0;
    o.st = kDfEmpty;
}

// counters[7] = the first line that starts at or after second_start (L: none)
__global__ void k_df_cut(const uint64_t *__restrict__ line_end, int64_t data_start, uint64_t L, uint64_t second_start,
                         unsigned long long *__restrict__ counters) {
    if (threadIdx.x || blockIdx.x) return;
    uint64_t lo = 0, hi = L;  // line li starts at line_end[li - 1] + 1: non-decreasing
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const uint64_t start = (uint64_t)line_start(line_end, data_start, mid);
        if (start >= second_start) hi = mid;
        else lo = mid + 1;
    }
    counters[7] = lo;
}

// The lane pass; a line it does not settle goes to queue[counters[5]++] for k_df_key_wave.
__global__ __launch_bounds__(kDfThreads) void k_df_key(DfLines D, int natural, uint32_t *__restrict__ queue,
                                                       unsigned long long *__restrict__ counters) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < D.L; li += nth) {
        const int64_t ls = line_start(D.line_end, D.data_start, li), le = (int64_t)D.line_end[li];
        DfLine o;
        df_clear(o);
        bool have = true;
        if (le > ls) {
            if (byte_at(D.buf, ls) == '#') o.st = kDfHeader;
            else have = df_lane_line(D, natural, ls, le, o);
        }
        if (have) {
            df_store(D, li, o);
            if (o.st == kDfSkipped) atomicAdd(&counters[4], 1ull);
        } else {
            queue[atomicAdd(&counters[5], 1ull)] = (uint32_t)li;
        }
    }
}

// The wave pass over the queued lines (counters[5] of them), a wave per line.
__global__ __launch_bounds__(kDfThreads) void k_df_key_wave(DfLines D, int natural, const uint32_t *__restrict__ queue,
                                                            unsigned long long *__restrict__ counters) {
    __shared__ int64_t s_tabs[kDfWaves][10];
    const uint64_t nq = counters[5];
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t q = wid; q < nq; q += nw) {
        const uint64_t li = (uint64_t)uniform32((int)queue[q]);
        const int64_t ls = uniform64(line_start(D.line_end, D.data_start, li)), le = uniform64((int64_t)D.line_end[li]);
        DfLine o;
        df_clear(o);
        df_wave_line(D, natural, ls, le, s_tabs[threadIdx.x / kWave], o);
        if (lane() == 0) {
            df_store(D, li, o);
            if (o.st == kDfSkipped) atomicAdd(&counters[4], 1ull);
        }
    }
}

// ---- the key text ------------------------------------------------------------------------------

// where the token [ts, te) of the ALT field [s, e) stands in ALT': the bytes (each with its ',') of
// the tokens that sort before it, an equal token when it starts earlier
__device__ __forceinline__ uint64_t df_token_place(const char *__restrict__ buf, int64_t s, int64_t e, int64_t ts, int64_t te) {
    uint64_t off = 0;
    int64_t a = s;
    for (int64_t p = s; p <= e; p++)
        if (p == e || byte_at(buf, p) == ',') {
            const int c = cmp_bytes(buf, a, p - a, ts, te - ts);
            if (c < 0 || (c == 0 && a < ts)) off += (uint64_t)(p - a) + 1u;
            a = p + 1;
        }
    return off;
}

// the token that starts at ts written to its place in ALT' (out: ALT's first key byte, key byte
// index k0); returns the hash sum of what it wrote
__device__ __forceinline__ uint64_t df_put_token(const char *__restrict__ buf, int64_t s, int64_t e, int64_t ts, char *out,
                                                 uint64_t k0) {
    int64_t te = ts;
    while (te < e && byte_at(buf, te) != ',') te++;
    const uint64_t off = df_token_place(buf, s, e, ts, te);
    uint64_t sum = 0;
    for (int64_t i = 0; i < te - ts; i++) {
        const uint32_t b = byte_at(buf, ts + i);
        out[off + (uint64_t)i] = (char)b;
        sum += hash_byte(b, k0 + off + (uint64_t)i);
    }
    const uint64_t end = off + (uint64_t)(te - ts);
    if (end < (uint64_t)(e - s)) {  // (not ALT''s last token)
        out[end] = ',';
        sum += hash_byte(',', k0 + end);
    }
    return sum;
}

// [s, e) copied to out[k ..] by one lane, then the separator (0: none)
__device__ __forceinline__ void df_lane_copy(const char *__restrict__ buf, int64_t s, int64_t e, uint32_t sep, char *out,
                                             uint64_t &k, uint64_t &sum) {
    for (int64_t p = s; p < e; p++) {
        const uint32_t b = byte_at(buf, p);
        out[k] = (char)b;
        sum += hash_byte(b, k++);
    }
    if (sep) {
        out[k] = (char)sep;
        sum += hash_byte(sep, k++);
    }
}

// the same by the whole wave (k uniform)
__device__ __forceinline__ void df_wave_copy(const char *__restrict__ buf, int64_t s, int64_t e, uint32_t sep, char *out,
                                             uint64_t &k, uint64_t &sum) {
    for (int64_t p = s + lane(); p < e; p += kWave) {
        const uint32_t b = byte_at(buf, p);
        out[k + (uint64_t)(p - s)] = (char)b;
        sum += hash_byte(b, k + (uint64_t)(p - s));
    }
    k += (uint64_t)(e - s);
    if (sep) {
        if (lane() == 0) {
            out[k] = (char)sep;
            sum += hash_byte(sep, k);
        }
        k++;
    }
}

// The lane pass over the data lines; a longer key or more tokens: queue[counters[9]++].
__global__ __launch_bounds__(kDfThreads) void k_df_text(DfLines D, const uint64_t *__restrict__ ord,
                                                        const uint64_t *__restrict__ koff, char *__restrict__ ktext,
                                                        uint64_t *__restrict__ hash, uint32_t *__restrict__ line,
                                                        uint32_t *__restrict__ queue, unsigned long long *__restrict__ counters) {
    const char *__restrict__ buf = D.buf;
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li < D.L; li += nth) {
        if (!D.isdata[li]) continue;
        line[ord[li]] = (uint32_t)li;
        const uint64_t klen = D.klen[li];
        const uint32_t ntok = D.ntok[li];
        if (klen > kDfLaneKey || ntok > kDfLaneTok) {
            queue[atomicAdd(&counters[9], 1ull)] = (uint32_t)li;
            continue;
        }
        const uint64_t *t = D.tabs + 5 * li;
        const int64_t ls = line_start(D.line_end, D.data_start, li), s = (int64_t)t[3] + 1, e = (int64_t)t[4];
        char *out = ktext + koff[li];
        uint64_t k = 0, sum = 0;
        df_lane_copy(buf, ls, (int64_t)t[0], ':', out, k, sum);
        df_lane_copy(buf, (int64_t)t[0] + 1, (int64_t)t[1], ':', out, k, sum);
        df_lane_copy(buf, (int64_t)t[2] + 1, (int64_t)t[3], ':', out, k, sum);
        if (ntok == 1) {
            df_lane_copy(buf, s, e, 0, out, k, sum);
        } else {
            for (int64_t p = s; p <= e; p++)
                if (p == s || byte_at(buf, p - 1) == ',') sum += df_put_token(buf, s, e, p, out + k, k);
        }
        hash[li] = hash_field(sum, klen);
    }
}

// The wave pass over the queued keys (counters[9] of them): the fields lane-strided, a token per lane.
__global__ __launch_bounds__(kDfThreads) void k_df_text_wave(DfLines D, const uint64_t *__restrict__ koff,
                                                             char *__restrict__ ktext, uint64_t *__restrict__ hash,
                                                             const uint32_t *__restrict__ queue,
                                                             const unsigned long long *__restrict__ counters) {
    const char *__restrict__ buf = D.buf;
    const uint64_t nq = counters[9];
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t q = wid; q < nq; q += nw) {
        const uint64_t li = (uint64_t)uniform32((int)queue[q]);
        const uint64_t *t = D.tabs + 5 * li;
        const int64_t ls = uniform64(line_start(D.line_end, D.data_start, li)), t0 = uniform64((int64_t)t[0]), t1 = uniform64((int64_t)t[1]),
                      t2 = uniform64((int64_t)t[2]), t3 = uniform64((int64_t)t[3]), e = uniform64((int64_t)t[4]);
        const int64_t s = t3 + 1;
        char *out = ktext + (uint64_t)uniform64((int64_t)koff[li]);
        uint64_t k = 0, sum = 0;
        df_wave_copy(buf, ls, t0, ':', out, k, sum);
        df_wave_copy(buf, t0 + 1, t1, ':', out, k, sum);
        df_wave_copy(buf, t2 + 1, t3, ':', out, k, sum);
        if (uniform32((int)D.ntok[li]) == 1) {
            df_wave_copy(buf, s, e, 0, out, k, sum);
        } else {
            // a token starts at s and after every comma (so possibly at e: an empty last token)
            for (int64_t w = s; w <= e; w += kWave) {
                const int64_t p = w + lane();
                if (p <= e && (p == s || byte_at(buf, p - 1) == ',')) sum += df_put_token(buf, s, e, p, out + k, k);
            }
        }
        const uint64_t total = (uint64_t)wave_sum<unsigned long long>((unsigned long long)sum);
        if (lane() == 0) hash[li] = hash_field(total, D.klen[li]);
    }
}

// ---- default mode: classes of equal key text ---------------------------------------------------

// (hash masked, line) of data line j
__global__ __launch_bounds__(kDfThreads) void k_df_pairs(uint64_t nd, const uint32_t *__restrict__ line,
                                                         const uint64_t *__restrict__ hash, uint64_t mask,
                                                         uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= nd) return;
    keys[j] = hash[line[j]] & mask;
    vals[j] = line[j];
}

struct DfKeys {
    const char *ktext;
    const uint64_t *koff, *klen;
};

__device__ __forceinline__ bool df_equal(const DfKeys &K, uint32_t x, uint32_t y) {
    const uint64_t n = K.klen[x];
    if (n != K.klen[y]) return false;
    const char *a = K.ktext + K.koff[x], *b = K.ktext + K.koff[y];
    for (uint64_t i = 0; i < n; i++)
        if (a[i] != b[i]) return false;
    return true;
}

__device__ __forceinline__ uint32_t df_rep_load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a head is its own class; another element equal to its head joins it, else it is pending
// (left[head] = 1, counters[6] counts them)
__global__ __launch_bounds__(kDfThreads) void k_df_verify(DfKeys K, uint64_t nd, const uint32_t *__restrict__ vals,
                                                          const uint32_t *__restrict__ head, uint32_t *__restrict__ rep,
                                                          uint32_t *__restrict__ first2, uint8_t *__restrict__ left,
                                                          unsigned long long *__restrict__ counters) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= nd) return;
    first2[j] = kDfPending;
    const uint32_t h = head[j];
    if (h == j || df_equal(K, vals[j], vals[h])) {
        rep[j] = h;
    } else {
        rep[j] = kDfPending;
        left[h] = 1;
        atomicAdd(&counters[6], 1ull);
    }
}

// A wave per run that has pending elements: in line order each one against the run's class heads
// so far (the run's head excepted: it differs), 64 candidates a step.
__global__ __launch_bounds__(kDfThreads) void k_df_resolve(DfKeys K, uint64_t nd, const uint64_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ vals, const uint8_t *__restrict__ left,
                                                           uint32_t *rep, const unsigned long long *__restrict__ counters) {
    if (counters[6] == 0) return;
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t h = wid; h < nd; h += nw) {
        if (!left[h]) continue;
        const uint64_t key = keys[h];
        for (uint64_t e = h + 1; e < nd && keys[e] == key; e++) {
            if (df_rep_load(rep + e) != kDfPending) continue;
            const uint32_t le = vals[e + (uint64_t)(lane() >> 6)];  // (per lane, as k_dd_resolve)
            uint32_t found = (uint32_t)e;
            for (uint64_t base = h + 1; base < e && found == (uint32_t)e; base += kWave) {
                const uint64_t c = base + (uint64_t)lane();
                const bool hit = c < e && df_rep_load(rep + c) == (uint32_t)c && df_equal(K, le, vals[c]);
                const uint64_t m = __ballot(hit);
                if (m) found = (uint32_t)(base + (uint64_t)__builtin_ctzll(m));
            }
            if (lane() == 0) __hip_atomic_store(rep + e, found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
}

// first2[class] = its first element that is a line of file 2
__global__ __launch_bounds__(kDfThreads) void k_df_first2(uint64_t nd, const uint32_t *__restrict__ vals,
                                                          const uint32_t *__restrict__ rep, uint32_t *__restrict__ first2,
                                                          const unsigned long long *__restrict__ counters) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= nd) return;
    const uint32_t r = rep[j];
    if (r < nd && vals[j] >= counters[7]) atomicMin(&first2[r], (uint32_t)j);
}

__global__ __launch_bounds__(kDfThreads) void k_df_decide(uint64_t nd, const uint32_t *__restrict__ vals,
                                                          const uint32_t *__restrict__ rep, const uint32_t *__restrict__ first2,
                                                          uint8_t *__restrict__ status,
                                                          const unsigned long long *__restrict__ counters) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= nd) return;
    const uint64_t cut = counters[7];
    const uint32_t r = rep[j];
    if (r >= nd) return;  // (never: every element has its class by now)
    const uint32_t f2 = first2[r];
    uint8_t st;
    if (vals[j] < cut) st = j != r ? kDfRepeat : f2 == kDfPending ? kDfUnique : kDfCommon;
    else st = j != f2 ? kDfRepeat : vals[r] < cut ? kDfCommon : kDfUnique;
    status[vals[j]] = st;
}

// ---- sorted mode -------------------------------------------------------------------------------

// compareKeys (:312-328) of lines x and y: CHROM (bytes, or compareChromNatural), POS as an
// integer, REF bytes, the raw ALT bytes
__device__ __forceinline__ int df_cmp(const DfLines &D, int natural, uint32_t x, uint32_t y) {
    const char *__restrict__ buf = D.buf;
    const uint64_t *tx = D.tabs + 5 * (uint64_t)x, *ty = D.tabs + 5 * (uint64_t)y;
    int c;
    if (natural) {
        const int64_t nx = D.natv[x], ny = D.natv[y];
        if (nx >= 0 && ny >= 0) {
            if (nx != ny) return nx < ny ? -1 : 1;
        } else if (nx >= 0) {
            return -1;
        } else if (ny >= 0) {
            return 1;
        }
        const int64_t sx = (int64_t)D.nsuf[x], sy = (int64_t)D.nsuf[y];
        c = cmp_bytes(buf, sx, (int64_t)tx[0] - sx, sy, (int64_t)ty[0] - sy);
    } else {
        const int64_t xs = line_start(D.line_end, D.data_start, x), ys = line_start(D.line_end, D.data_start, y);
        c = cmp_bytes(buf, xs, (int64_t)tx[0] - xs, ys, (int64_t)ty[0] - ys);
    }
    if (c) return c;
    const int64_t px = D.posv[x], py = D.posv[y];
    if (px != py) return px < py ? -1 : 1;
    c = cmp_bytes(buf, (int64_t)tx[2] + 1, (int64_t)(tx[3] - tx[2]) - 1, (int64_t)ty[2] + 1, (int64_t)(ty[3] - ty[2]) - 1);
    if (c) return c;
    return cmp_bytes(buf, (int64_t)tx[3] + 1, (int64_t)(tx[4] - tx[3]) - 1, (int64_t)ty[3] + 1, (int64_t)(ty[4] - ty[3]) - 1);
}

// counters[8] = 1 when a data line compares greater than the next data line of its file
__global__ __launch_bounds__(kDfThreads) void k_df_ordered(DfLines D, int natural, const uint32_t *__restrict__ line, uint64_t n1,
                                                           uint64_t nd, unsigned long long *__restrict__ counters) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j + 1 >= nd || j + 1 == n1) return;
    if (df_cmp(D, natural, line[j], line[j + 1]) > 0) counters[8] = 1ull;
}

// the first j in [lo, hi) whose line is not less than (upper: is greater than) line x
__device__ __forceinline__ uint64_t df_bound(const DfLines &D, int natural, const uint32_t *__restrict__ line, uint64_t lo,
                                             uint64_t hi, uint32_t x, bool upper) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const int c = df_cmp(D, natural, line[mid], x);
        if (upper ? c <= 0 : c < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Both files non-decreasing: a line is reported when its occurrence number among its file's equal
// lines is at least the other file's count of equal lines.
__global__ __launch_bounds__(kDfThreads) void k_df_bounds(DfLines D, int natural, const uint32_t *__restrict__ line, uint64_t n1,
                                                          uint64_t nd) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= nd) return;
    const uint32_t x = line[j];
    const bool second = j >= n1;
    const uint64_t own_lo = second ? n1 : 0, oth_lo = second ? 0 : n1, oth_hi = second ? n1 : nd;
    const uint64_t lb = df_bound(D, natural, line, oth_lo, oth_hi, x, false);
    const uint64_t ub = df_bound(D, natural, line, lb, oth_hi, x, true);
    const uint64_t occ = j - df_bound(D, natural, line, own_lo, j, x, false);
    D.status[x] = occ >= ub - lb ? kDfUnique : kDfCommon;
}

// The two-pointer loop (:461-477) from state[0..1], at most `steps` steps: one lane of one wave.
__global__ __launch_bounds__(kWave) void k_df_walk(DfLines D, int natural, const uint32_t *__restrict__ line, uint64_t n1,
                                                   uint64_t nd, uint64_t steps, uint64_t *__restrict__ state) {
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t n2 = nd - n1;
    uint64_t p1 = state[0], p2 = state[1];
    for (uint64_t s = 0; s < steps && p1 < n1 && p2 < n2; s++) {
        const uint32_t a = line[p1], b = line[n1 + p2];
        const int c = df_cmp(D, natural, a, b);
        if (c < 0) {
            D.status[a] = kDfUnique;
            p1++;
        } else if (c > 0) {
            D.status[b] = kDfUnique;
            p2++;
        } else {
            D.status[a] = kDfCommon;
            D.status[b] = kDfCommon;
            p1++;
            p2++;
        }
    }
    state[0] = p1;
    state[1] = p2;
}

// what the loop left (:480-487)
__global__ __launch_bounds__(kDfThreads) void k_df_drain(const uint32_t *__restrict__ line, uint64_t n1, uint64_t nd,
                                                         const uint64_t *__restrict__ state, uint8_t *__restrict__ status) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= nd) return;
    if (j < n1 ? j >= state[0] : j - n1 >= state[1]) status[line[j]] = kDfUnique;
}

// ---- the unique lines --------------------------------------------------------------------------

__global__ __launch_bounds__(kDfThreads) void k_df_flag(uint64_t L, const uint8_t *__restrict__ status, uint32_t *__restrict__ uflag) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li <= L; li += nth)
        uflag[li] = li < L && status[li] == kDfUnique ? 1u : 0u;
}

__global__ __launch_bounds__(kDfThreads) void k_df_place(uint64_t L, const uint32_t *__restrict__ uflag,
                                                         const uint64_t *__restrict__ uord, const uint64_t *__restrict__ koff,
                                                         const uint64_t *__restrict__ klen, uint64_t *__restrict__ len,
                                                         uint64_t *__restrict__ src) {
    const uint64_t nth = gridDim.x * (uint64_t)blockDim.x;
    for (uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; li <= L; li += nth) {
        if (li == L) {
            len[uord[L]] = 0;
        } else if (uflag[li]) {
            len[uord[li]] = klen[li] + 1u;
            src[uord[li]] = koff[li];
        }
    }
}

// unique lines per file, data lines per file, skipped lines, wave-path lines, (the path), the cut
__global__ void k_df_sum(uint64_t L, const uint64_t *__restrict__ ord, const uint64_t *__restrict__ uord,
                         const unsigned long long *__restrict__ counters, uint64_t *__restrict__ sum) {
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t cut = counters[7];
    sum[0] = uord[cut];
    sum[1] = uord[L] - uord[cut];
    sum[2] = ord[cut];
    sum[3] = ord[L] - ord[cut];
    sum[4] = counters[4];
    sum[5] = counters[5];
    sum[6] = 0;
    sum[7] = cut;
}

// ---- launchers ---------------------------------------------------------------------------------

hipError_t launch_df_cut(const uint64_t *line_end, int64_t data_start, uint64_t L, uint64_t second_start,
                         unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_df_cut, dim3(1), dim3(kWave), 0, s, line_end, data_start, L, second_start, counters);
    return hipGetLastError();
}

hipError_t launch_df_key(const DfLines &D, int natural, uint32_t *queue, unsigned long long *counters, hipStream_t s) {
    if (!D.L) return hipSuccess;
    hipLaunchKernelGGL(k_df_key, dim3(grid_for(D.L, kDfThreads, 8192)), dim3(kDfThreads), 0, s, D, natural, queue, counters);
    hipLaunchKernelGGL(k_df_key_wave, dim3(grid_for(D.L, kDfWaves, 2048)), dim3(kDfThreads), 0, s, D, natural, queue, counters);
    return hipGetLastError();
}

hipError_t launch_df_text(const DfLines &D, const uint64_t *ord, const uint64_t *koff, char *ktext, uint64_t *hash,
                          uint32_t *line, uint32_t *queue, unsigned long long *counters, hipStream_t s) {
    if (!D.L) return hipSuccess;
    hipLaunchKernelGGL(k_df_text, dim3(grid_for(D.L, kDfThreads, 8192)), dim3(kDfThreads), 0, s, D, ord, koff, ktext, hash, line,
                       queue, counters);
    hipLaunchKernelGGL(k_df_text_wave, dim3(grid_for(D.L, kDfWaves, 2048)), dim3(kDfThreads), 0, s, D, koff, ktext, hash, queue,
                       counters);
    return hipGetLastError();
}

hipError_t launch_df_pairs(uint64_t nd, const uint32_t *line, const uint64_t *hash, uint32_t hash_bits, uint64_t *keys,
                           uint32_t *vals, hipStream_t s) {
    if (!nd) return hipSuccess;
    const uint64_t mask = hash_bits && hash_bits < 64u ? (1ull << hash_bits) - 1u : ~0ull;
    hipLaunchKernelGGL(k_df_pairs, flat_grid(nd, kDfThreads), dim3(kDfThreads), 0, s, nd, line, hash, mask, keys, vals);
    return hipGetLastError();
}

hipError_t launch_df_classes(const char *ktext, const uint64_t *koff, const uint64_t *klen, uint64_t nd, const uint64_t *keys,
                             const uint32_t *vals, const uint32_t *head, uint32_t *rep, uint32_t *first2, uint8_t *left,
                             uint8_t *status, unsigned long long *counters, hipStream_t s) {
    if (!nd) return hipSuccess;
    const DfKeys K{ktext, koff, klen};
    hipLaunchKernelGGL(k_df_verify, flat_grid(nd, kDfThreads), dim3(kDfThreads), 0, s, K, nd, vals, head, rep, first2, left, counters);
    hipLaunchKernelGGL(k_df_resolve, dim3(grid_for(nd, kDfWaves, 2048)), dim3(kDfThreads), 0, s, K, nd, keys, vals, left, rep,
                       counters);
    hipLaunchKernelGGL(k_df_first2, flat_grid(nd, kDfThreads), dim3(kDfThreads), 0, s, nd, vals, rep, first2, counters);
    hipLaunchKernelGGL(k_df_decide, flat_grid(nd, kDfThreads), dim3(kDfThreads), 0, s, nd, vals, rep, first2, status, counters);
    return hipGetLastError();
}

hipError_t launch_df_ordered(const DfLines &D, int natural, const uint32_t *line, uint64_t n1, uint64_t nd,
                             unsigned long long *counters, hipStream_t s) {
    if (nd < 2) return hipSuccess;
    hipLaunchKernelGGL(k_df_ordered, flat_grid(nd, kDfThreads), dim3(kDfThreads), 0, s, D, natural, line, n1, nd, counters);
    return hipGetLastError();
}

hipError_t launch_df_bounds(const DfLines &D, int natural, const uint32_t *line, uint64_t n1, uint64_t nd, hipStream_t s) {
    if (!nd) return hipSuccess;
    hipLaunchKernelGGL(k_df_bounds, flat_grid(nd, kDfThreads), dim3(kDfThreads), 0, s, D, natural, line, n1, nd);
    return hipGetLastError();
}

hipError_t launch_df_walk(const DfLines &D, int natural, const uint32_t *line, uint64_t n1, uint64_t nd, uint64_t steps,
                          uint64_t *state, hipStream_t s) {
    hipLaunchKernelGGL(k_df_walk, dim3(1), dim3(kWave), 0, s, D, natural, line, n1, nd, steps, state);
    return hipGetLastError();
}

hipError_t launch_df_drain(const uint32_t *line, uint64_t n1, uint64_t nd, const uint64_t *state, uint8_t *status,
                           hipStream_t s) {
    if (!nd) return hipSuccess;
    hipLaunchKernelGGL(k_df_drain, flat_grid(nd, kDfThreads), dim3(kDfThreads), 0, s, line, n1, nd, state, status);
    return hipGetLastError();
}

hipError_t launch_df_flag(uint64_t L, const uint8_t *status, uint32_t *uflag, hipStream_t s) {
    hipLaunchKernelGGL(k_df_flag, dim3(grid_for(L + 1, kDfThreads * 4, 2048)), dim3(kDfThreads), 0, s, L, status, uflag);
    return hipGetLastError();
}

hipError_t launch_df_place(uint64_t L, const uint32_t *uflag, const uint64_t *uord, const uint64_t *koff,
                           const uint64_t *klen, uint64_t *len, uint64_t *src, hipStream_t s) {
    hipLaunchKernelGGL(k_df_place, dim3(grid_for(L + 1, kDfThreads * 4, 2048)), dim3(kDfThreads), 0, s, L, uflag, uord, koff,
                       klen, len, src);
    return hipGetLastError();
}

hipError_t launch_df_sum(uint64_t L, const uint64_t *ord, const uint64_t *uord, const unsigned long long *counters,
                         uint64_t *sum, hipStream_t s) {
    hipLaunchKernelGGL(k_df_sum, dim3(1), dim3(kWave), 0, s, L, ord, uord, counters, sum);
    return hipGetLastError();
}

}  // namespace vcfxg
