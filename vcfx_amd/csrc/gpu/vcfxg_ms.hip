// vcfxg_ms.hip -- VCFX_multiallelic_splitter's recode (VCFX_multiallelic_splitter.cpp:247-420,
// processFileMmap :422-646, splitMultiAllelicVariants :652-758): a data line of >= 9 fields whose
// ALT holds a comma becomes one output row per ALT allele, each with its INFO items and sample
// sub-fields recoded for that allele.  The first kernels here whose output is not a selection of
// the input's bytes, and the first to write more lines than they read.
//
// Byte model.  With t0..t8 the line's first nine tabs (t8 = the line's end when it has nine
// fields), row a (0-based, j = a + 1) of a line with n alleles is
//     [ls, t3]  alts[a]  [t4, t6]  INFO'  [t7, t8)  { '\t' sample' }  '\n'
// INFO' = the non-empty ';' items joined by ';' ("." when there is none), an item "key=value"
// whose key the table has as an INFO entry recoded in its value; sample' = one sub-field per
// FORMAT key joined by ':', "." for a key the sample has no sub-field for, sub-fields past the keys
// dropped.  A value is recoded by its key's class: A -> vals[j - 1], R -> vals[0],vals[j],
// G -> vals[0],vals[j],vals[(2n + 1 - j) j / 2] when it has (n + 1)(n + 2) / 2 values, else ".",
// GT -> each side of the first '/' or '|' mapped 0 -> 0, . -> ., j -> 1, else ., "." when both
// are; any other class is copied.  File mode drops one trailing tab of the line before counting
// fields; '\r' is a byte of the last field in both modes.
//
// The table (ID bytes, INFO | FORMAT, class A / R / G; one entry per ID) sits in LDS up to
// kMsTableLds bytes and is read from global memory past that.  The classes of a line's first
// kMsKeysLds FORMAT keys sit in LDS, per wave; a later key's class is looked up where it is used.
//
// Passes (vcfxg_api_ms.hip):
//   k_ms_scan    a wave per line: status, the nine tab offsets, nAlts, the line's cost in bytes
//   (scans)      hipcub exclusive sums: nAlts -> each line's first row; cost -> the block's cut
//   k_ms_cut     the lines this call takes (cost within the budget) and their rows
//   k_ms_len     a wave per row: the fixed parts' bytes; INFO and the samples swept 1 KiB a step,
//                16 B a lane, every lane recoding serially the items that start in its bytes
//   (scan)       hipcub exclusive sum of the row lengths
//   k_ms_write   the same walk: a wave scan of the lanes' item lengths places each item, the lane
//                writes it with byte stores
//   k_ms_ranges  each line's text offset, the data-line count
// Outside the domain (as the reference's int arithmetic): a GT allele index of more than 9
// digits, an ALT of 46,340 or more alleles; and a line of 2 GiB or more (offsets within a line,
// and the output bytes of a row's INFO field and of its samples, are 32-bit).
#include <algorithm>

#include "vcfxg_device.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kMsThreads = 256;
constexpr int kMsWaves = kMsThreads / kWave;
constexpr uint32_t kClsGt = 4;  // (device only: the key "GT"; 0..3 = kMsOther, kMsA, kMsR, kMsG)

// entries e[3 i ..]: the ID's offset from e in bytes, its length, section << 8 | class
struct MsTab {
    const uint32_t *e;
    uint32_t n;
};

struct MsArgs {
    const char *buf;
    int64_t data_start;
    const uint64_t *line_end;
    uint64_t l0;
    int stdin_mode;
    const uint32_t *table;
    uint32_t table_bytes, entries;
};

__device__ __forceinline__ void ms_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the table into LDS by the whole block when it fits
__device__ __forceinline__ MsTab ms_table(const MsArgs &A, uint32_t *s_tab) {
    if (A.table_bytes > kMsTableLds) return MsTab{A.table, A.entries};
    for (uint32_t i = threadIdx.x; i < A.table_bytes / 4u; i += blockDim.x) s_tab[i] = A.table[i];
    __syncthreads();
    return MsTab{s_tab, A.entries};
}

// the class of the key buf[ks, ke) in section sect, kMsOther when the table lacks it there
__device__ __forceinline__ uint32_t ms_lookup(const MsTab &T, const char *__restrict__ buf, int32_t ks, int32_t ke,
                                              uint32_t sect) {
    const uint32_t len = (uint32_t)(ke - ks);
    for (uint32_t i = 0; i < T.n; i++) {
        if (T.e[3u * i + 1u] != len) continue;
        const char *id = reinterpret_cast<const char *>(T.e) + T.e[3u * i];
        uint32_t k = 0;
        while (k < len && (uint32_t)(uint8_t)id[k] == byte_at(buf, ks + k)) k++;
        if (k == len) {
            const uint32_t sc = T.e[3u * i + 2u];
            return (sc >> 8) == sect ? (sc & 0xFFu) : (uint32_t)kMsOther;
        }
    }
    return kMsOther;
}

// the class of FORMAT [fs, fe)'s key i (i < its key count)
__device__ __forceinline__ uint32_t ms_key_class(const MsTab &T, const char *__restrict__ buf, int32_t fs, int32_t fe,
                                                 uint32_t i) {
    int32_t p = fs;
    for (uint32_t k = 0; k < i; k++) {
        while (p < fe && byte_at(buf, p) != ':') p++;
        p++;
    }
    int32_t q = p;
    while (q < fe && byte_at(buf, q) != ':') q++;
    if (q - p == 2 && byte_at(buf, p) == 'G' && byte_at(buf, p + 1) == 'T') return kClsGt;
    return ms_lookup(T, buf, p, q, kMsFormat);
}

// bytes equal to ch in [a, b) (wave-cooperative, wave-uniform)
__device__ __forceinline__ uint32_t ms_count(const char *__restrict__ buf, int32_t a, int32_t b, uint32_t ch) {
    uint32_t c = 0;
    for (int32_t w = a; w < b; w += kWave) {
        const int32_t p = w + lane();
        c += (uint32_t)__popcll(__ballot(p < b && byte_at(buf, p) == ch));
    }
    return c;
}

// piece k (0-based) of the comma list [a, b) (k <= its commas): [ps, pe) (wave-cooperative: a
// comma's rank is the commas in the lanes below it, and the commas of rank k - 1 and k say so)
__device__ __forceinline__ void ms_piece(const char *__restrict__ buf, int32_t a, int32_t b, uint32_t k, int32_t &ps,
                                         int32_t &pe) {
    uint32_t seen = 0;
    ps = a;
    pe = b;
    for (int32_t w = a; w < b; w += kWave) {
        const int32_t p = w + lane();
        const bool comma = p < b && byte_at(buf, p) == ',';
        const uint64_t m = __ballot(comma);
        const uint32_t rank = seen + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const uint64_t ms = __ballot(comma && rank + 1u == k), me = __ballot(comma && rank == k);
        if (ms) ps = w + __builtin_ctzll(ms) + 1;
        if (me) {
            pe = w + __builtin_ctzll(me);
            break;
        }
        seen += (uint32_t)__popcll(m);
    }
}

// ---- a lane's serial recode -------------------------------------------------------------------

struct MsLen {
    uint32_t n = 0;
    __device__ __forceinline__ void put(char) { n++; }
    __device__ __forceinline__ void copy(const char *, int32_t a, int32_t b) { n += (uint32_t)(b - a); }
};
struct MsPut {
    char *p;
    __device__ __forceinline__ void put(char c) { *p++ = c; }
    __device__ __forceinline__ void copy(const char *__restrict__ buf, int32_t a, int32_t b) {
        for (; a < b; a++) *p++ = buf[a];
    }
};

// what a row's lanes share (wave-uniform)
struct MsRow {
    const char *buf;     // the line's first byte: every offset below counts from it
    MsTab T;
    const uint8_t *cls;  // the classes of the first kMsKeysLds keys
    int32_t fs, fe;      // FORMAT
    uint32_t nk, j, n;   // its keys; the allele kept (1-based) of n
};

// one side of a genotype: conv of recodeSample :365-379
__device__ __forceinline__ char ms_gt_side(const char *__restrict__ buf, int32_t a, int32_t b, uint32_t j) {
    if (b - a == 1) {
        const uint32_t c = byte_at(buf, a);
        if (c == '0') return '0';
        if (c == '.') return '.';
    }
    uint32_t idx = 0;
    for (int32_t i = a; i < b; i++) {
        const uint32_t d = byte_at(buf, i) - '0';
        if (d > 9u) return '.';
        idx = idx * 10u + d;
    }
    return idx == j ? '1' : '.';
}

// the value [p, q) recoded by class c
template <typename Sink>
__device__ __forceinline__ void ms_value(Sink &S, const MsRow &R, uint32_t c, int32_t p, int32_t q) {
    const char *__restrict__ buf = R.buf;
    if (c == kMsOther) {
        S.copy(buf, p, q);
        return;
    }
    if (c == kClsGt) {
        int32_t d = p;
        while (d < q && byte_at(buf, d) != '/' && byte_at(buf, d) != '|') d++;
        if (d == q) {
            S.put('.');
            return;
        }
        const char x = ms_gt_side(buf, p, d, R.j), y = ms_gt_side(buf, d + 1, q, R.j);
        if (x == '.' && y == '.') S.put('.');
        else {
            S.put(x);
            S.put('/');
            S.put(y);
        }
        return;
    }
    // the picks of the comma list, ascending: A {j - 1}, R {0, j}, G {0, j, (2n + 1 - j) j / 2}
    uint32_t k0 = 0, k1 = R.j, k2 = 0;
    uint32_t np = 2;
    if (c == kMsA) {
        k0 = R.j - 1u;
        np = 1;
    } else if (c == kMsR) {
        if (q - p == 1 && byte_at(buf, p) == '.') {  // a lone "."
            S.put('.');
            return;
        }
    } else {
        uint32_t cnt = 1;
        for (int32_t i = p; i < q; i++) cnt += byte_at(buf, i) == ',';
        if (cnt != ((uint64_t)R.n + 1u) * ((uint64_t)R.n + 2u) / 2u) {
            S.put('.');
            return;
        }
        k2 = (uint32_t)((2ull * R.n + 1u - R.j) * R.j / 2u);
        np = 3;
    }
    uint32_t next = 0;
    uint32_t idx = 0;
    int32_t a = p;
    for (int32_t i = p; next < np; i++) {
        if (i < q && byte_at(buf, i) != ',') continue;
        if (idx == (next == 0 ? k0 : next == 1 ? k1 : k2)) {
            if (next) S.put(',');
            S.copy(buf, a, i);
            next++;
        }
        if (i == q) break;
        idx++;
        a = i + 1;
    }
    for (; next < np; next++) {  // the picks the list lacks
        if (next) S.put(',');
        S.put('.');
    }
}

// The item that starts at s (its separator at s - 1) and ends before r1 at the latest.
// info: an INFO item up to ';' -- nothing when empty, else ';' (when lead) and the item;
// else: a sample up to '\t' -- '\t' and one sub-field per FORMAT key.
template <typename Sink>
__device__ __forceinline__ void ms_item(Sink &S, const MsRow &R, int32_t s, int32_t r1, bool info, bool lead) {
    const char *__restrict__ buf = R.buf;
    int32_t p = s;
    uint32_t nkeys = R.nk, c0 = kMsOther;
    const uint32_t term = info ? ';' : ':', stop = info ? ';' : '\t';
    if (info) {
        int32_t e = s, eq = -1;
        for (; e < r1 && byte_at(buf, e) != ';'; e++)
            if (eq < 0 && byte_at(buf, e) == '=') eq = e;
        if (e == s) return;
        if (lead) S.put(';');
        if (eq >= 0) c0 = ms_lookup(R.T, buf, s, eq, kMsInfo);
        if (c0 == kMsOther) {  // a flag, a key the table lacks as INFO, a number kept as it is
            S.copy(buf, s, e);
            return;
        }
        S.copy(buf, s, eq + 1);
        p = eq + 1;
        nkeys = 1;
    } else {
        S.put('\t');
    }
    bool more = true;  // the item has a sub-field for this key
    for (uint32_t i = 0; i < nkeys; i++) {
        if (i) S.put(':');
        if (!more) {
            S.put('.');
            continue;
        }
        int32_t q = p;
        while (q < r1 && byte_at(buf, q) != term && byte_at(buf, q) != stop) q++;
        const uint32_t c = info ? c0 : i < kMsKeysLds ? (uint32_t)R.cls[i] : ms_key_class(R.T, buf, R.fs, R.fe, i);
        ms_value(S, R, c, p, q);
        more = !info && q < r1 && byte_at(buf, q) == ':';
        p = q + 1;
    }
}

// The items of [r0, r1): one starts behind r0 and behind every sep byte.  Returns the bytes of
// all of them, each with its leading separator.  kWrite: item at out + its offset, an INFO item
// one byte earlier and the first without its ';' (the field is the items joined).
template <bool kWrite>
__device__ __forceinline__ uint32_t ms_sweep(const MsRow &R, int32_t r0, int32_t r1, bool info, char *out) {
    const char *__restrict__ buf = R.buf;
    const uint32_t rep = info ? 0x3B3B3B3Bu : kRepTab;
    uint32_t carry = 0, acc = 0;
    // (16 B loads: w + the line's own misalignment is a multiple of 16)
    for (int32_t w = r0 - (int32_t)(((uint32_t)(uintptr_t)buf + (uint32_t)r0) & 15u); w < r1; w += kWaveStep) {
        const int32_t blk = w + lane() * kBlockBytes;
        uint32_t m = 0;
        if (blk < r1) {
            m = eq_mask16(load16(buf, blk), rep) & range16(blk, r0, r1);
            if (r0 >= blk && r0 < blk + 16) m |= 1u << (uint32_t)(r0 - blk);
        }
        uint32_t cnt = 0;
        for (uint32_t mm = m; mm; mm &= mm - 1u) {
            MsLen L;
            ms_item(L, R, blk + __builtin_ctz(mm) + 1, r1, info, true);
            cnt += L.n;
        }
        if (kWrite) {
            const uint32_t incl = wave_incl_scan32(cnt);
            uint32_t off = carry + incl - cnt;
            for (uint32_t mm = m; mm; mm &= mm - 1u) {
                const bool lead = !info || off != 0;
                char *const p0 = out + off - (info && off ? 1u : 0u);
                MsPut P{p0};
                ms_item(P, R, blk + __builtin_ctz(mm) + 1, r1, info, lead);
                if (P.p != p0) off += (uint32_t)(P.p - p0) + (lead ? 0u : 1u);
            }
            carry += lane_last(incl);
        } else {
            acc += cnt;
        }
    }
    return kWrite ? carry : wave_sum<uint32_t>(acc);
}

__device__ __forceinline__ int32_t ms_geom(const uint32_t *__restrict__ g, int k) { return uniform32((int)g[k]); }

__device__ __forceinline__ void ms_copy(char *__restrict__ out, const char *__restrict__ buf, int32_t a, int32_t b) {
    for (int32_t i = a + lane(); i < b; i += kWave) out[i - a] = buf[i];
}

// ---- kernels ------------------------------------------------------------------------------------

// per line: status, nAlts (alt[li]; 0 unless the line splits), geom[10]: the nine tabs and the end
// (offsets from the line's start; tab 8 = the end on a line of nine fields), its cost in text bytes
__global__ __launch_bounds__(kMsThreads) void k_ms_scan(MsArgs A, uint64_t n, uint8_t *__restrict__ status,
                                                        int32_t *__restrict__ alt, uint32_t *__restrict__ geom,
                                                        uint64_t *__restrict__ cost) {
    __shared__ uint32_t s_t[kMsWaves][kMsGeom];
    const char *__restrict__ buf = A.buf;
    uint32_t *t = s_t[threadIdx.x / kWave];
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t nw = (gridDim.x * (uint64_t)blockDim.x) / kWave;
    for (uint64_t i = wid; i < n; i += nw) {
        const uint64_t li = A.l0 + i;
        const int64_t ls = li ? (int64_t)A.line_end[li - 1] + 1 : A.data_start;
        const int64_t le = (int64_t)A.line_end[li];
        uint8_t st = kMsEmpty;
        uint32_t nalt = 0;
        if (le > ls) {
            if (byte_at(buf, ls) == '#') st = kMsHeader;
            else {
                st = kMsCopy;
                int64_t end = le;
                if (!A.stdin_mode && byte_at(buf, le - 1) == '\t') end--;  // (no trailing empty field)
                uint32_t nt = 0;
                for (int64_t w = ls & ~(int64_t)15; w < end && nt < 9u; w += kWaveStep) {
                    const int64_t blk = w + (int64_t)lane() * kBlockBytes;
                    uint32_t m = 0;
                    if (blk < end) m = eq_mask16(load16(buf, blk), kRepTab) & range_mask16(blk, ls, end);
                    const uint32_t c = (uint32_t)__popc(m);
                    const uint32_t incl = wave_incl_scan32(c);
                    uint32_t idx = nt + incl - c;
                    for (; m && idx < 9u; m &= m - 1u, idx++) t[idx] = (uint32_t)(blk + __builtin_ctz(m) - ls);
                    nt += lane_last(incl);
                }
                ms_wave_sync();
                if (nt >= 8u) {
                    const uint32_t commas = ms_count(buf + ls, (int32_t)t[3] + 1, (int32_t)t[4], ',');
                    if (commas) {
                        st = kMsSplit;
                        nalt = commas + 1u;
                        if (lane() == 0) {
                            if (nt == 8u) t[8] = (uint32_t)(end - ls);
                            t[9] = (uint32_t)(end - ls);
                        }
                        ms_wave_sync();
                        if (lane() < kMsGeom) geom[i * kMsGeom + lane()] = t[lane()];
                    }
                }
                ms_wave_sync();
            }
        }
        if (lane() == 0) {
            status[li] = st;
            alt[li] = (int32_t)nalt;
            cost[i] = (uint64_t)nalt * (uint64_t)(le - ls + 1);
        }
    }
}

// the lines this call takes: the most whose cost stays within the budget, one at least
__global__ void k_ms_cut(const uint64_t *__restrict__ costoff, const uint64_t *__restrict__ rowbase, uint64_t n,
                         uint64_t budget, uint64_t *__restrict__ small) {
    if (threadIdx.x || blockIdx.x) return;
    uint64_t lo = 1, hi = n;  // the largest k in [1, n] with costoff[k] <= budget (k = 1 when none)
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) / 2;
        if (costoff[mid] <= budget) lo = mid;
        else hi = mid - 1;
    }
    small[0] = lo;
    small[1] = rowbase[lo];
}

// Row r of the block: its line and allele from rowbase, then the byte model above.  kWrite: the
// bytes at out + off[r]; else len[r] = their number.
template <bool kWrite>
__device__ __forceinline__ void ms_rows(const MsArgs &A, uint32_t *s_tab, uint8_t (*s_cls)[kMsKeysLds], uint64_t n,
                                        uint64_t rows, const uint64_t *__restrict__ rowbase,
                                        const int32_t *__restrict__ alt, const uint32_t *__restrict__ geom,
                                        uint64_t *__restrict__ len, const uint64_t *__restrict__ off,
                                        char *__restrict__ out, unsigned long long *__restrict__ counters) {
    MsRow R;
    R.T = ms_table(A, s_tab);
    uint8_t *cls = s_cls[threadIdx.x / kWave];
    R.cls = cls;
    const uint64_t wid = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    const uint64_t r = wid;  // (a wave per row and no loop: what finds the row is dead before the sweeps)
    if (r < rows) {
        uint64_t lo = 0, hi = n - 1;  // the line i with rowbase[i] <= r < rowbase[i + 1]
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (rowbase[mid + 1] <= r) lo = mid + 1;
            else hi = mid;
        }
        const uint64_t i = (uint64_t)uniform64((int64_t)lo), li = A.l0 + i;
        const uint32_t a = (uint32_t)(r - rowbase[i]);
        const int64_t ls = li ? (int64_t)A.line_end[li - 1] + 1 : A.data_start;
        const uint32_t *g = geom + i * kMsGeom;
        const int32_t t3 = ms_geom(g, 3), t4 = ms_geom(g, 4), t6 = ms_geom(g, 6), t7 = ms_geom(g, 7), t8 = ms_geom(g, 8),
                      end = ms_geom(g, 9);
        const char *__restrict__ buf = A.buf + ls;
        R.buf = buf;
        R.fs = t7 + 1;
        R.fe = t8;
        R.nk = ms_count(buf, R.fs, R.fe, ':') + 1u;
        R.j = a + 1u;
        R.n = (uint32_t)alt[li];
        if ((uint32_t)lane() < min(R.nk, kMsKeysLds)) cls[lane()] = (uint8_t)ms_key_class(R.T, buf, R.fs, R.fe, (uint32_t)lane());
        ms_wave_sync();
        int32_t ps, pe;
        ms_piece(buf, t3 + 1, t4, a, ps, pe);
        char *o = kWrite ? out + off[r] : nullptr;
        uint64_t L = 0;
        if (kWrite) {
            ms_copy(o, buf, 0, t3 + 1);
            ms_copy(o + (t3 + 1), buf, ps, pe);
            ms_copy(o + (t3 + 1) + (pe - ps), buf, t4, t6 + 1);
        }
        L += (uint64_t)(t3 + 1) + (uint64_t)(pe - ps) + (uint64_t)(t6 + 1 - t4);
        const uint64_t info = ms_sweep<kWrite>(R, t6, t7, true, kWrite ? o + L : nullptr);
        if (kWrite && !info && lane() == 0) o[L] = '.';
        L += info ? info - 1u : 1u;
        if (kWrite) ms_copy(o + L, buf, t7, t8);
        L += (uint64_t)(t8 - t7);
        if (t8 < end) L += ms_sweep<kWrite>(R, t8, end, false, kWrite ? o + L : nullptr);
        if (kWrite) {
            if (lane() == 0) o[L] = '\n';
        } else if (lane() == 0) {
            len[r] = L + 1u;
            if (a == 0 && (R.nk > kMsKeysLds || A.table_bytes > kMsTableLds)) atomicAdd(&counters[1], 1ull);
        }
    }
}

__global__ __launch_bounds__(kMsThreads) void k_ms_len(MsArgs A, uint64_t n, uint64_t rows,
                                                       const uint64_t *__restrict__ rowbase,
                                                       const int32_t *__restrict__ alt, const uint32_t *__restrict__ geom,
                                                       uint64_t *__restrict__ len, unsigned long long *__restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];
    __shared__ uint8_t s_cls[kMsWaves][kMsKeysLds];
    ms_rows<false>(A, s_tab, s_cls, n, rows, rowbase, alt, geom, len, nullptr, nullptr, counters);
}

__global__ __launch_bounds__(kMsThreads) void k_ms_write(MsArgs A, uint64_t n, uint64_t rows,
                                                         const uint64_t *__restrict__ rowbase,
                                                         const int32_t *__restrict__ alt, const uint32_t *__restrict__ geom,
                                                         const uint64_t *__restrict__ off, char *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];
    __shared__ uint8_t s_cls[kMsWaves][kMsKeysLds];
    ms_rows<true>(A, s_tab, s_cls, n, rows, rowbase, alt, geom, nullptr, off, out, nullptr);
}

// lineoff[i] = the text offset of line i's rows (n + 1 entries); counters[0] += the data lines
__global__ void k_ms_ranges(uint64_t l0, uint64_t n, const uint8_t *__restrict__ status,
                            const uint64_t *__restrict__ rowbase, const uint64_t *__restrict__ rowoff,
                            uint64_t *__restrict__ lineoff, unsigned long long *__restrict__ counters) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    bool data = false;
    if (i <= n) lineoff[i] = rowoff[rowbase[i]];
    if (i < n) data = status[l0 + i] == kMsCopy || status[l0 + i] == kMsSplit;
    const uint64_t m = __ballot(data);
    if (lane() == 0 && m) atomicAdd(&counters[0], (unsigned long long)__popcll(m));
}

static MsArgs ms_args(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, int stdin_mode,
                      const uint32_t *table, uint32_t table_bytes, uint32_t entries) {
    MsArgs A;
    A.buf = buf;
    A.data_start = data_start;
    A.line_end = line_end;
    A.l0 = l0;
    A.stdin_mode = stdin_mode;
    A.table = table;
    A.table_bytes = table_bytes;
    A.entries = entries;
    return A;
}

static unsigned ms_blocks(uint64_t waves) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((waves + kMsWaves - 1) / kMsWaves, 8192));
}

static unsigned ms_row_blocks(uint64_t rows) { return (unsigned)((rows + kMsWaves - 1) / kMsWaves); }

hipError_t launch_ms_scan(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                          int stdin_mode, uint8_t *status, int32_t *alt, uint32_t *geom, uint64_t *cost, hipStream_t s) {
    if (!n) return hipSuccess;
    const MsArgs A = ms_args(buf, data_start, line_end, l0, stdin_mode, nullptr, 0, 0);
    hipLaunchKernelGGL(k_ms_scan, dim3(ms_blocks(n)), dim3(kMsThreads), 0, s, A, n, status, alt, geom, cost);
    return hipGetLastError();
}

hipError_t launch_ms_cut(const uint64_t *costoff, const uint64_t *rowbase, uint64_t n, uint64_t budget, uint64_t *small,
                         hipStream_t s) {
    hipLaunchKernelGGL(k_ms_cut, dim3(1), dim3(kWave), 0, s, costoff, rowbase, n, budget, small);
    return hipGetLastError();
}

hipError_t launch_ms_len(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                         int stdin_mode, const uint32_t *table, uint32_t table_bytes, uint32_t entries, uint64_t rows,
                         const uint64_t *rowbase, const int32_t *alt, const uint32_t *geom, uint64_t *len,
                         unsigned long long *counters, hipStream_t s) {
    if (!rows) return hipSuccess;
    const MsArgs A = ms_args(buf, data_start, line_end, l0, stdin_mode, table, table_bytes, entries);
    hipLaunchKernelGGL(k_ms_len, dim3(ms_row_blocks(rows)), dim3(kMsThreads), table_bytes <= kMsTableLds ? table_bytes : 0, s,
                       A, n, rows, rowbase, alt, geom, len, counters);
    return hipGetLastError();
}

hipError_t launch_ms_write(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t l0, uint64_t n,
                           int stdin_mode, const uint32_t *table, uint32_t table_bytes, uint32_t entries, uint64_t rows,
                           const uint64_t *rowbase, const int32_t *alt, const uint32_t *geom, const uint64_t *off,
                           char *out, hipStream_t s) {
    if (!rows) return hipSuccess;
    const MsArgs A = ms_args(buf, data_start, line_end, l0, stdin_mode, table, table_bytes, entries);
    hipLaunchKernelGGL(k_ms_write, dim3(ms_row_blocks(rows)), dim3(kMsThreads), table_bytes <= kMsTableLds ? table_bytes : 0,
                       s, A, n, rows, rowbase, alt, geom, off, out);
    return hipGetLastError();
}

hipError_t launch_ms_ranges(uint64_t l0, uint64_t n, const uint8_t *status, const uint64_t *rowbase,
                            const uint64_t *rowoff, uint64_t *lineoff, unsigned long long *counters, hipStream_t s) {
    hipLaunchKernelGGL(k_ms_ranges, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, l0, n, status, rowbase, rowoff,
                       lineoff, counters);
    return hipGetLastError();
}

}  // namespace vcfxg
