// vcfxg_fx.hip -- VCFX_field_extractor's projection (VCFX_field_extractor.cpp:319-505 file mode,
// :538-702 stdin mode): every data line becomes one TSV row of cells, each cell found by name inside
// the record.
//
// Byte model.  An output column is a standard column (fields 0..7), an INFO key, or one sub-field of
// one sample column; a cell is (offset from the line's start, length) of input bytes, or one of the
// constants "." (kFxDot) and "1" (kFxOne, an INFO flag) in the length word.  A row is its cells'
// bytes joined by tabs, then '\n'.  The table (fx_table_words) holds the columns, the INFO keys, the
// distinct sub-fields, the sample cells and the requested sample columns as a bitmask with a rank
// word per mask word (SxArgs::mask is the model); it is in LDS when it fits kFxTableLds bytes and read
// from global memory otherwise.
//
// Two passes over the indexed lines:
//   k_fx_cells  a wave per line.  (1) sx_walk's sweep, 16 B per lane and 1 KiB per step, tab masks
//               from the loaded bytes, the tab count carried across the lanes by a DPP scan and
//               across the steps in a scalar register: the lanes that own tabs 1..9 leave them in
//               LDS, the lanes that own a requested sample column's two tabs leave its span in
//               global memory; the sweep STOPS at the step that ends the last needed field.  (2) the
//               standard cells.  (3) the INFO keys and (4) the FORMAT sub-fields, each one token
//               sweep of vcfxg_fields.h over that field alone.  (5) per sample cell the colon token
//               with the sub-field's index.  (6) the row's length.  A cell is written, and read
//               again, only by lane (column mod 64): first match (file mode) and last match (stdin
//               mode) across the steps are that lane's read-modify-write.
//   (scans)     rows numbered by the scan of the row flags, row offsets the 64-bit scan of the lengths
//   k_fx_write  a block per tile of kFxTileRows lines, whose rows are one contiguous piece of the
//               text: the lanes copy their cells, tabs and newlines into an LDS stage of kFxStage
//               bytes, the block flushes it as aligned 16 B stores (only the tile's first and last
//               piece, shared with the neighbouring tiles, go byte by byte), window after window for
//               rows longer than the stage.
#include <type_traits>

#include "vcfxg_device.h"
#include "vcfxg_fields.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kFxThreads = 256;
constexpr int kFxWaves = kFxThreads / kWave;

// the table's words from LDS, or from global memory by a vector load whose index is kept in a vector
// register (scalar loads, with their 64-bit addresses and clustered results, filled the scalar registers
// until they spilled).  u(i): a word that every lane asks for, in a scalar register.
template <bool kLds>
struct FxTab {
    const uint32_t *w;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const {
        if (!kLds) asm volatile("" : "+v"(i));
        return w[i];
    }
    __device__ __forceinline__ uint32_t u(uint32_t i) const {
        return kLds ? w[i] : (uint32_t)uniform32((int)(*this)(i));
    }
};

// keys of `stride` words each at word `base`: {pool offset, length, ...}; the pool at word `pool`
template <bool kLds>
struct FxKeys {
    FxTab<kLds> T;
    uint32_t base, stride, pool;
    __device__ __forceinline__ uint32_t len(uint32_t k) const { return T(base + k * stride + 1u); }
    __device__ __forceinline__ uint32_t byte(uint32_t k, uint32_t i) const {
        const uint32_t o = T(base + k * stride) + i;
        return (T(pool + (o >> 2)) >> ((o & 3u) * 8u)) & 0xFFu;
    }
};

// the wave's LDS accesses before this point are complete and visible to its other lanes
__device__ __forceinline__ void fx_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// ... and its global stores to its other lanes (one compute unit, one L1)
__device__ __forceinline__ void fx_wave_sync_global() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool kLds>
__global__ __launch_bounds__(kFxThreads) void k_fx_cells(const char *__restrict__ buf, uint32_t n,
                                                         const uint32_t *__restrict__ tab, uint32_t tab_words,
                                                         const FxOut *__restrict__ O) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];
    __shared__ uint32_t s_t[kFxWaves][12];
    __shared__ uint32_t s_head[kFxHWords];  // (the header's words in LDS for both variants)
    if (threadIdx.x < kFxHWords) s_head[threadIdx.x] = tab[threadIdx.x];
    if (kLds)
        for (uint32_t i = threadIdx.x; i < tab_words; i += blockDim.x) s_tab[i] = tab[i];
    __syncthreads();
    const FxTab<kLds> T{kLds ? s_tab : tab};
    // (the header's words are read where a phase uses them, behind a compiler barrier, so that they do
    // not all stay in scalar registers across the whole line loop: kept there they spilled)
#define FX_PHASE() asm volatile("" ::: "memory")
    uint32_t *wt = s_t[threadIdx.x / kWave];  // wt[f] = the tab before field f (1..9), from the line's start
    // (line numbers fit 31 bits: vcfxg_fields_scan refuses more)
    const uint32_t wid = (uint32_t)uniform32((int)((blockIdx.x * blockDim.x + threadIdx.x) / kWave));
    const uint32_t nw = (gridDim.x * blockDim.x) / kWave;
    for (uint32_t li = wid; li < n; li += nw) {
        FX_PHASE();
        const bool stdin_mode = s_head[kFxHStdin] != 0u;
        const uint32_t ncols = s_head[kFxHNcols], nsc = s_head[kFxHNsc];
        const int64_t ls = li ? (int64_t)O->line_end[li - 1] + 1 : O->data_start;
        int64_t le = (int64_t)O->line_end[li];
        if (!stdin_mode && le > ls && byte_at(buf, le - 1) == '\r') le--;
        if (le <= ls || byte_at(buf, ls) == '#') {
            if (lane() == 0) {
                O->status[li] = le <= ls ? kFxEmpty : kFxHeader;
                O->isrow[li] = 0u;
                O->rowlen[li] = 0u;
            }
            continue;
        }
        const uint32_t L = (uint32_t)(le - ls);
        uint32_t *row = O->cells + (uint64_t)li * ncols * 2u;
        // (1) the sweep
        uint32_t nt = 0;  // tabs before this step (wave-uniform)
        {
        const uint32_t lastk = s_head[kFxHLastk], nwords = s_head[kFxHNwords], o_mask = s_head[kFxHMask], o_rank = s_head[kFxHRank];
        uint32_t *sp = O->spans + (uint64_t)li * nsc * 2u;
        for (int64_t w = ls & ~(int64_t)15; w < le; w += kWaveStep) {
            const int64_t blk = w + (int64_t)lane() * kBlockBytes;
            uint32_t tm = 0;
            if (blk < le) tm = eq_mask16(load16(buf, blk), kRepTab) & range_mask16(blk, ls, le);
            const uint32_t c = (uint32_t)__popc(tm);
            const uint32_t incl = wave_incl_scan32(c);
            const uint32_t base = nt + incl - c;  // the field number of the lane's first byte
            nt += lane_last(incl);
            if (tm) {
                uint64_t kb = 0;  // bit i = field base + i is a requested sample column
                if (nsc && base + 16u >= 9u) {
                    const uint32_t i0 = min(base >> 5, nwords), i1 = min(i0 + 1u, nwords + 1u);
                    kb = ((((uint64_t)T(o_mask + i1)) << 32) | T(o_mask + i0)) >> (base & 31u);
                }
                uint32_t t = base < 9u || kb ? tm : 0u, i = 0;  // (past field 9 only a requested column's tabs matter)
                while (t) {
                    const uint32_t p = (uint32_t)(blk - ls) + (uint32_t)__builtin_ctz(t);
                    t &= t - 1u;
                    i++;
                    const uint32_t f = base + i;  // the tab ends field f - 1 and opens field f
                    if (f <= 9u) wt[f] = p;
                    if ((kb >> i) & 1u) sp[2u * (T(o_rank + (f >> 5)) + (uint32_t)__popc(T(o_mask + (f >> 5)) & ((1u << (f & 31u)) - 1u)))] = p + 1u;
                    if ((kb >> (i - 1u)) & 1u) {
                        const uint32_t g = f - 1u;
                        sp[2u * (T(o_rank + (g >> 5)) + (uint32_t)__popc(T(o_mask + (g >> 5)) & ((1u << (g & 31u)) - 1u))) + 1u] = p;
                    }
                }
            }
            if (nt > lastk) break;  // (nt is exact up to lastk + 1: every counted tab has been recorded)
        }
        }
        fx_wave_sync();
        if (nsc) fx_wave_sync_global();
        // field f <= 8 is [f_start(f), f_end(f)) when nt >= f
        auto f_start = [&](uint32_t f) { return f ? wt[f] + 1u : 0u; };
        auto f_end = [&](uint32_t f) { return nt >= f + 1u ? wt[f + 1u] : L; };
        // (2) the standard cells; every other cell starts as "."
        FX_PHASE();
        for (uint32_t c = (uint32_t)lane(), o_cols = s_head[kFxHCols]; c < ncols; c += kWave) {
            uint32_t off = 0, len = kFxDot;
            const uint32_t f = T(o_cols + 2u * c + 1u);
            if (T(o_cols + 2u * c) == kFxStd && nt >= f) off = f_start(f), len = f_end(f) - off;
            row[2u * c] = off;
            row[2u * c + 1u] = len;
        }
        // (3) the INFO keys
        FX_PHASE();
        const uint32_t nkeys = s_head[kFxHNkeys], o_pool = s_head[kFxHPool];
        if (nkeys && nt >= 7u) {
            const uint32_t o_keys = s_head[kFxHKeys];
            const uint32_t a = f_start(7u), b = f_end(7u);
            bool ok = b > a;
            if (ok) {
                const uint32_t b0 = byte16(load16(buf, (ls + a) & ~(int64_t)15), (uint32_t)((ls + a) & 15));
                ok = stdin_mode ? b0 != '.' : !(b - a == 1u && b0 == '.');
            }
            if (ok) {
                const FxKeys<kLds> K{T, o_keys, 3u, o_pool};
                auto hit = [&](uint32_t k, uint32_t, uint32_t e, uint32_t d, uint32_t) {
                    const uint32_t c = T.u(o_keys + 3u * k + 2u);
                    if ((uint32_t)lane() == (c & 63u) && (stdin_mode || row[2u * c + 1u] == kFxDot)) {
                        row[2u * c] = e < d ? e + 1u : 0u;
                        row[2u * c + 1u] = e < d ? d - e - 1u : kFxOne;
                    }
                };
                info_find_keys(buf, ls, le, a, b, stdin_mode ? kTokNonEmpty : kTokBeforeEnd, stdin_mode, nkeys, K, hit);
            }
        }
        FX_PHASE();
        const uint32_t nsamp = s_head[kFxHNsamp];
        if (nsamp && nt >= 9u) {
            const uint32_t nsub = s_head[kFxHNsub], o_subs = s_head[kFxHSubs], o_samp = s_head[kFxHSamp];
            // (4) the index of every distinct sub-field inside FORMAT
            uint32_t *sub = O->subidx + (uint64_t)li * nsub;
            for (uint32_t j = (uint32_t)lane(); j < nsub; j += kWave) sub[j] = kFieldNone;
            const FxKeys<kLds> K{T, o_subs, 2u, o_pool};
            auto hit = [&](uint32_t k, uint32_t, uint32_t, uint32_t, uint32_t ord) {
                if ((uint32_t)lane() == (k & 63u) && sub[k] == kFieldNone) sub[k] = ord;
            };
            format_find_keys(buf, ls, le, f_start(8u), f_end(8u), nsub, K, hit);
            // (5) the sample cells
            const uint32_t *sp = O->spans + (uint64_t)li * nsc * 2u;
            for (uint32_t i = 0; i < nsamp; i++) {
                const uint32_t c = T.u(o_samp + 4u * i), col = T.u(o_samp + 4u * i + 1u), j = T.u(o_samp + 4u * i + 2u);
                const uint32_t sw = T.u(o_samp + 4u * i + 3u), sid = sw & 0x7FFFFFFFu;
                if (!col || col > nt || ((sw >> 31) && (uint64_t)ls < O->names_from)) continue;
                uint32_t cur = kFxDot, idx = 0;
                if (stdin_mode) {  // (INFO was asked first)
                    if ((uint32_t)lane() == (c & 63u)) cur = row[2u * c + 1u];
                    cur = (uint32_t)__shfl((int)cur, (int)(c & 63u));
                }
                if (cur != kFxDot) continue;
                if ((uint32_t)lane() == (sid & 63u)) idx = sub[sid];
                idx = (uint32_t)__shfl((int)idx, (int)(sid & 63u));
                if (idx == kFieldNone) continue;
                const uint32_t a = sp[2u * j], b = col < nt ? sp[2u * j + 1u] : L;
                uint32_t off, len;
                if (nth_colon_token(buf, ls, le, a, b, idx, off, len) && (uint32_t)lane() == (c & 63u)) {
                    row[2u * c] = off;
                    row[2u * c + 1u] = len;
                }
            }
        }
        // (6) file mode prints an empty value as "."; the row's bytes
        FX_PHASE();
        uint64_t sum = 0;
        for (uint32_t c = (uint32_t)lane(); c < ncols; c += kWave) {
            uint32_t len = row[2u * c + 1u];
            if (len == 0u && !stdin_mode) {
                row[2u * c] = 0u;
                row[2u * c + 1u] = len = kFxDot;
            }
            sum += len >= kFxOne ? 1u : len;
        }
        sum = wave_sum(sum);
        if (lane() == 0) {
            O->status[li] = kFxRow;
            O->isrow[li] = 1u;
            O->rowlen[li] = sum + ncols;
        }
        fx_wave_sync();  // (wt is the next line's)
    }
#undef FX_PHASE
}

// the cell's text bytes [q0, q1) to stage positions [at + q0, ...) (at may be negative: the window
// starts inside the cell)
__device__ __forceinline__ void fx_copy(const char *__restrict__ buf, int64_t src, uint32_t q0, uint32_t q1, char *stage,
                                        int64_t at) {
    for (int64_t blk = (src + q0) & ~(int64_t)15; blk < src + (int64_t)q1; blk += 16) {
        const uint4 v = load16(buf, blk);  // (holds a byte of the cell: inside the line)
        const int64_t lo = blk > src + q0 ? blk : src + q0, hi = blk + 16 < src + q1 ? blk + 16 : src + q1;
        for (int64_t p = lo; p < hi; p++) stage[at + (p - src)] = (char)byte16(v, (uint32_t)(p - blk));
    }
}

__global__ __launch_bounds__(kFxThreads) void k_fx_write(const char *__restrict__ buf, int64_t data_start,
                                                         const uint64_t *__restrict__ line_end, uint64_t n, uint32_t ncols,
                                                         const uint8_t *__restrict__ status,
                                                         const uint64_t *__restrict__ rowoff,
                                                         const uint32_t *__restrict__ cells, char *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) char stage[kFxStage];
    {
        const uint64_t l0 = (uint64_t)blockIdx.x * kFxTileRows, l1 = l0 + kFxTileRows < n ? l0 + kFxTileRows : n;
        const uint64_t O0 = rowoff[l0], O1 = rowoff[l1];
        for (uint64_t w0 = O0 & ~15ull; w0 < O1; w0 += kFxStage) {
            const uint64_t w1 = w0 + kFxStage < O1 ? w0 + kFxStage : O1;
            for (uint64_t li = l0 + threadIdx.x / kWave; li < l1; li += kFxWaves) {
                if (status[li] != kFxRow) continue;
                const uint64_t ro = rowoff[li];
                if (rowoff[li + 1] <= w0 || ro >= w1) continue;
                const int64_t ls = li ? (int64_t)line_end[li - 1] + 1 : data_start;
                const uint32_t *row = cells + li * ncols * 2u;
                uint64_t done = 0;  // the row's bytes before these 64 columns
                for (uint32_t c0 = 0; c0 < ncols; c0 += kWave) {
                    const uint32_t c = c0 + (uint32_t)lane();
                    const bool valid = c < ncols;
                    const uint32_t off = valid ? row[2u * c] : 0u, len = valid ? row[2u * c + 1u] : 0u;
                    const uint32_t tl = len >= kFxOne ? 1u : len;  // the cell's text; then its tab or the '\n'
                    const uint64_t mine = valid ? (uint64_t)tl + 1u : 0u;
                    const uint64_t incl = wave_incl_scan(mine);
                    const uint64_t pos = ro + done + incl - mine;
                    done += wave_bcast(incl, kWave - 1);
                    // (no lane leaves the loop body early: the next round's scan needs them all)
                    if (valid && pos < w1 && pos + mine > w0) {
                        // text bytes [q0, q1) of the cell fall into the window: stage positions
                        // at + q, 0 <= at + q0 and at + q1 <= w1 - w0 <= kFxStage
                        const uint32_t q0 = pos < w0 ? (uint32_t)(w0 - pos) : 0u;
                        const uint32_t q1 = pos + tl > w1 ? (uint32_t)(w1 - pos) : tl;
                        const int64_t at = (int64_t)(pos - w0);  // (as a signed difference: negative when pos < w0)
                        if (q0 < q1) {
                            if (len >= kFxOne) stage[at] = len == kFxDot ? '.' : '1';  // (tl = 1, q0 = 0: pos >= w0)
                            else fx_copy(buf, ls + (int64_t)off, q0, q1, stage, at);
                        }
                        const uint64_t sep = pos + tl;
                        if (sep >= w0 && sep < w1) stage[sep - w0] = c + 1u == ncols ? '\n' : '\t';
                    }
                }
            }
            __syncthreads();
            for (uint64_t g = w0 + 16ull * threadIdx.x; g < w1; g += 16ull * kFxThreads) {
                const char *s = stage + (g - w0);
                if (g >= O0 && g + 16 <= O1) {
                    *reinterpret_cast<uint4 *>(out + g) = *reinterpret_cast<const uint4 *>(s);
                } else {  // the tile's first or last piece: its other bytes are a neighbouring tile's
                    const uint64_t a = g > O0 ? g : O0, b = g + 16 < O1 ? g + 16 : O1;
                    for (uint64_t p = a; p < b; p++) out[p] = s[p - g];
                }
            }
            __syncthreads();
        }
    }
}

hipError_t launch_fx_cells(const char *buf, uint64_t n, const uint32_t *table, uint32_t table_words, const FxOut *out,
                           hipStream_t s) {
    if (!n) return hipSuccess;
    if (n >= (1ull << 31)) return hipErrorInvalidValue;
    const uint64_t want = (n + kFxWaves - 1) / kFxWaves;
    const unsigned blocks = (unsigned)(want < 16384 ? want : 16384);
    if (fx_table_in_lds(table_words))
        hipLaunchKernelGGL(k_fx_cells<true>, dim3(blocks), dim3(kFxThreads), 4 * (size_t)table_words, s, buf, (uint32_t)n,
                           table, table_words, out);
    else
        hipLaunchKernelGGL(k_fx_cells<false>, dim3(blocks), dim3(kFxThreads), 0, s, buf, (uint32_t)n, table, table_words,
                           out);
    return hipGetLastError();
}

hipError_t launch_fx_write(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t n, uint32_t ncols,
                           const uint8_t *status, const uint64_t *rowoff, const uint32_t *cells, char *out, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t tiles = (n + kFxTileRows - 1) / kFxTileRows;  // (a block each)
    if (tiles >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fx_write, dim3((unsigned)tiles), dim3(kFxThreads), 0, s, buf, data_start,
                       line_end, n, ncols, status, rowoff, cells, out);
    return hipGetLastError();
}

}  // namespace vcfxg
