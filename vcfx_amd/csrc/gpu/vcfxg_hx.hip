// vcfxg_hx.hip -- VCFX_haplotype_extractor (VCFX_haplotype_extractor.cpp: processVariantFast :376-568,
// phaseIsConsistent :303-349, outputBlock :362-373): runs of consecutive phased variants cut into
// blocks, a block a row of text, every sample's genotypes along the block joined with '|'.  The first
// kernels here that segment the records, and the first transpose whose cells differ in width.
//
// Byte model.  A member is a data line whose n_samples GT sub-fields all hold a '|'.  Member m opens a
// block unless it has the CHROM of member m - 1, pos[m] - pos[m - 1] <= block size (signed) and, under
// -c, no sample flips between the two.  Row b is
//     CHROM \t START \t END { \t gt(first, s) | gt(first + 1, s) | ... | gt(last, s) }(s < n) \n
// so cell (m, s) is its separator ('\t' for the block's first member, else '|') and its GT, len + 1
// bytes, at  row_off[b] + head[b] + base[b][s] + pre[m][s]:  pre = the exclusive sum of the widths of
// sample s along the block's members up to m, base = the exclusive sum along the samples of the block's
// per-sample totals.
//
// Passes (vcfxg_api_hx.hip):
//   k_hx_scan      a wave per line: status, POS, the GT key's index, CHROM's length; for a member its
//                  cells (GT offset in the line, length: 4 + 4 bytes, so no GT inside the domain is
//                  too long for a cell) into the line-major matrix, a lane per sample start.  A line of
//                  FORMAT "GT" whose samples are all "a|b" is recognised in one masked sweep and stores
//                  no cell: its cells are (region + 4 s, 3) wherever a later pass asks for them
//   (scan)         hipcub exclusive sum of the member flags: the member numbers
//   k_hx_members   member -> line; the per-line member number
//   k_hx_break     a wave per member: CHROM bytes, the signed POS difference and the flip test over
//                  both lines' cells (an any-reduction, the first flipping sample kept)
//   (scan)         exclusive sum of the block-start flags: the block numbers
//   k_hx_blocks    first and last member of every block; block and flip per line
//   k_hx_tile_sum  tiles of 32 members x 64 samples, a lane per sample: the widths summed since the
//                  tile's last block start
//   k_hx_carry     a thread per sample along the tiles: what the open block holds before each tile
//   k_hx_totals    the tile walked again from its carry: the per-sample total at every block end
//   k_hx_rows      a wave per block: the exclusive sum of the totals along the samples (in place),
//                  the head's length, the row's length
//   (scan)         exclusive sum of the row lengths: 64-bit row offsets
//   k_hx_heads     CHROM, START, END in decimal and the '\n' of every row
//   k_hx_emit      the tile once more: wave 0 reads along the samples and leaves every cell and its
//                  offset in LDS (the running sums never leave the registers); then the waves write
//                  along one sample's run, a lane per member, which is contiguous inside a block
// LDS: a tile row is 64 entries of 16 bytes and one entry of padding (1040 bytes), so the 32 lanes that
// read one sample's column fall in 16 different 16-byte slots.
// Outside the domain: a POS above 2147483647 (the sum wraps in 64 bits here, in the reference's int
// there); a NUL byte; a line of 2 GiB or more (offsets within a line are 32-bit).
#include <algorithm>

#include "vcfxg_device.h"
#include "vcfxg_kernels.h"

namespace vcfxg {

constexpr int kHxThreads = 256;
constexpr int kHxWaves = kHxThreads / kWave;
constexpr uint32_t kHxRowEntries = kHxTileSamples + 1;  // 16-byte entries per LDS tile row

static_assert(kHxTileSamples == (uint32_t)kWave, "a lane per sample of the tile");
static_assert(2 * kHxTileMembers == (uint32_t)kWave, "a wave writes two samples' runs, a lane per member");

__device__ __forceinline__ void hx_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int64_t hx_line_start(const uint64_t *__restrict__ line_end, int64_t data_start, uint64_t li) {
    return li ? (int64_t)line_end[li - 1] + 1 : data_start;
}

// the GT sub-field of the sample that starts at st (line offsets; the line's fields end at E): its
// offset and length (extractNthField :196-214: empty when the sample has fewer sub-fields)
__device__ __forceinline__ uint64_t hx_cell(const char *__restrict__ b, int32_t st, int32_t E, int32_t gi, bool &phased) {
    int32_t p = st;
    bool found = true;
    for (int32_t k = 0; k < gi; k++) {
        while (p < E && byte_at(b, p) != ':' && byte_at(b, p) != '\t') p++;
        if (p >= E || byte_at(b, p) == '\t') {
            found = false;
            break;
        }
        p++;
    }
    int32_t q = p;
    bool bar = false;
    if (found)
        for (; q < E; q++) {
            const uint32_t c = byte_at(b, q);
            if (c == ':' || c == '\t') break;
            bar |= c == '|';
        }
    phased = found && bar;
    return (uint64_t)(uint32_t)p | ((uint64_t)(uint32_t)(q - p) << 32);
}

// cell (line, s): a fixed-stride line (fixed[line] = its sample region's offset, never 0) has the closed
// form "a|b" every four bytes and no row in the matrix
__device__ __forceinline__ uint64_t hx_cell_at(const uint64_t *__restrict__ cells, uint32_t fixed_s, uint64_t line,
                                               uint32_t n_samples, uint64_t s) {
    return fixed_s ? (uint64_t)(fixed_s + 4u * (uint32_t)s) | (3ull << 32) : cells[line * (uint64_t)n_samples + s];
}

// the sample region [Sa, Ea) is units "a|b\t" (the last without its tab): tabs at the offsets 3 mod 4 and
// nowhere else, '|' at 1 mod 4, no ':' at 0 and 2 mod 4.  One masked sweep, wave-uniform answer
__device__ __forceinline__ bool hx_fixed_region(const char *__restrict__ buf, int64_t Sa, int64_t Ea) {
    bool off = false;
    for (int64_t w = Sa & ~(int64_t)15; w < Ea; w += kWaveStep) {
        const int64_t blk = w + (int64_t)lane() * kBlockBytes;
        if (blk < Ea) {
            const uint4 v = load16(buf, blk);
            const uint32_t rm = range_mask16(blk, Sa, Ea), ph = (uint32_t)(blk - Sa) & 3u;
            // byte j of the block is at region offset (ph + j) mod 4
            const uint32_t m0 = (0x11111111u << ((0u - ph) & 3u)) & 0xFFFFu, m1 = (0x11111111u << ((1u - ph) & 3u)) & 0xFFFFu,
                           m2 = (0x11111111u << ((2u - ph) & 3u)) & 0xFFFFu, m3 = (0x11111111u << ((3u - ph) & 3u)) & 0xFFFFu;
            off |= (eq_mask16(v, kRepTab) & rm) != (m3 & rm);
            off |= (eq_mask16(v, 0x7C7C7C7Cu) & m1 & rm) != (m1 & rm);
            off |= (eq_mask16(v, kRepColon) & (m0 | m2) & rm) != 0u;
        }
    }
    return !__any(off);
}

// The general sweep of the line at ls with sample region [Sa, Ea]: a lane per sample start in its 16 B
// (the byte Sa and the byte after every later tab; a start may be the byte Ea itself, the empty field
// after a final tab); the start's rank among them is the sample's number.  row[k] = sample k's cell;
// true when the line has n_samples of them and every GT holds a '|'.  EVERY LANE MUST BE ACTIVE.
__device__ __forceinline__ bool hx_sweep_cells(const char *__restrict__ buf, int64_t ls, int64_t Sa, int64_t Ea, int32_t gi,
                                               uint32_t n_samples, uint64_t *__restrict__ row) {
    const char *__restrict__ b = buf + ls;
    const int32_t E = (int32_t)(Ea - ls);
    uint32_t seen = 0;
    bool bad = false;
    for (int64_t w = Sa & ~(int64_t)15; w <= Ea && seen < n_samples; w += kWaveStep) {
        const int64_t blk = w + (int64_t)lane() * kBlockBytes;
        uint32_t starts = 0;
        if (blk <= Ea) {
            const uint32_t tm = blk < Ea ? eq_mask16(load16(buf, blk), kRepTab) & range_mask16(blk, Sa, Ea) : 0u;
            starts = (tm << 1) & 0xFFFFu;
            if (blk > Sa && byte_at(buf, blk - 1) == '\t') starts |= 1u;
            if (Sa >= blk && Sa < blk + 16) starts |= 1u << (Sa - blk);
            const int64_t hi = Ea + 1 - blk;
            if (hi < 16) starts &= (1u << hi) - 1u;
        }
        const uint32_t c = (uint32_t)__popc(starts);
        const uint32_t incl = wave_incl_scan32(c);
        uint32_t k = seen + incl - c;
        for (; starts; starts &= starts - 1u, k++)
            if (k < n_samples) {
                bool ph;
                row[k] = hx_cell(b, (int32_t)(blk + __builtin_ctz(starts) - ls), E, gi, ph);
                bad |= !ph;
            }
        seen += lane_last(incl);
    }
    return seen >= n_samples && !__any(bad);
}

// ---- scan -----------------------------------------------------------------------------------------

__global__ __launch_bounds__(kHxThreads) void k_hx_scan(const char *__restrict__ buf, int64_t data_start,
                                                        const uint64_t *__restrict__ line_end, uint64_t n, int stdin_mode,
                                                        uint32_t n_samples, uint8_t *__restrict__ status,
                                                        int64_t *__restrict__ pos, uint32_t *__restrict__ flag,
                                                        uint32_t *__restrict__ chrom_len, uint32_t *__restrict__ fixed,
                                                        uint32_t *__restrict__ general, uint64_t *__restrict__ cells) {
    __shared__ uint32_t s_t[kHxWaves][12];
    uint32_t *t = s_t[threadIdx.x / kWave];
    // (a wave per line and no loop: fewer values live across the sweeps)
    const uint64_t li = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    if (li < n) {
        const int64_t ls = hx_line_start(line_end, data_start, li);
        const int64_t le = (int64_t)line_end[li];
        uint8_t st = kHxEmpty;
        int64_t pv = 0;
        uint32_t cl = 0, fx = 0;
        if (le > ls) {
            const int64_t end = le - (byte_at(buf, le - 1) == '\r' ? 1 : 0);
            if (end == ls) {
                st = stdin_mode ? kHxShort : kHxEmpty;  // (:739-744: on stdin the strip comes after the test)
            } else if (byte_at(buf, ls) == '#') {
                st = kHxHeader;
            } else {
                uint32_t nt = 0;  // all the line's tabs; the first nine kept
                for (int64_t w = ls & ~(int64_t)15; w < end; w += kWaveStep) {
                    const int64_t blk = w + (int64_t)lane() * kBlockBytes;
                    uint32_t m = 0;
                    if (blk < end) m = eq_mask16(load16(buf, blk), kRepTab) & range_mask16(blk, ls, end);
                    const uint32_t c = (uint32_t)__popc(m);
                    const uint32_t incl = wave_incl_scan32(c);
                    uint32_t idx = nt + incl - c;
                    for (; m && idx < 9u; m &= m - 1u, idx++) t[idx] = (uint32_t)(blk + __builtin_ctz(m) - ls);
                    nt += lane_last(incl);
                    if (nt >= 9u + n_samples) break;  // (fields past the named samples decide nothing)
                }
                hx_wave_sync();
                if (nt < 9u) {
                    st = kHxShort;
                } else {
                    const int32_t t0 = uniform32((int)t[0]), t1 = uniform32((int)t[1]), t7 = uniform32((int)t[7]),
                                  t8 = uniform32((int)t[8]);
                    const char *__restrict__ b = buf + ls;
                    cl = (uint32_t)t0;
                    bool digits = true;
                    uint64_t v = 0;
                    for (int32_t p = t0 + 1; p < t1; p++) {  // (wave-uniform: POS is a few bytes)
                        const uint32_t c = byte_at(b, p) - '0';
                        if (c >= 10u) {
                            digits = false;
                            break;
                        }
                        v = v * 10u + c;
                    }
                    if (!digits) {
                        st = kHxBadPos;
                    } else {
                        pv = (int64_t)v;
                        const int32_t gi = gt_index(buf, ls + t7 + 1, ls + t8);
                        if (gi < 0) {
                            st = kHxNoGt;
                        } else {
                            const int64_t Sa = ls + t8 + 1;
                            if (gi == 0 && t8 - t7 == 3 && end - Sa == 4 * (int64_t)n_samples - 1 && hx_fixed_region(buf, Sa, end)) {
                                st = kHxMember;
                                fx = (uint32_t)t8 + 1u;
                            } else {
                                st = hx_sweep_cells(buf, ls, Sa, end, gi, n_samples, cells + li * (uint64_t)n_samples) ? kHxMember
                                                                                                                     : kHxUnphased;
                            }
                        }
                    }
                }
                hx_wave_sync();
            }
        }
        if (lane() == 0) {
            status[li] = st;
            pos[li] = pv;
            flag[li] = st == kHxMember;
            chrom_len[li] = cl;
            fixed[li] = fx;
            general[li] = st == kHxMember && !fx;
        }
    }
}

// ---- segmentation ---------------------------------------------------------------------------------

__global__ __launch_bounds__(kHxThreads) void k_hx_members(uint64_t n, const uint32_t *__restrict__ flag,
                                                           const uint64_t *__restrict__ mnum, uint64_t *__restrict__ mline,
                                                           uint64_t *__restrict__ lmember, uint64_t *__restrict__ lblock,
                                                           uint32_t *__restrict__ lflip) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) {
        mline[mnum[i]] = i;
        lmember[i] = mnum[i];
    } else {
        lmember[i] = ~0ull;
        lblock[i] = ~0ull;
        lflip[i] = ~0u;
    }
}

// a wave per member m: start[m] = it opens a block; flip[m] = the first sample that flips between
// members m - 1 and m when CHROM and distance let m extend (n_samples: none, or not examined)
__global__ __launch_bounds__(kHxThreads) void k_hx_break(const char *__restrict__ buf, int64_t data_start,
                                                         const uint64_t *__restrict__ line_end, uint64_t nm,
                                                         const uint64_t *__restrict__ mline, const int64_t *__restrict__ pos,
                                                         const uint32_t *__restrict__ chrom_len,
                                                         const uint32_t *__restrict__ fixed,
                                                         const uint64_t *__restrict__ cells, uint32_t n_samples,
                                                         int64_t block_size, int check, uint32_t *__restrict__ start,
                                                         uint32_t *__restrict__ flip) {
    const uint64_t m = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    if (m >= nm) return;
    uint32_t opens = 1, fl = n_samples;
    if (m) {
        const uint64_t i = (uint64_t)uniform64((int64_t)mline[m]), j = (uint64_t)uniform64((int64_t)mline[m - 1]);
        const char *__restrict__ bi = buf + hx_line_start(line_end, data_start, i);
        const char *__restrict__ bj = buf + hx_line_start(line_end, data_start, j);
        const uint32_t ci = chrom_len[i], cj = chrom_len[j];
        bool can = ci == cj && pos[i] - pos[j] <= block_size;
        if (can) {
            bool diff = false;
            for (uint32_t p = (uint32_t)lane(); p < ci; p += kWave) diff |= byte_at(bi, p) != byte_at(bj, p);
            can = !__any(diff);
        }
        if (can && check) {
            const uint32_t fi = fixed[i], fj = fixed[j];
            for (uint32_t s0 = 0; s0 < n_samples; s0 += kWave) {
                const uint32_t s = s0 + (uint32_t)lane();
                bool f = false;
                if (s < n_samples) {
                    const uint64_t cn = hx_cell_at(cells, fi, i, n_samples, s), cp = hx_cell_at(cells, fj, j, n_samples, s);
                    const uint32_t ln = (uint32_t)(cn >> 32), lp = (uint32_t)(cp >> 32);
                    if (ln >= 3u && lp >= 3u) {
                        const uint32_t a = byte_at(bj, (uint32_t)cp), b = byte_at(bj, (uint32_t)cp + lp - 1u);
                        const uint32_t c = byte_at(bi, (uint32_t)cn), d = byte_at(bi, (uint32_t)cn + ln - 1u);
                        f = a != c && b != d && a == d && b == c;
                    }
                }
                const uint64_t fm = __ballot(f);
                if (fm) {
                    fl = s0 + (uint32_t)__builtin_ctzll(fm);
                    break;
                }
            }
        }
        opens = !can || fl < n_samples;
    }
    if (lane() == 0) {
        start[m] = opens;
        flip[m] = fl;
    }
}

__device__ __forceinline__ uint64_t hx_block_of(const uint64_t *__restrict__ bnum, const uint32_t *__restrict__ start, uint64_t m) {
    return bnum[m] + start[m] - 1u;
}

__global__ __launch_bounds__(kHxThreads) void k_hx_blocks(uint64_t nm, const uint64_t *__restrict__ mline,
                                                          const uint32_t *__restrict__ start,
                                                          const uint64_t *__restrict__ bnum, const uint32_t *__restrict__ flip,
                                                          uint64_t *__restrict__ first, uint64_t *__restrict__ last,
                                                          uint64_t *__restrict__ lblock, uint32_t *__restrict__ lflip) {
    const uint64_t m = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (m >= nm) return;
    const uint64_t b = hx_block_of(bnum, start, m);
    if (start[m]) first[b] = m;
    if (m + 1 == nm || start[m + 1]) last[b] = m;
    lblock[mline[m]] = b;
    lflip[mline[m]] = flip[m];
}

// ---- layout ---------------------------------------------------------------------------------------

// block (x, y): members [32 x, 32 x + 32), samples [64 y, 64 y + 64), a lane per sample.
// kTotals = false: agg[x][s] = the widths summed since the tile's last block start (the whole tile's
// when it has none), tstart[x] = it has one.  kTotals = true: the same walk from carry[x][s]; at every
// block end the running sum is the block's total for s.
template <bool kTotals>
__global__ __launch_bounds__(kWave) void k_hx_tile(uint64_t nm, uint32_t n_samples, const uint64_t *__restrict__ mline,
                                                   const uint32_t *__restrict__ start, const uint64_t *__restrict__ bnum,
                                                   const uint32_t *__restrict__ fixed, const uint64_t *__restrict__ cells,
                                                   const uint64_t *__restrict__ carry, uint64_t *__restrict__ out,
                                                   uint32_t *__restrict__ tstart) {
    const uint64_t m0 = (uint64_t)blockIdx.x * kHxTileMembers;
    const uint32_t tm = (uint32_t)std::min<uint64_t>(kHxTileMembers, nm - m0);
    const uint32_t s = blockIdx.y * kHxTileSamples + threadIdx.x;
    const bool in = s < n_samples;
    const uint64_t col = in ? s : 0;  // (lanes past the samples walk column 0 and store nothing)
    uint64_t acc = kTotals ? carry[(uint64_t)blockIdx.x * n_samples + col] : 0;
    uint32_t any = 0;
    for (uint32_t k = 0; k < tm; k++) {
        const uint64_t m = m0 + k;
        if (start[m]) {
            acc = 0;
            any = 1;
        }
        const uint64_t li = mline[m];
        acc += (hx_cell_at(cells, fixed[li], li, n_samples, col) >> 32) + 1u;
        if (kTotals && in && (m + 1 == nm || start[m + 1])) out[hx_block_of(bnum, start, m) * n_samples + s] = acc;
    }
    if (!kTotals) {
        if (in) out[(uint64_t)blockIdx.x * n_samples + s] = acc;
        if (blockIdx.y == 0 && threadIdx.x == 0) tstart[blockIdx.x] = any;
    }
}

// a thread per sample along the tiles: carry[t][s] = what the block open at tile t's first member holds
// of s before it
__global__ __launch_bounds__(kHxThreads) void k_hx_carry(uint64_t n_tiles, uint32_t n_samples,
                                                         const uint64_t *__restrict__ agg, const uint32_t *__restrict__ tstart,
                                                         uint64_t *__restrict__ carry) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_samples) return;
    uint64_t c = 0;
    for (uint64_t t = 0; t < n_tiles; t++) {
        const uint64_t a = agg[t * n_samples + s];
        carry[t * n_samples + s] = c;
        c = tstart[t] ? a : c + a;
    }
}

__device__ __forceinline__ uint32_t hx_digits(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10u) {
        v /= 10u;
        d++;
    }
    return d;
}

// a wave per block b: base[b][s] (in place of the totals), head[b], row_len[b], START and END
__global__ __launch_bounds__(kHxThreads) void k_hx_rows(uint64_t nb, uint32_t n_samples, const uint64_t *__restrict__ first,
                                                        const uint64_t *__restrict__ last, const uint64_t *__restrict__ mline,
                                                        const int64_t *__restrict__ pos, const uint32_t *__restrict__ chrom_len,
                                                        uint64_t *__restrict__ base, uint32_t *__restrict__ head,
                                                        uint64_t *__restrict__ row_len, int64_t *__restrict__ bstart,
                                                        int64_t *__restrict__ bend) {
    const uint64_t b = (uint64_t)uniform64((int64_t)((blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kWave));
    if (b >= nb) return;
    uint64_t *__restrict__ row = base + b * n_samples;
    uint64_t run = 0;
    for (uint32_t s0 = 0; s0 < n_samples; s0 += kWave) {
        const uint32_t s = s0 + (uint32_t)lane();
        const uint64_t v = s < n_samples ? row[s] : 0;
        const uint64_t incl = wave_incl_scan<uint64_t>(v);
        if (s < n_samples) row[s] = run + incl - v;
        run += wave_bcast<uint64_t>(incl, kWave - 1);
    }
    if (lane() == 0) {
        const uint64_t lf = mline[first[b]], ll = mline[last[b]];
        const int64_t ps = pos[lf], pe = pos[ll];
        const uint32_t h = chrom_len[lf] + 1u + hx_digits((uint64_t)ps) + 1u + hx_digits((uint64_t)pe);
        head[b] = h;
        row_len[b] = (uint64_t)h + run + 1u;
        bstart[b] = ps;
        bend[b] = pe;
    }
}

// ---- emit -----------------------------------------------------------------------------------------

__device__ __forceinline__ char *hx_decimal(char *dst, uint64_t v, uint32_t nd) {
    for (uint32_t k = nd; k-- > 0;) {
        dst[k] = (char)('0' + v % 10u);
        v /= 10u;
    }
    return dst + nd;
}

__global__ __launch_bounds__(kHxThreads) void k_hx_heads(const char *__restrict__ buf, int64_t data_start,
                                                         const uint64_t *__restrict__ line_end, uint64_t nb,
                                                         const uint64_t *__restrict__ first, const uint64_t *__restrict__ mline,
                                                         const uint32_t *__restrict__ chrom_len,
                                                         const int64_t *__restrict__ bstart, const int64_t *__restrict__ bend,
                                                         const uint64_t *__restrict__ row_off,
                                                         const uint64_t *__restrict__ row_len, char *__restrict__ text) {
    const uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint64_t li = mline[first[b]];
    const char *__restrict__ src = buf + hx_line_start(line_end, data_start, li);
    char *dst = text + row_off[b];
    const uint32_t cl = chrom_len[li];
    for (uint32_t k = 0; k < cl; k++) dst[k] = src[k];
    dst += cl;
    *dst++ = '\t';
    dst = hx_decimal(dst, (uint64_t)bstart[b], hx_digits((uint64_t)bstart[b]));
    *dst++ = '\t';
    hx_decimal(dst, (uint64_t)bend[b], hx_digits((uint64_t)bend[b]));
    text[row_off[b] + row_len[b] - 1u] = '\n';
}

struct HxEntry {
    uint64_t off;   // the cell's first byte (its separator) from the start of its sample's run in the block
    uint64_t cell;  // GT offset in the line | length << 32
};
static_assert(sizeof(HxEntry) == 16, "an LDS slot");

// block (x, y): members [32 x, 32 x + 32), samples [64 y, 64 y + 64)
__global__ __launch_bounds__(kHxThreads) void k_hx_emit(const char *__restrict__ buf, int64_t data_start,
                                                        const uint64_t *__restrict__ line_end, uint64_t nm, uint32_t n_samples,
                                                        const uint64_t *__restrict__ mline, const uint32_t *__restrict__ start,
                                                        const uint64_t *__restrict__ bnum, const uint32_t *__restrict__ fixed,
                                                        const uint64_t *__restrict__ cells,
                                                        const uint64_t *__restrict__ carry, const uint64_t *__restrict__ base,
                                                        const uint32_t *__restrict__ head, const uint64_t *__restrict__ row_off,
                                                        char *__restrict__ text) {
    __shared__ __attribute__((aligned(16))) HxEntry tile[kHxTileMembers * kHxRowEntries];
    const uint64_t m0 = (uint64_t)blockIdx.x * kHxTileMembers;
    const uint32_t tm = (uint32_t)std::min<uint64_t>(kHxTileMembers, nm - m0);
    const uint32_t s0 = blockIdx.y * kHxTileSamples;
    const uint32_t nsb = std::min<uint32_t>(kHxTileSamples, n_samples - s0);
    const uint32_t wv = threadIdx.x / kWave, ln = (uint32_t)lane();
    // in: wave 0, a lane per sample, along the members
    if (wv == 0 && ln < nsb) {
        const uint32_t s = s0 + ln;
        uint64_t acc = carry[(uint64_t)blockIdx.x * n_samples + s];
        for (uint32_t k = 0; k < tm; k++) {
            const uint64_t m = m0 + k;
            if (start[m]) acc = 0;
            const uint64_t li = mline[m];
            const uint64_t c = hx_cell_at(cells, fixed[li], li, n_samples, s);
            tile[k * kHxRowEntries + ln] = HxEntry{acc, c};
            acc += (c >> 32) + 1u;
        }
    }
    __syncthreads();
    // out: half a wave per sample, a lane per member
    const uint32_t k = ln & (kHxTileMembers - 1u), half = ln / kHxTileMembers;
    if (k >= tm) return;
    const uint64_t m = m0 + k;
    const uint64_t b = hx_block_of(bnum, start, m);
    const char sep = start[m] ? '\t' : '|';
    const char *__restrict__ src = buf + hx_line_start(line_end, data_start, mline[m]);
    const uint64_t row = row_off[b] + head[b];
    const uint64_t *__restrict__ bs = base + b * n_samples + s0;
    for (uint32_t sl = 2u * wv + half; sl < nsb; sl += 2u * kHxWaves) {
        const HxEntry e = tile[k * kHxRowEntries + sl];
        const uint32_t go = (uint32_t)e.cell, len = (uint32_t)(e.cell >> 32);
        char *dst = text + row + bs[sl] + e.off;
        if (len == 3u && ((uintptr_t)dst & 3u) == 0) {  // "a|b" on an aligned dword
            *reinterpret_cast<uint32_t *>(dst) = (uint32_t)(uint8_t)sep | (byte_at(src, go) << 8) | (byte_at(src, go + 1u) << 16) |
                                                 (byte_at(src, go + 2u) << 24);
        } else {
            dst[0] = sep;
            for (uint32_t p = 0; p < len; p++) dst[1u + p] = src[go + p];
        }
    }
}

// ---- launches -------------------------------------------------------------------------------------

static unsigned hx_grid(uint64_t n, uint64_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

uint64_t hx_tiles(uint64_t nm) { return (nm + kHxTileMembers - 1) / kHxTileMembers; }

static bool hx_grid_ok(uint64_t nm, uint32_t n_samples) {
    return hx_tiles(nm) < (1ull << 31) && ((uint64_t)n_samples + kHxTileSamples - 1) / kHxTileSamples <= 65535;
}

hipError_t launch_hx_scan(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t n, int stdin_mode,
                          uint32_t n_samples, uint8_t *status, int64_t *pos, uint32_t *flag, uint32_t *chrom_len,
                          uint32_t *fixed, uint32_t *general, uint64_t *cells, hipStream_t s) {
    if (!n) return hipSuccess;
    if (n >= (1ull << 33)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hx_scan, dim3(hx_grid(n, kHxWaves)), dim3(kHxThreads), 0, s, buf, data_start, line_end, n, stdin_mode, n_samples, status,
                       pos, flag, chrom_len, fixed, general, cells);
    return hipGetLastError();
}

hipError_t launch_hx_members(uint64_t n, const uint32_t *flag, const uint64_t *mnum, uint64_t *mline, uint64_t *lmember,
                             uint64_t *lblock, uint32_t *lflip, hipStream_t s) {
    if (!n) return hipSuccess;
    if (n >= (1ull << 39)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hx_members, dim3(hx_grid(n, kHxThreads)), dim3(kHxThreads), 0, s, n, flag, mnum, mline, lmember, lblock,
                       lflip);
    return hipGetLastError();
}

hipError_t launch_hx_break(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t nm, const uint64_t *mline,
                           const int64_t *pos, const uint32_t *chrom_len, const uint32_t *fixed, const uint64_t *cells,
                           uint32_t n_samples, int64_t block_size, int check, uint32_t *start, uint32_t *flip, hipStream_t s) {
    if (!nm) return hipSuccess;
    if (nm >= (1ull << 33)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hx_break, dim3(hx_grid(nm, kHxWaves)), dim3(kHxThreads), 0, s, buf, data_start, line_end, nm, mline, pos,
                       chrom_len, fixed, cells, n_samples, block_size, check, start, flip);
    return hipGetLastError();
}

hipError_t launch_hx_blocks(uint64_t nm, const uint64_t *mline, const uint32_t *start, const uint64_t *bnum,
                            const uint32_t *flip, uint64_t *first, uint64_t *last, uint64_t *lblock, uint32_t *lflip,
                            hipStream_t s) {
    if (!nm) return hipSuccess;
    hipLaunchKernelGGL(k_hx_blocks, dim3(hx_grid(nm, kHxThreads)), dim3(kHxThreads), 0, s, nm, mline, start, bnum, flip, first,
                       last, lblock, lflip);
    return hipGetLastError();
}

hipError_t launch_hx_layout(uint64_t nm, uint64_t nb, uint32_t n_samples, const uint64_t *mline, const uint32_t *start,
                            const uint64_t *bnum, const uint32_t *fixed, const uint64_t *cells, const uint64_t *first,
                            const uint64_t *last,
                            const int64_t *pos, const uint32_t *chrom_len, uint64_t *agg, uint32_t *tstart, uint64_t *carry,
                            uint64_t *base, uint32_t *head, uint64_t *row_len, int64_t *bstart, int64_t *bend,
                            hipStream_t s) {
    if (!nm) return hipSuccess;
    if (!hx_grid_ok(nm, n_samples) || nb >= (1ull << 33)) return hipErrorInvalidValue;
    const dim3 tiles((unsigned)hx_tiles(nm), (n_samples + kHxTileSamples - 1) / kHxTileSamples);
    hipLaunchKernelGGL(k_hx_tile<false>, tiles, dim3(kWave), 0, s, nm, n_samples, mline, start, bnum, fixed, cells, nullptr, agg, tstart);
    hipLaunchKernelGGL(k_hx_carry, dim3(hx_grid(n_samples, kHxThreads)), dim3(kHxThreads), 0, s, hx_tiles(nm), n_samples, agg,
                       tstart, carry);
    hipLaunchKernelGGL(k_hx_tile<true>, tiles, dim3(kWave), 0, s, nm, n_samples, mline, start, bnum, fixed, cells, carry, base, nullptr);
    hipLaunchKernelGGL(k_hx_rows, dim3(hx_grid(nb, kHxWaves)), dim3(kHxThreads), 0, s, nb, n_samples, first, last, mline, pos,
                       chrom_len, base, head, row_len, bstart, bend);
    return hipGetLastError();
}

hipError_t launch_hx_heads(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t nb, const uint64_t *first,
                           const uint64_t *mline, const uint32_t *chrom_len, const int64_t *bstart, const int64_t *bend,
                           const uint64_t *row_off, const uint64_t *row_len, char *text, hipStream_t s) {
    if (!nb) return hipSuccess;
    hipLaunchKernelGGL(k_hx_heads, dim3(hx_grid(nb, kHxThreads)), dim3(kHxThreads), 0, s, buf, data_start, line_end, nb, first,
                       mline, chrom_len, bstart, bend, row_off, row_len, text);
    return hipGetLastError();
}

hipError_t launch_hx_emit(const char *buf, int64_t data_start, const uint64_t *line_end, uint64_t nm, uint32_t n_samples,
                          const uint64_t *mline, const uint32_t *start, const uint64_t *bnum, const uint32_t *fixed,
                          const uint64_t *cells, const uint64_t *carry, const uint64_t *base, const uint32_t *head,
                          const uint64_t *row_off, char *text, hipStream_t s) {
    if (!nm) return hipSuccess;
    if (!hx_grid_ok(nm, n_samples)) return hipErrorInvalidValue;
    const dim3 tiles((unsigned)hx_tiles(nm), (n_samples + kHxTileSamples - 1) / kHxTileSamples);
    hipLaunchKernelGGL(k_hx_emit, tiles, dim3(kHxThreads), 0, s, buf, data_start, line_end, nm, n_samples, mline, start, bnum,
                       fixed, cells, carry, base, head, row_off, text);
    return hipGetLastError();
}

}  // namespace vcfxg
