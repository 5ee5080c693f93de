// vcfxg_api_fx.hip -- VCFX_field_extractor over the indexed lines (the C ABI of include/vcfx_gpu.h):
// the table (no host synchronisation beyond its upload), the scan (one: the rows and the text's
// size), the rows' text (none before the caller fetches it)
#include <unordered_map>

#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(kFxEmpty == VCFXG_FX_EMPTY && kFxHeader == VCFXG_FX_HEADER && kFxRow == VCFXG_FX_ROW && kFxStd == VCFXG_FX_STD &&
                  kFxInfo == VCFXG_FX_INFO && kFxSample == VCFXG_FX_SAMPLE && kFxNone == VCFXG_FX_NONE &&
                  kFxDot == VCFXG_FX_DOT && kFxOne == VCFXG_FX_ONE && kFxTableLds == VCFXG_FX_TABLE_LDS &&
                  kFxTileRows == VCFXG_FX_TILE_ROWS && kFxStage == VCFXG_FX_STAGE && VCFXG_FX_CELL_BYTES == 8,
              "field_extractor constants");

template <typename T>
static int fx_fetch(vcfxg_ctx *c, DevBuf &b, uint64_t first, uint64_t count, T *host) {
    if (host && count)
        HIPCHK(c, hipMemcpyAsync(host, P<T>(b) + first, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream));
    return VCFXG_OK;
}

extern "C" {

// The table's words (vcfxg_kernels.h) built from the columns and uploaded.
int vcfxg_fields_load(vcfxg_ctx *c, const vcfxg_fx_col *cols, uint32_t n, const char *pool, uint32_t pool_bytes, int mode) {
    if (!c || !cols || !n || n >= (1u << 28) || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (pool_bytes && !pool) return VCFXG_E_ARG;
    const bool stdin_mode = mode == VCFXG_MODE_STDIN;
    auto in_pool = [&](uint32_t off, uint32_t len) { return off <= pool_bytes && len <= pool_bytes - off; };
    uint32_t lastk = 0;
    std::vector<uint32_t> keys, subs, samp, scol;
    std::unordered_map<std::string, uint32_t> sub_id;
    for (uint32_t i = 0; i < n; i++) {
        const vcfxg_fx_col &f = cols[i];
        if (f.kind > VCFXG_FX_NONE) return VCFXG_E_ARG;
        if (f.kind == VCFXG_FX_STD) {
            if (f.col > 7) return VCFXG_E_ARG;
            lastk = std::max(lastk, f.col);
        }
        const bool keyed = f.kind == VCFXG_FX_INFO || (f.kind == VCFXG_FX_SAMPLE && stdin_mode && f.key_len != VCFXG_FX_NOKEY);
        if (keyed) {
            if (f.key_len == VCFXG_FX_NOKEY || !in_pool(f.key_off, f.key_len)) return VCFXG_E_ARG;
            keys.insert(keys.end(), {f.key_off, f.key_len, i});
            lastk = std::max(lastk, 7u);
        }
        if (f.kind == VCFXG_FX_SAMPLE) {
            if ((f.col && f.col < 9) || f.col > 0x7FFFFFFFu || !in_pool(f.sub_off, f.sub_len)) return VCFXG_E_ARG;
            const auto it = sub_id.emplace(std::string(pool + f.sub_off, f.sub_len), (uint32_t)sub_id.size());
            if (it.second) subs.insert(subs.end(), {f.sub_off, f.sub_len});
            samp.insert(samp.end(), {i, f.col, 0u, it.first->second | (f.named ? 1u << 31 : 0u)});
            if (f.col) {
                scol.push_back(f.col);
                lastk = std::max(lastk, f.col);
            }
        }
    }
    std::sort(scol.begin(), scol.end());
    scol.erase(std::unique(scol.begin(), scol.end()), scol.end());
    const uint32_t nsc = (uint32_t)scol.size(), nwords = nsc ? scol.back() / 32u + 1u : 0u;
    for (size_t i = 0; i < samp.size(); i += 4)
        if (samp[i + 1]) samp[i + 2] = (uint32_t)(std::lower_bound(scol.begin(), scol.end(), samp[i + 1]) - scol.begin());
    const uint64_t total = (uint64_t)kFxHWords + 2ull * n + keys.size() + subs.size() + samp.size() + (nwords + 2ull) +
                           (nwords + 1ull) + (pool_bytes + 3ull) / 4 + 1;
    if (total >= (1ull << 31)) return VCFXG_E_NOMEM;
    std::vector<uint32_t> &T = c->fx_tab_host;  // (the source of the asynchronous copy)
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (an earlier load's copy has left it)
    T.assign((size_t)total, 0u);
    uint32_t o = kFxHWords;
    T[kFxHNcols] = n, T[kFxHNkeys] = (uint32_t)(keys.size() / 3), T[kFxHNsub] = (uint32_t)(subs.size() / 2);
    T[kFxHNsamp] = (uint32_t)(samp.size() / 4), T[kFxHNsc] = nsc, T[kFxHLastk] = lastk, T[kFxHNwords] = nwords;
    T[kFxHStdin] = stdin_mode ? 1u : 0u;
    T[kFxHCols] = o;
    for (uint32_t i = 0; i < n; i++) T[o + 2 * i] = cols[i].kind, T[o + 2 * i + 1] = cols[i].kind == VCFXG_FX_STD ? cols[i].col : 0u;
    o += 2 * n;
    T[kFxHKeys] = o;
    std::copy(keys.begin(), keys.end(), T.begin() + o);
    o += (uint32_t)keys.size();
    T[kFxHSubs] = o;
    std::copy(subs.begin(), subs.end(), T.begin() + o);
    o += (uint32_t)subs.size();
    T[kFxHSamp] = o;
    std::copy(samp.begin(), samp.end(), T.begin() + o);
    o += (uint32_t)samp.size();
    T[kFxHMask] = o;
    for (uint32_t col : scol) T[o + col / 32u] |= 1u << (col & 31u);
    T[kFxHRank] = o + nwords + 2;
    for (uint32_t w = 0, r = 0; w <= nwords; w++) {
        T[o + nwords + 2 + w] = r;
        r += (uint32_t)__builtin_popcount(T[o + w]);
    }
    o += 2 * nwords + 3;
    T[kFxHPool] = o;
    if (pool_bytes) std::memcpy(&T[o], pool, pool_bytes);
    T[kFxHTotal] = (uint32_t)total;
    c->fx_loaded = false;
    c->fx_scanned = {};
    const int r = ensure(c, c->fx_tab, 4 * (size_t)total);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(c->fx_tab.p, T.data(), 4 * (size_t)total, hipMemcpyHostToDevice, c->stream));
    c->fx_ncols = n;
    c->fx_nsc = nsc;
    c->fx_nsub = (uint32_t)(subs.size() / 2);
    c->fx_loaded = true;
    return VCFXG_OK;
}

// The cell pass over every indexed line, the two scans: ONE host synchronisation.
int vcfxg_fields_scan(vcfxg_ctx *c, uint64_t names_from, vcfxg_summary *out) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed || !c->fx_loaded) return VCFXG_E_STATE;
    if (c->n_lines >= (1ull << 31)) return VCFXG_E_ARG;  // (the kernels hold line numbers in 32 bits)
    DENSE(c);
    HIPCHK(c, hipSetDevice(c->device));
    c->fx_scanned = {};
    c->fx_rows = c->fx_text = 0;
    if (out) std::memset(out, 0, sizeof *out);
    const uint64_t n = c->n_lines, nc = c->fx_ncols;
    const uint32_t words = c->fx_tab_host[kFxHTotal];
    if (n) {
        if (n > (~0ull / 8) / nc) return VCFXG_E_NOMEM;
        int r = ensure(c, c->fx_status, n + 1);
        if (!r) r = ensure(c, c->fx_isrow, 4 * (n + 1));
        if (!r) r = ensure(c, c->fx_rownum, 8 * (n + 1));
        if (!r) r = ensure(c, c->fx_rowlen, 8 * (n + 1));
        if (!r) r = ensure(c, c->fx_rowoff, 8 * (n + 1));
        if (!r) r = ensure(c, c->fx_cells, 8 * n * nc);
        if (!r) r = ensure(c, c->fx_span, 8 * n * std::max<uint64_t>(c->fx_nsc, 1));
        if (!r) r = ensure(c, c->fx_out, sizeof(FxOut));
        if (!r) r = ensure(c, c->fx_sub, 4 * n * std::max<uint64_t>(c->fx_nsub, 1));
        if (r) return r;
        HIPCHK(c, hipMemsetAsync(P<uint32_t>(c->fx_isrow) + n, 0, 4, c->stream));
        HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->fx_rowlen) + n, 0, 8, c->stream));
        prof_begin(c, "fx_cells");
        FxOut &O = c->fx_out_host;  // (the source of an asynchronous copy: it lives with the context)
        O = FxOut{P<uint8_t>(c->fx_status), P<uint32_t>(c->fx_isrow), P<uint64_t>(c->fx_rowlen), P<uint32_t>(c->fx_cells),
                  P<uint32_t>(c->fx_span),  P<uint32_t>(c->fx_sub),   names_from,
                  P<uint64_t>(c->line_end), (int64_t)c->data_start};
        HIPCHK(c, hipMemcpyAsync(c->fx_out.p, &O, sizeof O, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_fx_cells(P<char>(c->input), n, P<uint32_t>(c->fx_tab),
                                  words, P<FxOut>(c->fx_out), c->stream));
        prof_end(c, "fx_cells");
        prof_begin(c, "fx_number");
        r = exclusive_scan(c, P<uint32_t>(c->fx_isrow), P<uint64_t>(c->fx_rownum), (size_t)n + 1);
        if (!r) r = exclusive_scan(c, P<uint64_t>(c->fx_rowlen), P<uint64_t>(c->fx_rowoff), (size_t)n + 1);
        prof_end(c, "fx_number");
        if (r) return r;
        uint64_t *tail = c->fx_tail;  // (the destination of asynchronous copies)
        HIPCHK(c, hipMemcpyAsync(&tail[0], P<uint64_t>(c->fx_rownum) + n, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&tail[1], P<uint64_t>(c->fx_rowoff) + n, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->fx_rows = tail[0];
        c->fx_text = tail[1];
        prof_collect(c);
    }
    mark_done(c, c->fx_scanned);
    if (out) {
        out->n_lines = n;
        out->rows = out->data_lines = c->fx_rows;
        out->text_bytes = c->fx_text;
        out->general_records = fx_table_in_lds(words) ? 0 : 1;
    }
    return VCFXG_OK;
}

int vcfxg_fields_lines(vcfxg_ctx *c, uint64_t first, uint64_t count, uint8_t *status, uint64_t *row, uint64_t *row_off) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->fx_scanned)) return VCFXG_E_STATE;
    if (first > c->n_lines || count > c->n_lines - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    int r = fx_fetch(c, c->fx_status, first, count, status);
    if (!r) r = fx_fetch(c, c->fx_rownum, first, count, row);
    if (!r) r = fx_fetch(c, c->fx_rowoff, first, count, row_off);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_fields_cells(vcfxg_ctx *c, uint64_t first, uint64_t count, uint32_t *cells) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->fx_scanned)) return VCFXG_E_STATE;
    if (first > c->n_lines || count > c->n_lines - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    if (!cells) return VCFXG_E_ARG;
    const int r = fx_fetch(c, c->fx_cells, first * c->fx_ncols * 2, count * c->fx_ncols * 2, cells);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_fields_text(vcfxg_ctx *c, vcfxg_summary *out) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->fx_scanned)) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    if (out) std::memset(out, 0, sizeof *out);
    const int r = ensure(c, c->text, c->fx_text + 16);
    if (r) return r;
    c->text_bytes = c->fx_text;
    if (c->fx_text) {
        prof_begin(c, "fx_write");
        HIPCHK(c, launch_fx_write(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end), c->n_lines, c->fx_ncols,
                                  P<uint8_t>(c->fx_status), P<uint64_t>(c->fx_rowoff), P<uint32_t>(c->fx_cells),
                                  P<char>(c->text), c->stream));
        prof_end(c, "fx_write");
        prof_collect(c);
    }
    if (out) {
        out->n_lines = c->n_lines;
        out->rows = out->data_lines = c->fx_rows;
        out->text_bytes = c->fx_text;
    }
    return VCFXG_OK;
}

}  // extern "C"
