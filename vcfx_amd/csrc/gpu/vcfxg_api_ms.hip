// vcfxg_api_ms.hip -- VCFX_multiallelic_splitter over a block of indexed lines (the C ABI of
// include/vcfx_gpu.h): scan, row numbering, the cut at the byte budget, row lengths, their scan,
// the rows, each line's text range (two host synchronisations for the row count and the text size)
#include "vcfxg_ctx.h"

using namespace vcfxg;

static_assert(kMsEmpty == VCFXG_MS_EMPTY && kMsCopy == VCFXG_MS_COPY && kMsSplit == VCFXG_MS_SPLIT &&
                  kMsHeader == VCFXG_MS_HEADER && kMsOther == VCFXG_MS_NUM_OTHER && kMsA == VCFXG_MS_NUM_A &&
                  kMsR == VCFXG_MS_NUM_R && kMsG == VCFXG_MS_NUM_G && kMsInfo == VCFXG_MS_INFO &&
                  kMsFormat == VCFXG_MS_FORMAT && kMsKeysLds == VCFXG_MS_KEYS_LDS && kMsTableLds == VCFXG_MS_TABLE_LDS,
              "multiallelic_split constants");

// The device table: one entry per ID, the last declaration's (section, class), and only the
// classes that recode (an ID whose last declaration is any other number is as good as absent).
// words: entries x {ID offset in bytes, ID length, section << 8 | class}, then the ID bytes.
static uint32_t ms_build_table(const vcfxg_ms_params *p, std::vector<uint32_t> &words) {
    std::map<std::string, uint32_t> last;
    for (uint64_t i = 0; i < p->n_entries; i++) {
        const vcfxg_ms_entry &e = p->table[i];
        last[std::string(e.id ? e.id : "", e.id_len)] = ((uint32_t)e.section << 8) | e.number;
    }
    for (auto it = last.begin(); it != last.end();)
        it = (it->second & 0xFFu) == VCFXG_MS_NUM_OTHER ? last.erase(it) : std::next(it);
    const uint32_t ne = (uint32_t)last.size();
    size_t bytes = 12 * (size_t)ne;
    for (const auto &kv : last) bytes += (kv.first.size() + 3) / 4 * 4;
    words.assign(bytes / 4 + 1, 0u);
    uint32_t off = 12 * ne, k = 0;
    for (const auto &kv : last) {
        words[3 * k] = off;
        words[3 * k + 1] = (uint32_t)kv.first.size();
        words[3 * k + 2] = kv.second;
        std::memcpy(reinterpret_cast<char *>(words.data()) + off, kv.first.data(), kv.first.size());
        off += (uint32_t)((kv.first.size() + 3) / 4 * 4);
        k++;
    }
    return ne;
}

extern "C" {

int vcfxg_multiallelic_split(vcfxg_ctx *c, uint64_t l0, uint64_t l1, const vcfxg_ms_params *p, vcfxg_summary *out) {
    if (!c || !p || (p->n_entries && !p->table) || p->n_entries >= (1ull << 24) ||
        (p->mode != VCFXG_MODE_FILE && p->mode != VCFXG_MODE_STDIN))
        return VCFXG_E_ARG;
    for (uint64_t i = 0; i < p->n_entries; i++)
        if (p->table[i].section > VCFXG_MS_FORMAT || p->table[i].number > VCFXG_MS_NUM_G ||
            (p->table[i].id_len && !p->table[i].id))
            return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    if (l0 > l1 || l1 > c->n_lines) return VCFXG_E_ARG;
    l1 = std::min(l1, l0 + c->ms_block);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n = l1 - l0, L = c->n_lines;
    c->text_bytes = 0;
    c->ms_done = {};
    if (out) std::memset(out, 0, sizeof *out);
    if (!n) return VCFXG_OK;
    const uint32_t ne = ms_build_table(p, c->ms_tab_host);
    const size_t tb = 4 * (c->ms_tab_host.size() - 1);
    if (tb >= (1ull << 31)) return VCFXG_E_ARG;
    int r = ensure(c, c->ms_tab, tb + 4);
    if (!r) r = af_buffers(c, L, StatusOwner::other);
    if (!r) r = ensure(c, c->ms_geom, 4 * (size_t)kMsGeom * n);
    if (!r) r = ensure(c, c->ms_cost, 8 * (n + 1));
    if (!r) r = ensure(c, c->ms_costoff, 8 * (n + 1));
    if (!r) r = ensure(c, c->ms_rowbase, 8 * (n + 1));
    if (!r) r = ensure(c, c->ms_lineoff, 8 * (n + 1));
    if (!r) r = ensure(c, c->ms_small, 16);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(c->ms_tab.p, c->ms_tab_host.data(), tb + 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->ms_cost) + n, 0, 8, c->stream));
    const char *buf = P<char>(c->input);
    const uint64_t *le = P<uint64_t>(c->line_end);
    const int stdin_mode = p->mode == VCFXG_MODE_STDIN;
    prof_begin(c, "ms_scan");
    HIPCHK(c, launch_ms_scan(buf, (int64_t)c->data_start, le, l0, n, stdin_mode, P<uint8_t>(c->status), P<int32_t>(c->alt),
                             P<uint32_t>(c->ms_geom), P<uint64_t>(c->ms_cost), c->stream));
    prof_end(c, "ms_scan");
    prof_begin(c, "ms_number");
    r = exclusive_scan(c, P<uint32_t>(c->alt) + l0, P<uint64_t>(c->ms_rowbase), (size_t)n + 1);
    if (!r) r = exclusive_scan(c, P<uint64_t>(c->ms_cost), P<uint64_t>(c->ms_costoff), (size_t)n + 1);
    if (r) return r;
    HIPCHK(c, launch_ms_cut(P<uint64_t>(c->ms_costoff), P<uint64_t>(c->ms_rowbase), n, c->ms_bytes,
                            P<uint64_t>(c->ms_small), c->stream));
    prof_end(c, "ms_number");
    static thread_local uint64_t tail[5];
    HIPCHK(c, hipMemcpyAsync(&tail[0], c->ms_small.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t taken = tail[0], rows = tail[1];
    r = ensure(c, c->rowlen, 8 * (rows + 1));
    if (!r) r = ensure(c, c->rowoff, 8 * (rows + 1));
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->rowlen) + rows, 0, 8, c->stream));
    prof_begin(c, "ms_len");
    HIPCHK(c, launch_ms_len(buf, (int64_t)c->data_start, le, l0, taken, stdin_mode, P<uint32_t>(c->ms_tab), (uint32_t)tb, ne,
                            rows, P<uint64_t>(c->ms_rowbase), P<int32_t>(c->alt), P<uint32_t>(c->ms_geom),
                            P<uint64_t>(c->rowlen), P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "ms_len");
    prof_begin(c, "ms_offsets");
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)rows + 1);
    prof_end(c, "ms_offsets");
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(&tail[2], P<uint64_t>(c->rowoff) + rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t text = tail[2];
    r = ensure(c, c->text, text + 16);
    if (r) return r;
    prof_begin(c, "ms_write");
    HIPCHK(c, launch_ms_write(buf, (int64_t)c->data_start, le, l0, taken, stdin_mode, P<uint32_t>(c->ms_tab), (uint32_t)tb,
                              ne, rows, P<uint64_t>(c->ms_rowbase), P<int32_t>(c->alt), P<uint32_t>(c->ms_geom),
                              P<uint64_t>(c->rowoff), P<char>(c->text), c->stream));
    prof_end(c, "ms_write");
    HIPCHK(c, launch_ms_ranges(l0, taken, P<uint8_t>(c->status), P<uint64_t>(c->ms_rowbase), P<uint64_t>(c->rowoff),
                               P<uint64_t>(c->ms_lineoff), P<unsigned long long>(c->counters), c->stream));
    HIPCHK(c, hipMemcpyAsync(&tail[3], c->counters.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = text;
    c->ms_l0 = l0;
    c->ms_n = taken;
    mark_done(c, c->ms_done);
    if (out) {
        out->n_lines = taken;
        out->rows = rows;
        out->data_lines = tail[3];
        out->general_records = tail[4];
        out->text_bytes = text;
    }
    return VCFXG_OK;
}

int vcfxg_ms_line_ranges(vcfxg_ctx *c, uint64_t first, uint64_t count, uint64_t *off) {
    if (!c || !off) return VCFXG_E_ARG;
    if (!c->indexed || !is_done(c, c->ms_done)) return VCFXG_E_STATE;
    if (first < c->ms_l0 || first + count > c->ms_l0 + c->ms_n) return VCFXG_E_ARG;
    HIPCHK(c, hipMemcpyAsync(off, P<uint64_t>(c->ms_lineoff) + (first - c->ms_l0), 8 * (count + 1), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

}  // extern "C"
