// vcfxg_api_lines.hip -- the tools over ranges of indexed lines: VCFX_allele_counter and
// VCFX_sample_extractor (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"

using namespace vcfxg;

extern "C" {

// VCFX_allele_counter over indexed lines [l0, l1): row bytes, a scan, the rows (one host
// synchronisation for the text size)
int vcfxg_allele_counter(vcfxg_ctx *c, uint64_t l0, uint64_t l1, const vcfxg_ac_params *p, vcfxg_summary *out) {
    if (!c || !p || (p->m && (!p->sample || !p->name_off)) || p->kind < 0 || p->kind > 2 || p->m >= (1ull << 31))
        return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    if (l0 > l1 || l1 > c->n_lines) return VCFXG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t m = p->m, n = l1 - l0, L = c->n_lines;
    // slot i reads eff[i]: the selection itself, or (seq) its running maximum
    c->ac_eff_host.resize(m + 1);
    c->ac_noff_host.assign(p->name_off, p->name_off + m + 1);
    uint32_t run = 0, mx = 0;
    for (uint64_t i = 0; i < m; i++) {
        run = p->seq ? std::max(run, p->sample[i]) : p->sample[i];
        c->ac_eff_host[i] = run;
        mx = std::max(mx, run);
    }
    const uint64_t nb = p->name_off[m] - p->name_off[0];
    if (p->name_off[0] != 0) return VCFXG_E_ARG;
    c->ac_names_host.assign(p->names ? p->names : "", (size_t)nb);
    const uint64_t scap = (uint64_t)mx + 1;
    // the selection in k_ac_fmt's LDS when it fits in 40 KiB (the sample indices, 32-bit name
    // offsets and the names); VCFXG_AC_SEL_GLOBAL=1 keeps it in global memory (test hook)
    // an identity selection (slot i reads sample i: every sample, in order) keeps no index array
    bool ident = true;
    for (uint64_t i = 0; i < m && ident; i++) ident = c->ac_eff_host[i] == i;
    const uint64_t sel_bytes = (((ident ? 0 : 4 * m) + 4 * (m + 1) + (p->name_off[m] - p->name_off[0]) + 15) / 16) * 16;
    const uint32_t sel_lds = sel_bytes <= 40960 && !getenv("VCFXG_AC_SEL_GLOBAL") ? (uint32_t)sel_bytes : 0u;
    // text rows under a selection whose names share one length L <= 11: k_ac_rows writes the
    // fixed-stride records straight from registers (vcfxg_ac.hip); VCFXG_AC_DIRECT=0 keeps every
    // record on k_ac_fmt's LDS image (A/B and test hook)
    static const bool direct_env = [] {
        const char *e = getenv("VCFXG_AC_DIRECT");
        return !(e && e[0] == '0');
    }();
    const uint64_t L0 = m ? p->name_off[1] - p->name_off[0] : 0;
    bool direct = direct_env && p->kind == 0 && m > 0 && m <= 4096 && L0 <= 11 &&
                  vcfxg::ac_rows_lds((uint32_t)m, ident ? 1 : 0) <= vcfxg::ac_rows_lds_max();
    for (uint64_t i = 0; i < m && direct; i++) direct = p->name_off[i + 1] - p->name_off[i] == L0;
    if (direct) {
        c->ac_etab_host.assign(16 * m, 0);
        for (uint64_t i = 0; i < m; i++) {
            uint8_t *e = &c->ac_etab_host[16 * i];
            std::memcpy(e + 11 - L0, c->ac_names_host.data() + p->name_off[i], (size_t)L0);
            std::memcpy(e + 11, "\t0\t0\n", 5);
        }
    }
    // grid: a wave per line up to 2048 blocks, and at most 1 GiB of per-wave sample tables
    const uint64_t waves_per_block = (uint64_t)(vcfxg::ac_threads() / 64);
    uint64_t blocks = std::min<uint64_t>((n + waves_per_block - 1) / waves_per_block, 2048);
    blocks = std::max<uint64_t>(1, std::min<uint64_t>(blocks, (1ull << 30) / (4 * scap * waves_per_block)));
    int r = ensure(c, c->ac_eff, 4 * (m + 1));
    if (!r) r = ensure(c, c->ac_noff, 8 * (m + 1));
    if (!r) r = ensure(c, c->ac_names, nb + 1);
    if (!r) r = ensure(c, c->ac_scratch, 4 * scap * waves_per_block * blocks);
    if (!r && direct) {
        // the entries and k_ac_nib's counts for k_ac_rows (n x ceil(m / 64) x 32 B); without room
        // for them every record takes k_ac_fmt
        int rd = ensure(c, c->ac_etab, 16 * m);
        if (!rd) rd = ensure(c, c->ac_nib, n * ((m + 63) / 64) * 32);
        if (rd == VCFXG_E_NOMEM) {
            (void)hipGetLastError();  // (a failed hipMalloc leaves its error to be read once)
            c->err.clear();
            direct = false;
        } else
            r = rd;
    }
    if (!r) r = af_buffers(c, L, StatusOwner::other);
    if (!r) r = ensure(c, c->af_meta, vcfxg::ac_meta_bytes() * (L + 1));
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(c->ac_eff.p, c->ac_eff_host.data(), 4 * (m + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ac_noff.p, c->ac_noff_host.data(), 8 * (m + 1), hipMemcpyHostToDevice, c->stream));
    if (nb) HIPCHK(c, hipMemcpyAsync(c->ac_names.p, c->ac_names_host.data(), nb, hipMemcpyHostToDevice, c->stream));
    if (direct)
        HIPCHK(c, hipMemcpyAsync(c->ac_etab.p, c->ac_etab_host.data(), 16 * m, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->rowlen) + n, 0, 8, c->stream));
    const char *buf = P<char>(c->input);
    prof_begin(c, "ac_len");
    HIPCHK(c, vcfxg::launch_ac_len(buf, (int64_t)c->data_start, P<uint64_t>(c->line_end), l0, l1, (unsigned)blocks,
                                   P<uint32_t>(c->ac_eff), P<uint64_t>(c->ac_noff), P<char>(c->ac_names),
                                   P<uint32_t>(c->ac_scratch), (uint32_t)m, (uint32_t)scap, p->seq, p->kind,
                                   ident ? 1 : 0, direct ? 1 : 0, direct ? P<uint32_t>(c->ac_nib) : nullptr,
                                   P<uint8_t>(c->status), P<uint64_t>(c->rowlen), c->af_meta.p,
                                   P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "ac_len");
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)n + 1);
    if (r) return r;
    static thread_local uint64_t tail[6];
    HIPCHK(c, hipMemcpyAsync(&tail[0], P<uint64_t>(c->rowoff) + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&tail[1], c->counters.p, 40, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t text = tail[0];
    r = ensure(c, c->text, text + 1);
    if (r) return r;
    prof_begin(c, "ac_fmt");
    if (direct) {
        const uint64_t rw = (uint64_t)(vcfxg::ac_rows_threads() / 64);
        const unsigned rb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + rw - 1) / rw, 1024));
        HIPCHK(c, vcfxg::launch_ac_rows(buf, (int64_t)c->data_start, P<uint64_t>(c->line_end), l0, l1, rb,
                                        P<uint32_t>(c->ac_eff), (uint32_t)m, ident ? 1 : 0, c->ac_etab.p, (uint32_t)L0,
                                        P<uint32_t>(c->ac_nib), c->af_meta.p, P<uint64_t>(c->rowoff), P<char>(c->text),
                                        c->stream));
    }
    if (!direct || tail[5])  // (the records k_ac_rows does not take)
        HIPCHK(c, vcfxg::launch_ac_fmt(buf, (int64_t)c->data_start, P<uint64_t>(c->line_end), l0, l1, (unsigned)blocks,
                                       P<uint32_t>(c->ac_eff), P<uint64_t>(c->ac_noff), P<char>(c->ac_names),
                                       P<uint32_t>(c->ac_scratch), (uint32_t)m, (uint32_t)scap, p->seq, p->kind, sel_lds,
                                       ident ? 1 : 0, direct ? 1 : 0, P<uint8_t>(c->status), c->af_meta.p,
                                       P<uint64_t>(c->rowoff), P<char>(c->text), c->stream));
    prof_end(c, "ac_fmt");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = text;
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = n;
        out->rows = tail[1];
        out->data_lines = tail[2];
        out->warn_lines = tail[3];
        out->general_records = tail[4];
        out->text_bytes = text;
    }
    return VCFXG_OK;
}

static_assert(vcfxg::kSxEmpty == VCFXG_SX_EMPTY && vcfxg::kSxRow == VCFXG_SX_ROW && vcfxg::kSxShort == VCFXG_SX_SHORT &&
                  vcfxg::kSxHeader == VCFXG_SX_HEADER && vcfxg::kSxNoSample == VCFXG_SX_NO_SAMPLES &&
                  vcfxg::kSxPre == VCFXG_SX_PRE && vcfxg::kSxChrom == VCFXG_SX_CHROM,
              "sample_extract line statuses");
// VCFX_sample_extractor over indexed lines [l0, min(l1, l0 + sx_block)): statuses and output bytes,
// a scan, the bytes (one host synchronisation for the text size)
int vcfxg_sample_extract(vcfxg_ctx *c, uint64_t l0, uint64_t l1, const vcfxg_sx_params *p, vcfxg_summary *out) {
    if (!c || !p || (p->m && !p->cols) || p->m >= (1ull << 31) ||
        (p->mode != VCFXG_MODE_FILE && p->mode != VCFXG_MODE_STDIN))
        return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    if (l0 > l1 || l1 > c->n_lines) return VCFXG_E_ARG;
    l1 = std::min(l1, l0 + c->sx_block);
    for (uint64_t i = 0; i < p->m; i++)  // field numbers past FORMAT, ascending
        if (p->cols[i] < 9 || p->cols[i] >= (1u << 31) || (i && p->cols[i] <= p->cols[i - 1])) return VCFXG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n = l1 - l0, L = c->n_lines;
    const uint32_t m = (uint32_t)p->m, lastk = m ? p->cols[m - 1] : 8u, nwords = lastk / 32u + 1u;
    c->sx_mask_host.assign((size_t)nwords + 2, 0u);
    c->sx_mask_host[0] = 0x1FFu;
    for (uint32_t i = 0; i < m; i++) c->sx_mask_host[p->cols[i] >> 5] |= 1u << (p->cols[i] & 31u);
    int r = ensure(c, c->sx_mask, 4 * ((size_t)nwords + 2));
    if (!r) r = af_buffers(c, L, StatusOwner::other);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(c->sx_mask.p, c->sx_mask_host.data(), 4 * ((size_t)nwords + 2), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->rowlen) + n, 0, 8, c->stream));
    const uint64_t wpb = (uint64_t)(vcfxg::sx_threads() / 64);
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + wpb - 1) / wpb, 8192));
    const char *buf = P<char>(c->input);
    const int stdin_mode = p->mode == VCFXG_MODE_STDIN, seen = p->seen_chrom ? 1 : 0;
    prof_begin(c, "sx_len");
    HIPCHK(c, vcfxg::launch_sx_len(buf, (int64_t)c->data_start, P<uint64_t>(c->line_end), l0, l1, blocks,
                                   P<uint32_t>(c->sx_mask), nwords, lastk, m, stdin_mode, seen, P<uint8_t>(c->status),
                                   P<uint64_t>(c->rowlen), P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "sx_len");
    prof_begin(c, "sx_scan");
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)n + 1);
    prof_end(c, "sx_scan");
    if (r) return r;
    static thread_local uint64_t tail[5];
    HIPCHK(c, hipMemcpyAsync(&tail[0], P<uint64_t>(c->rowoff) + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&tail[1], c->counters.p, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t text = n ? tail[0] : 0;
    c->text_bytes = 0;
    r = ensure(c, c->text, text + 16);
    if (r) return r;
    prof_begin(c, "sx_write");
    HIPCHK(c, vcfxg::launch_sx_write(buf, (int64_t)c->data_start, P<uint64_t>(c->line_end), l0, l1, blocks,
                                     P<uint32_t>(c->sx_mask), nwords, lastk, m, stdin_mode, seen, P<uint8_t>(c->status),
                                     P<uint64_t>(c->rowoff), P<char>(c->text), c->stream));
    prof_end(c, "sx_write");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = text;
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = n;
        if (n) {
            out->rows = tail[1];
            out->data_lines = tail[2];
            out->warn_lines = tail[3] + tail[4];
        }
        out->text_bytes = text;
    }
    return VCFXG_OK;
}

}  // extern "C"
