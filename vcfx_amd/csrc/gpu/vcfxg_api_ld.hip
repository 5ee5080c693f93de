// vcfxg_api_ld.hip -- VCFX_ld_calculator: the prepare paths (indexed and walk), the streaming
// pair pass and the matrix (the C ABI of include/vcfx_gpu.h)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "vcfxg_ctx.h"
#include "vcfxg_ld.h"

using namespace vcfxg;

extern "C" {

struct U16ToU64 {
    __host__ __device__ uint64_t operator()(const uint16_t &x) const { return x; }
};

// the shared tail of the LD prepare paths: M variants with ld_vars / ld_fast / ld_Gp, the
// prefix offsets ld_poff (pbytes in all) and the per-group flags ld_gflag_host in place (and
// ld_Gc when ld_gc_ready): the sparse-missing / masked planes the groups need, the prefixes
static int ld_prepare_finish(vcfxg_ctx *c, uint64_t M, int n_samples, int kpad, int kp4, int id_dot_to_pos,
                             uint64_t pbytes, bool sync_end, uint64_t *n_variants) {
    int r = VCFXG_OK;
    if (!c->ld_gc_ready) {
        for (uint64_t g = 0; g * vcfxg::kLdFastBlock < M; g++)
            if (c->ld_gflag_host[g] != 1) return VCFXG_E_STATE;  // (the walk gathers Gc for these)
    }
    r = ensure(c, c->ld_prefix, pbytes + 16);
    if (r) return r;
    // a group with a missing genotype: the valid-mask and squared-dosage planes of the
    // missing-data kernel (k_ld_mask), next to the dosage plane ld_Gp
    c->ld_vq = false;
    c->ld_sp = false;
    for (uint64_t g = 0; g * vcfxg::kLdFastBlock < M; g++) {
        c->ld_vq = c->ld_vq || c->ld_gflag_host[g] == 0;
        c->ld_sp = c->ld_sp || c->ld_gflag_host[g] == 2;
    }
    // the sparse-missing kernel's extra planes (CSR + the [sample][variant] u16 plane, about twice
    // the int8 plane) must not make an input fail that the masked kernel alone fits: when they do
    // not fit, every sparse group goes back to k_ld_mask (VCFXG_LD_SPARSE_NOMEM=1: a test hook
    // that takes this way as if the allocation had failed)
    static const bool sparse_nomem_hook = [] {
        const char *e = getenv("VCFXG_LD_SPARSE_NOMEM");
        return e && e[0] == '1';
    }();
    auto sparse_to_mask = [&]() -> int {
        (void)hipGetLastError();  // (a failed hipMalloc leaves its error to be read once)
        prof_end(c, "ld_sparse_prep");
        c->ld_sp = false;
        c->ld_vq = true;
        for (auto &f : c->ld_gflag_host)
            if (f == 2) f = 0;
        if (M)
            HIPCHK(c, hipMemcpyAsync(c->ld_gflag.p, c->ld_gflag_host.data(),
                                     (M + vcfxg::kLdFastBlock - 1) / vcfxg::kLdFastBlock, hipMemcpyHostToDevice, c->stream));
        c->err.clear();
        return VCFXG_OK;
    };
    if (c->ld_sp && sparse_nomem_hook) {
        r = sparse_to_mask();
        if (r) return r;
    }
    if (c->ld_sp) {
        // the missing samples of every variant (CSR) and the contribution plane of the
        // sparse-missing kernel (vcfxg_ld_fast.hip, kSp)
        prof_begin(c, "ld_sparse_prep");
        r = ensure(c, c->ld_moff, 8 * (M + 1));
        if (r == VCFXG_E_NOMEM) r = sparse_to_mask();
        if (r) return r;
    }
    if (c->ld_sp) {
        struct MissOf {
            int ns;
            __host__ __device__ uint64_t operator()(const vcfxg::LdVar &v) const { return (uint64_t)(ns - v.cnt); }
        };
        hipcub::TransformInputIterator<uint64_t, MissOf, const vcfxg::LdVar *> min(P<vcfxg::LdVar>(c->ld_vars),
                                                                                   MissOf{n_samples});
        size_t tmp2 = 0;
        HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, min, P<uint64_t>(c->ld_moff), (int)M + 1, c->stream));
        r = ensure(c, c->scan_tmp, tmp2);
        if (r) return r;
        // (entry M of the input is vars[M]: its cnt is written as ns below, so moff[M] = total)
        static thread_local vcfxg::LdVar pad_var;
        pad_var = vcfxg::LdVar{};
        pad_var.cnt = n_samples;
        HIPCHK(c, hipMemcpyAsync(P<vcfxg::LdVar>(c->ld_vars) + M, &pad_var, sizeof pad_var, hipMemcpyHostToDevice,
                                 c->stream));
        HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, tmp2, min, P<uint64_t>(c->ld_moff), (int)M + 1,
                                                   c->stream));
        static thread_local uint64_t entries;
        HIPCHK(c, hipMemcpyAsync(&entries, P<uint64_t>(c->ld_moff) + M, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const uint64_t mp = (M + vcfxg::kLdFastBlock - 1) / vcfxg::kLdFastBlock * vcfxg::kLdFastBlock;
        r = ensure(c, c->ld_midx, 2 * entries + 16);
        if (!r) r = ensure(c, c->ld_mvar, 4 * entries + 16);
        if (!r) r = ensure(c, c->ld_midx16, 32 * (M + 1));
        if (!r) r = ensure(c, c->ld_sprec, sizeof(vcfxg::LdSpRec) * (M + 1));
        if (!r) r = ensure(c, c->ld_gt16, 2 * (size_t)n_samples * mp + 64);
        if (r == VCFXG_E_NOMEM) r = sparse_to_mask();
        if (r) return r;
    }
    if (c->ld_sp) {
        const uint64_t mp = (M + vcfxg::kLdFastBlock - 1) / vcfxg::kLdFastBlock * vcfxg::kLdFastBlock;
        HIPCHK(c, vcfxg::launch_ld_miss_fill(P<int8_t>(c->ld_Gc), M, kpad, n_samples, P<uint64_t>(c->ld_moff),
                                             P<uint16_t>(c->ld_midx), P<uint32_t>(c->ld_mvar), P<uint16_t>(c->ld_midx16),
                                             c->stream));
        HIPCHK(c, vcfxg::launch_ld_gt16(P<int8_t>(c->ld_Gc), M, kpad, n_samples, mp, P<uint16_t>(c->ld_gt16),
                                        c->stream));
        HIPCHK(c, vcfxg::launch_ld_sprec(P<vcfxg::LdVar>(c->ld_vars), M, n_samples, P<vcfxg::LdSpRec>(c->ld_sprec),
                                         c->stream));
        c->ld_mp = mp;
        prof_end(c, "ld_sparse_prep");
    }
    if (c->ld_vq) {
        r = ensure(c, c->ld_Gv, (size_t)(M + 1) * kp4 + 64);
        if (!r) r = ensure(c, c->ld_Gq, (size_t)(M + 1) * kp4 + 64);
        if (r) return r;
        prof_begin(c, "ld_pack_vq");
        HIPCHK(c, vcfxg::launch_ld_pack_vq(P<int8_t>(c->ld_Gc), M, kpad, n_samples, P<uint8_t>(c->ld_Gv),
                                           P<uint8_t>(c->ld_Gq), kp4, c->stream));
        prof_end(c, "ld_pack_vq");
    }
    HIPCHK(c, vcfxg::launch_ld_prefix(1, P<vcfxg::LdVar>(c->ld_vars), M, P<char>(c->input), id_dot_to_pos,
                                      P<uint64_t>(c->ld_poff), P<char>(c->ld_prefix), c->stream));
    if (sync_end) HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->ld_m = M;
    c->ld_kpad = kpad;
    c->ld_kp4 = kp4;
    c->ld_ns = n_samples;
    c->ld_prefix_bytes = pbytes;
    c->ld_chrom_ids = false;
    if (n_variants) *n_variants = M;
    return VCFXG_OK;
}

int vcfxg_ld_prepare(vcfxg_ctx *c, int n_samples, int id_dot_to_pos, const char *rchrom, size_t rlen, int has_region,
                     int rstart, int rend, int parse_mode, uint64_t *n_variants) {
    if (!c || n_samples < 0 || (has_region && !rchrom && rlen)) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t L = c->n_lines;
    const int kpad = n_samples > 0 ? ((n_samples + 63) / 64) * 64 : 64;  // MFMA k-steps of 32 B
    int r = ensure(c, c->ld_G, (size_t)L * kpad + 64);
    if (!r) r = ensure(c, c->ld_lines, sizeof(vcfxg::LdLine) * (L + 1));
    if (!r) r = ensure(c, c->ld_vidx, 8 * (L + 1));
    if (!r) r = ensure(c, c->ld_valid, 4 * (L + 1));
    if (!r) r = ensure(c, c->query, rlen + 1);
    if (r) return r;
    c->query_host.assign(rchrom ? rchrom : "", rlen);
    if (rlen) {
        c->query_dev_p = nullptr;
        HIPCHK(c, hipMemcpyAsync(c->query.p, c->query_host.data(), rlen, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(c->ld_G.p, 0xFF, (size_t)L * kpad + 64, c->stream));
    vcfxg::LdParseArgs a{n_samples, kpad, has_region, rstart, rend, (int64_t)rlen, P<char>(c->query), parse_mode};
    prof_begin(c, "ld_parse");
    HIPCHK(c, vcfxg::launch_ld_parse(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end),
                                     P<uint64_t>(c->d_nlines), L, a, P<int8_t>(c->ld_G), P<vcfxg::LdLine>(c->ld_lines),
                                     c->stream));
    prof_end(c, "ld_parse");
    // compact order: exclusive scan of the valid flags (first member of LdLine)
    struct ValidOf {
        __host__ __device__ uint64_t operator()(const vcfxg::LdLine &x) const { return x.valid; }
    };
    hipcub::TransformInputIterator<uint64_t, ValidOf, const vcfxg::LdLine *> vin(P<vcfxg::LdLine>(c->ld_lines),
                                                                                 ValidOf());
    size_t tmp = 0;
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, vin, P<uint64_t>(c->ld_vidx), (int)L, c->stream));
    r = ensure(c, c->scan_tmp, tmp);
    if (r) return r;
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, tmp, vin, P<uint64_t>(c->ld_vidx), (int)L, c->stream));
    static thread_local uint64_t last[2];
    static thread_local vcfxg::LdLine lastline;
    if (L) {
        HIPCHK(c, hipMemcpyAsync(&last[0], P<uint64_t>(c->ld_vidx) + L - 1, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&lastline, P<vcfxg::LdLine>(c->ld_lines) + L - 1, sizeof lastline,
                                 hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t M = L ? last[0] + lastline.valid : 0;
    r = ensure(c, c->ld_Gc, (size_t)(M + 1) * kpad + 64);
    if (!r) r = ensure(c, c->ld_vars, sizeof(vcfxg::LdVar) * (M + 1));
    if (!r) r = ensure(c, c->ld_fast, sizeof(vcfxg::LdFast) * (M + 1));
    const int kp4 = vcfxg::ld_kp4(n_samples);
    if (!r) r = ensure(c, c->ld_Gp, (size_t)(M + 1) * kp4 + 64);
    if (!r) r = ensure(c, c->ld_gflag, M / vcfxg::kLdFastBlock + 2);
    if (!r) r = ensure(c, c->ld_plen, 8 * (M + 2));
    if (!r) r = ensure(c, c->ld_poff, 8 * (M + 2));
    if (r) return r;
    prof_begin(c, "ld_compact");
    HIPCHK(c, vcfxg::launch_ld_compact(P<vcfxg::LdLine>(c->ld_lines), P<uint64_t>(c->ld_vidx), P<uint64_t>(c->d_nlines),
                                       L, kpad, n_samples, P<int8_t>(c->ld_G), P<int8_t>(c->ld_Gc),
                                       P<vcfxg::LdVar>(c->ld_vars), P<vcfxg::LdFast>(c->ld_fast), c->stream));
    HIPCHK(c, vcfxg::launch_ld_pack4(P<int8_t>(c->ld_Gc), M, kpad, n_samples, P<uint8_t>(c->ld_Gp), kp4, c->stream));
    prof_end(c, "ld_compact");
    // VCFXG_LD_SPARSE=0: no sparse-missing groups (their tiles take k_ld_mask)
    static const bool sparse_env = [] {
        const char *e = getenv("VCFXG_LD_SPARSE");
        return !(e && e[0] == '0');
    }();
    const int sparse = sparse_env && n_samples > 0 && n_samples <= 16383 ? 1 : 0;  // (Sxy as u16 in the epilogue)
    HIPCHK(c, vcfxg::launch_ld_groups(P<vcfxg::LdVar>(c->ld_vars), M, n_samples, sparse, P<uint8_t>(c->ld_gflag),
                                      c->stream));
    c->ld_gflag_host.assign(M / vcfxg::kLdFastBlock + 1, 0);
    if (M)
        HIPCHK(c, hipMemcpyAsync(c->ld_gflag_host.data(), c->ld_gflag.p, (M + vcfxg::kLdFastBlock - 1) / vcfxg::kLdFastBlock,
                                 hipMemcpyDeviceToHost, c->stream));
    // per-variant "chrom\tpos\tid" prefixes
    HIPCHK(c, vcfxg::launch_ld_prefix(0, P<vcfxg::LdVar>(c->ld_vars), M, P<char>(c->input), id_dot_to_pos,
                                      P<uint64_t>(c->ld_plen), nullptr, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->ld_plen) + M, 0, 8, c->stream));
    r = exclusive_scan(c, P<uint64_t>(c->ld_plen), P<uint64_t>(c->ld_poff), (size_t)M + 1);
    if (r) return r;
    static thread_local uint64_t pbytes;
    HIPCHK(c, hipMemcpyAsync(&pbytes, P<uint64_t>(c->ld_poff) + M, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ld_gc_ready = true;
    return ld_prepare_finish(c, M, n_samples, kpad, kp4, id_dot_to_pos, pbytes, true, n_variants);
}

// vcfxg_index(data_start) + vcfxg_ld_prepare in one call, with the same variants, rows, sums and
// prefixes.  The default for records averaging >= 512 B with n_samples <= 4096: the LD walk
// (vcfxg_ld.hip k_ld_walk: one HBM pass over the records, no line index), then one compaction
// that writes the variant records, the FP4 rows and the prefix lengths, and ONE host
// synchronisation for the variant count, the prefix bytes and the group flags.  The int8 rows in
// variant order (ld_Gc) are gathered only when some variant misses a call (the sparse-missing and
// masked kernels read them).  A walker over its line capacity, or an input the walk does not
// take, runs vcfxg_index + vcfxg_ld_prepare (VCFXG_LD_WALK=0: always).  The context is not
// indexed afterwards (vcfxg_line_ends and the per-line calls need vcfxg_index).
int vcfxg_ld_prepare_region(vcfxg_ctx *c, size_t data_start, int n_samples, int id_dot_to_pos, const char *rchrom,
                            size_t rlen, int has_region, int rstart, int rend, int parse_mode, uint64_t *n_variants) {
    if (!c || n_samples < 0 || (has_region && !rchrom && rlen)) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    if (data_start > c->n) data_start = c->n;
    new_index(c);
    HIPCHK(c, hipSetDevice(c->device));
    static const bool walk_env = [] {
        const char *e = getenv("VCFXG_LD_WALK");
        return !(e && e[0] == '0');
    }();
    const int64_t lo = (int64_t)data_start, hi = (int64_t)c->n;
    // the walkers' chunk: the record walks' (128 KiB for ~10 KB records), halved while the input
    // would give fewer than about 2 rounds of walkers over the chip (a 1 GB LD shard: 64 KiB;
    // each walker's last round otherwise runs with the chip half empty); VCFXG_LD_WALK_CHUNK
    // overrides
    static const int64_t ld_chunk_env = getenv("VCFXG_LD_WALK_CHUNK") ? atol(getenv("VCFXG_LD_WALK_CHUNK")) : 0;
    int64_t C = c->walk_chunk;
    if (ld_chunk_env >= 4096) C = ld_chunk_env;
    else
        while (C > 32768 && (hi - lo) / C < 2 * 20 * (int64_t)std::max(c->n_cu, 1)) C /= 2;
    const WalkPlan pl = walk_plan(c, data_start, C);
    const int64_t nw = pl.nw;
    const uint64_t cap_w = pl.cap_w, cap = pl.cap;
    const bool walk = walk_env && nw > 0 && n_samples > 0 && n_samples <= 4096 && walk_wanted(c, false) &&
                      pl.fits_gt16;
    auto indexed_path = [&]() -> int {
        note_schedule(c, "ld_index");
        int r = vcfxg_index(c, data_start, nullptr);
        return r ? r : vcfxg_ld_prepare(c, n_samples, id_dot_to_pos, rchrom, rlen, has_region, rstart, rend, parse_mode,
                                        n_variants);
    };
    if (!walk) return indexed_path();
    const int kpad = ((n_samples + 63) / 64) * 64;
    const int kp4 = vcfxg::ld_kp4(n_samples);
    int r = ensure(c, c->ld_G, (size_t)cap * kpad + 64);
    if (!r) r = ensure(c, c->ld_lines, sizeof(vcfxg::LdLine) * (cap + 1));
    if (!r) r = ensure(c, c->ld_wcnt, 8 * (size_t)(nw + 1));
    if (!r) r = ensure(c, c->ld_wval, 8 * (size_t)(nw + 1));
    if (!r) r = ensure(c, c->ld_vbase, 8 * (size_t)(nw + 1));
    if (!r) r = ensure(c, c->ld_small, 64);
    if (!r) r = ensure(c, c->ld_pend, 8 * (cap + 1));
    if (!r) r = ensure(c, c->ld_vars, sizeof(vcfxg::LdVar) * (cap + 1));
    if (!r) r = ensure(c, c->ld_fast, sizeof(vcfxg::LdFast) * (cap + 1));
    if (!r) r = ensure(c, c->ld_Gp, (size_t)(cap + 1) * kp4 + 64);
    if (!r) r = ensure(c, c->ld_gflag, cap / vcfxg::kLdFastBlock + 2);
    if (!r) r = ensure(c, c->ld_plen, 8 * (cap + 2));
    if (!r) r = ensure(c, c->ld_poff, 8 * (cap + 2));
    if (!r) r = ensure(c, c->query, rlen + 1);
    if (r) return r;
    if (rlen) {
        c->query_host.assign(rchrom, rlen);
        c->query_dev_p = nullptr;
        HIPCHK(c, hipMemcpyAsync(c->query.p, c->query_host.data(), rlen, hipMemcpyHostToDevice, c->stream));
    }
    const char *buf = P<char>(c->input);
    // small: [0] walk overflow (u32) | flags (u32: bit 0 = an incomplete variant), [1] M,
    // [2] pending lines
    uint64_t *small = P<uint64_t>(c->ld_small);
    unsigned *ovf = reinterpret_cast<unsigned *>(small), *flags = ovf + 1;
    HIPCHK(c, hipMemsetAsync(small, 0, 24, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->ld_wval) + nw, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ld_plen.p, 0, 8 * (cap + 1), c->stream));
    vcfxg::LdParseArgs a{n_samples, kpad, has_region, rstart, rend, (int64_t)rlen, P<char>(c->query), parse_mode};
    prof_begin(c, "ld_walk");
    HIPCHK(c, vcfxg::launch_ld_walk(buf, lo, hi, C, c->hint_span, cap_w, a, P<int8_t>(c->ld_G),
                                    P<vcfxg::LdLine>(c->ld_lines), P<uint64_t>(c->ld_wcnt), P<uint64_t>(c->ld_wval),
                                    ovf, reinterpret_cast<unsigned long long *>(small + 2), P<uint64_t>(c->ld_pend),
                                    c->stream));
    prof_end(c, "ld_walk");
    prof_begin(c, "ld_compact");
    r = exclusive_scan(c, P<uint64_t>(c->ld_wval), P<uint64_t>(c->ld_vbase), (size_t)nw + 1);
    if (r) return r;
    HIPCHK(c, vcfxg::launch_ld_wcompact(nw, cap_w, P<uint64_t>(c->ld_wcnt), P<uint64_t>(c->ld_vbase),
                                        P<vcfxg::LdLine>(c->ld_lines), n_samples, buf, id_dot_to_pos,
                                        P<vcfxg::LdVar>(c->ld_vars), P<vcfxg::LdFast>(c->ld_fast),
                                        P<uint64_t>(c->ld_plen), flags, small + 1, c->stream));
    prof_end(c, "ld_compact");
    static const bool sparse_env = [] {
        const char *e = getenv("VCFXG_LD_SPARSE");
        return !(e && e[0] == '0');
    }();
    const int sparse = sparse_env && n_samples <= 16383 ? 1 : 0;
    HIPCHK(c, vcfxg::launch_ld_groups(P<vcfxg::LdVar>(c->ld_vars), cap, n_samples, sparse, P<uint8_t>(c->ld_gflag),
                                      c->stream, small + 1));
    r = exclusive_scan(c, P<uint64_t>(c->ld_plen), P<uint64_t>(c->ld_poff), (size_t)cap + 1);
    if (r) return r;
    // one synchronisation: overflow, flags, M, the prefix bytes (plen is 0 past M) and the
    // group flags (computed for every group below cap; the first ceil(M / 256) are M's)
    static thread_local uint64_t sm[3];
    const uint64_t ng = (cap + vcfxg::kLdFastBlock - 1) / vcfxg::kLdFastBlock;
    c->ld_gflag_host.assign(ng + 1, 0);
    HIPCHK(c, hipMemcpyAsync(sm, small, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sm + 2, P<uint64_t>(c->ld_poff) + cap, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ld_gflag_host.data(), c->ld_gflag.p, ng, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((uint32_t)sm[0]) {  // a walker ran out of line slots (short lines): the index path
        prof_collect(c);
        c->walk_overflowed = true;
        return indexed_path();
    }
    note_schedule(c, "ld_walk");
    const uint64_t M = sm[1], pbytes = sm[2];
    prof_begin(c, "ld_pack");  // the FP4 rows, from the walk's slots
    HIPCHK(c, vcfxg::launch_ld_pack4(P<int8_t>(c->ld_G), M, kpad, n_samples, P<uint8_t>(c->ld_Gp), kp4, c->stream,
                                     P<vcfxg::LdVar>(c->ld_vars)));
    prof_end(c, "ld_pack");
    c->ld_gflag_host.resize(M / vcfxg::kLdFastBlock + 1);
    for (uint64_t g = (M + vcfxg::kLdFastBlock - 1) / vcfxg::kLdFastBlock; g < c->ld_gflag_host.size(); g++)
        c->ld_gflag_host[g] = 0;  // (past M: as the indexed path leaves them)
    c->ld_gc_ready = false;
    if ((sm[0] >> 32) & 1u) {  // some variant misses a call: its group's kernels read ld_Gc
        r = ensure(c, c->ld_Gc, (size_t)(M + 1) * kpad + 64);
        if (r) return r;
        prof_begin(c, "ld_gather");
        HIPCHK(c, vcfxg::launch_ld_gather(P<vcfxg::LdVar>(c->ld_vars), M, P<int8_t>(c->ld_G), kpad,
                                          P<int8_t>(c->ld_Gc), c->stream));
        prof_end(c, "ld_gather");
        c->ld_gc_ready = true;
    }
    c->indexed = false;  // (no line index: vcfxg_index before any per-line call)
    return ld_prepare_finish(c, M, n_samples, kpad, kp4, id_dot_to_pos, pbytes, false, n_variants);
}

// exact chrom equality ids (for max_dist): strings are the first field of each prefix
static int ld_chrom_ids(vcfxg_ctx *c) {
    if (c->ld_chrom_ids) return VCFXG_OK;
    const uint64_t M = c->ld_m;
    std::vector<uint64_t> poff(M + 1);
    std::string pre(c->ld_prefix_bytes, '\0');
    HIPCHK(c, hipMemcpyAsync(poff.data(), c->ld_poff.p, 8 * (M + 1), hipMemcpyDeviceToHost, c->stream));
    if (!pre.empty())
        HIPCHK(c, hipMemcpyAsync(&pre[0], c->ld_prefix.p, pre.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::map<std::string, uint32_t> ids;
    std::vector<uint32_t> id(M + 1);
    for (uint64_t v = 0; v < M; v++) {
        size_t a = poff[v], tab = pre.find('\t', a);
        auto ins = ids.emplace(pre.substr(a, tab - a), (uint32_t)ids.size());
        id[v] = ins.first->second;
    }
    int r = ensure(c, c->ld_cid, 4 * (M + 1));
    if (r) return r;
    c->ld_cid_host.swap(id);
    HIPCHK(c, hipMemcpyAsync(c->ld_cid.p, c->ld_cid_host.data(), 4 * M, hipMemcpyHostToDevice, c->stream));
    c->ld_chrom_ids = true;
    return VCFXG_OK;
}

int vcfxg_ld_stream_chunk(vcfxg_ctx *c, uint64_t j0, uint64_t j1, uint64_t window, double threshold, int max_dist,
                          uint64_t *n_pairs, uint64_t *text_bytes) {
    if (!c) return VCFXG_E_ARG;
    const uint64_t M = c->ld_m;
    if (j1 > M) j1 = M;
    if (window > M) window = M;  // a wider window holds the same pairs (and stays int64-safe)
    if (j0 >= j1 || M < 2) {
        c->text_bytes = 0;
        if (n_pairs) *n_pairs = 0;
        if (text_bytes) *text_bytes = 0;
        return VCFXG_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t BM = vcfxg::kLdBlock;
    if (max_dist > 0) {
        int r = ld_chrom_ids(c);
        if (r) return r;
    }
    // block lists.  Count-table columns are 64-blocks: row block J pairs with column blocks
    // I0(J) = (J*64 - window)/64 .. J.  Pairs of 256-groups that are all complete go to the
    // 256x256 X.X^T kernel (k_ld_fast); every other 64-block to the general kernel.
    const uint64_t FB = vcfxg::kLdFastBlock;
    auto ifirst = [&](uint64_t J) { const uint64_t jr0 = J * BM; return jr0 > window ? (jr0 - window) / BM : 0; };
    const std::vector<uint8_t> &gf = c->ld_gflag_host;
    constexpr uint64_t kSub = vcfxg::kLdFastBlock / BM;  // 64-blocks per fast group
    // a 64-block whose 256-group the fast or the sparse-missing kernel covers (with another such)
    auto gcomp = [&](uint64_t b64) { const uint8_t g = gf[b64 / kSub]; return g == 1 || (g == 2 && c->ld_sp); };
    static const bool use_mask = [] {
        const char *e = getenv("VCFXG_LD_MASK");
        return !(e && e[0] == '0');
    }();
    // the block lists are a pure function of (j0, j1, window, M, the kernel choice, the
    // per-group complete flags): a call with the same ones reuses the last lists and their
    // device copy (building 77 K tile pairs and copying them cost ~0.13 ms of host time per call)
    const bool mask_on = use_mask && c->ld_vq;
    const bool sp_on = c->ld_sp;
    const uint64_t pkey[5] = {j0, j1, window, M, (mask_on ? 1u : 0u) | (sp_on ? 2u : 0u)};
    const bool hit = c->ld_plan_dev != nullptr && c->ld_plan_dev == c->ld_blocks.p &&
                     std::equal(pkey, pkey + 5, c->ld_plan_key) && c->ld_plan_gf == gf;
    std::vector<uint32_t> blocks;
    uint64_t nb = 1;
    uint32_t nfast = 0, nmask = 0, nbl = 0, nsp = 0;
    for (uint64_t J = j0 / BM; J * BM < j1; J++) nb = std::max<uint64_t>(nb, J - ifirst(J) + 1);
    nb = (nb + 7) & ~(uint64_t)7;  // (k_ld_rowscan reads a row's counts 8 slots per 16 B load)
    if (hit) {
        nfast = c->ld_plan_n[0];
        nmask = c->ld_plan_n[1];
        nbl = c->ld_plan_n[2];
        nsp = c->ld_plan_n[3];
    } else {
        // fast list first, in kSuper x kSuper super-tiles (row blocks J x column blocks I): the
        // kernel maps contiguous list ranges to one XCD, so the blocks an XCD runs at once share
        // 2*kSuper operand tiles through its L2 instead of streaming distinct ones
        static const uint64_t kSuper = [] {
            const char *e = getenv("VCFXG_LD_SUPER");
            const long v = e ? atol(e) : 0;
            return (uint64_t)(v > 0 ? v : 4);
        }();
        const uint64_t Jb = j0 / FB, Je = (j1 + FB - 1) / FB;
        // pass 0: both groups complete (k_ld_fast); pass 1: both complete or sparse-missing, not
        // both complete (the sparse-missing form, kSp)
        for (int pass = 0; pass < (sp_on ? 2 : 1); pass++) {
            auto take = [&](uint64_t I, uint64_t J) {
                return pass == 0 ? gf[I] == 1 && gf[J] == 1 : gf[I] && gf[J] && (gf[I] == 2 || gf[J] == 2);
            };
            for (uint64_t J0 = Jb; J0 < Je; J0 += kSuper) {
                const uint64_t J1 = std::min(Je, J0 + kSuper);
                const uint64_t Ilo = ifirst(kSub * J0) / kSub;
                for (uint64_t I0 = Ilo; I0 < J1; I0 += kSuper)
                    for (uint64_t J = J0; J < J1; J++) {
                        if (!gf[J]) continue;
                        const uint64_t Imin = std::max(I0, ifirst(kSub * J) / kSub), Imax = std::min(I0 + kSuper, J + 1);
                        for (uint64_t I = Imin; I < Imax; I++)
                            if (take(I, J)) {
                                blocks.push_back((uint32_t)I);
                                blocks.push_back((uint32_t)J);
                            }
                    }
            }
            if (pass == 0) nfast = (uint32_t)(blocks.size() / 2);
            else nsp = (uint32_t)(blocks.size() / 2) - nfast;
        }
        // the missing-data tiles (k_ld_mask, default): every 128 x 128 tile pair in the window
        // whose 256-groups are not both complete (those are k_ld_fast's); VCFXG_LD_MASK=0 keeps the
        // previous int8 kernel (k_ld_block) over every 64-block pair with an incomplete side

        if (use_mask && c->ld_vq) {
            constexpr uint64_t TM = vcfxg::kLdMaskTile, kPerG = vcfxg::kLdFastBlock / vcfxg::kLdMaskTile;
            for (uint64_t J2 = j0 / TM; J2 * TM < j1; J2++) {
                const uint64_t I2lo = ifirst(J2 * (TM / BM)) / (TM / BM);  // the first 64-row's window start
                const uint8_t gj = gf[J2 / kPerG];
                for (uint64_t I2 = I2lo; I2 <= J2; I2++) {
                    const uint8_t gi = gf[I2 / kPerG];
                    if (gi == 1 && gj == 1) continue;           // a complete group pair: k_ld_fast
                    if (sp_on && gi && gj) continue;            // complete / sparse: the kSp kernel
                    blocks.push_back((uint32_t)I2);
                    blocks.push_back((uint32_t)J2);
                }
            }
            nmask = (uint32_t)(blocks.size() / 2) - nfast - nsp;
        } else {
            // for a complete row block J only the incomplete column blocks, found in the sorted list
            // of them (no scan over the whole window triangle on the host)
            const uint64_t Jlast = (j1 + BM - 1) / BM;
            std::vector<uint32_t> inc;
            for (uint64_t b = ifirst(j0 / BM); b < Jlast; b++)
                if (!gcomp(b)) inc.push_back((uint32_t)b);
            for (uint64_t J = j0 / BM; J * BM < j1; J++) {
                const uint64_t I0 = ifirst(J);
                if (!gcomp(J)) {
                    for (uint64_t I = I0; I <= J; I++) {
                        blocks.push_back((uint32_t)I);
                        blocks.push_back((uint32_t)J);
                    }
                    continue;
                }
                for (auto it = std::lower_bound(inc.begin(), inc.end(), (uint32_t)I0); it != inc.end() && *it <= J; ++it) {
                    blocks.push_back(*it);
                    blocks.push_back((uint32_t)J);
                }
            }
            nbl = (uint32_t)(blocks.size() / 2) - nfast - nsp;
        }
    }
    const uint64_t rows = j1 - j0;
    int r = hit ? VCFXG_OK : ensure(c, c->ld_blocks, 4 * blocks.size() + 8);
    if (!r) r = ensure(c, c->ld_cnt, 2 * rows * nb + 16);
    if (!r) r = ensure(c, c->ld_off, 4 * (rows * nb + 1));  // u32 offsets inside each row
    if (!r) r = ensure(c, c->ld_rowoff, 16 * (rows + 1));      // row totals, then row starts
    if (r) return r;
    if (!hit) {
        c->ld_blocks_host.swap(blocks);
        HIPCHK(c, hipMemcpyAsync(c->ld_blocks.p, c->ld_blocks_host.data(), 4 * c->ld_blocks_host.size(),
                                 hipMemcpyHostToDevice, c->stream));
        std::copy(pkey, pkey + 5, c->ld_plan_key);
        c->ld_plan_gf = gf;
        c->ld_plan_n[0] = nfast;
        c->ld_plan_n[1] = nmask;
        c->ld_plan_n[2] = nbl;
        c->ld_plan_n[3] = nsp;
        c->ld_plan_dev = c->ld_blocks.p;
    }
    // (no clearing of ld_cnt: the count kernels write every window slot the row scan reads)
    vcfxg::LdWindowArgs a{M, c->ld_kpad, c->ld_ns, window, threshold, max_dist, j0, j1, nb, 0.0, 0};
    // prefilter margin: |fp64 r^2 - exact r^2| of the reference's sequence is < ~1.2e-14 * n
    // (vx >= (n-1)/n^2 for a polymorphic complete variant); delta covers it 100-fold
    a.tm = threshold - (1e-6 + 1e-10 * (double)c->ld_ns);
    a.all_pass = a.tm <= 0.0;
    a.kp4 = c->ld_kp4;
    const uint32_t *cid = max_dist > 0 ? P<uint32_t>(c->ld_cid) : nullptr;
    const uint32_t *fbl = P<uint32_t>(c->ld_blocks), *sbl = fbl + 2 * (size_t)nfast,
                   *gbl = sbl + 2 * (size_t)nsp;
    vcfxg::LdSparse spa;
    if (nsp) {
        spa.vars = P<vcfxg::LdVar>(c->ld_vars);
        spa.gt16 = P<uint16_t>(c->ld_gt16);
        spa.mp = c->ld_mp;
        spa.moff = P<uint64_t>(c->ld_moff);
        spa.midx = P<uint16_t>(c->ld_midx);
        spa.mvar = P<uint32_t>(c->ld_mvar);
        spa.midx16 = P<uint16_t>(c->ld_midx16);
        spa.rec = P<vcfxg::LdSpRec>(c->ld_sprec);
        const double big = 4.0 * (double)c->ld_ns * (double)c->ld_ns;  // (k_ld_mask's bound)
        spa.pe = (float)(big * std::ldexp(1.0, -23) + 1.0);
    }
    // staging for the pairs the count pass finds (capacity: what the last chunk needed, at
    // least 4 M pairs; a larger chunk overflows once and the emit pass recomputes)
    vcfxg::LdStage stg;
    {
        const uint64_t qcap = 16ull * (nfast + nsp) + 16;
        const uint64_t tcap = c->ld_stage_cap_fixed ? c->ld_stage_cap_fixed : std::max<uint64_t>(c->ld_temp_cap, 4ull << 20);
        int r0 = ensure(c, c->ld_temp, sizeof(vcfxg::LdPair) * tcap);
        if (!r0) r0 = ensure(c, c->ld_quarters, sizeof(vcfxg::LdQuarter) * qcap);
        if (!r0) r0 = ensure(c, c->ld_stage_ctr, 64);
        if (r0) return r0;
        HIPCHK(c, hipMemsetAsync(c->ld_stage_ctr.p, 0, 64, c->stream));
        // (the register count path, n <= 23170, is the one that stages)
        stg.temp = c->ld_ns <= 23170 ? P<vcfxg::LdPair>(c->ld_temp) : nullptr;
        stg.cap = tcap;
        stg.quarters = P<vcfxg::LdQuarter>(c->ld_quarters);
        stg.qcap = qcap;
        stg.ctr = P<unsigned long long>(c->ld_stage_ctr);
        stg.overflow = reinterpret_cast<unsigned *>(P<unsigned long long>(c->ld_stage_ctr) + 2);
    }
    prof_begin(c, "ld_count");
    HIPCHK(c, vcfxg::launch_ld_fast(1, P<uint8_t>(c->ld_Gp), P<vcfxg::LdFast>(c->ld_fast), cid, a, fbl, nfast,
                                    P<uint16_t>(c->ld_cnt), vcfxg::LdOffsets{}, nullptr, stg, c->stream));
    prof_end(c, "ld_count");
    prof_begin(c, "ld_count_sparse");
    HIPCHK(c, vcfxg::launch_ld_sparse(1, P<uint8_t>(c->ld_Gp), spa, cid, a, sbl, nsp, P<uint16_t>(c->ld_cnt),
                                      vcfxg::LdOffsets{}, nullptr, stg, c->stream));
    prof_end(c, "ld_count_sparse");
    prof_begin(c, "ld_count_gen");
    HIPCHK(c, vcfxg::launch_ld_block(1, P<int8_t>(c->ld_Gc), P<vcfxg::LdVar>(c->ld_vars), cid, a, gbl, nbl,
                                     P<uint16_t>(c->ld_cnt), vcfxg::LdOffsets{}, nullptr, c->stream));
    prof_end(c, "ld_count_gen");
    prof_begin(c, "ld_count_mask");
    HIPCHK(c, vcfxg::launch_ld_mask(1, P<uint8_t>(c->ld_Gp), P<uint8_t>(c->ld_Gv), P<uint8_t>(c->ld_Gq),
                                    P<vcfxg::LdVar>(c->ld_vars), cid, a, gbl, nmask, P<uint16_t>(c->ld_cnt),
                                    vcfxg::LdOffsets{}, nullptr, c->stream));
    prof_end(c, "ld_count_mask");
    // ordered offsets: per-row scan of the count table (u32 inside a row), then the rows
    uint64_t *rowtot = P<uint64_t>(c->ld_rowoff), *rowbase = rowtot + (rows + 1);
    HIPCHK(c, vcfxg::launch_ld_rowscan(P<uint16_t>(c->ld_cnt), rows, nb, j0, window, P<uint32_t>(c->ld_off), rowtot,
                                       c->stream));
    HIPCHK(c, hipMemsetAsync(rowtot + rows, 0, 8, c->stream));
    r = exclusive_scan(c, rowtot, rowbase, (size_t)rows + 1);
    if (r) return r;
    vcfxg::LdOffsets offs;
    offs.row = rowbase;
    offs.in_row = P<uint32_t>(c->ld_off);
    static thread_local uint64_t tot, sctr[3];
    HIPCHK(c, hipMemcpyAsync(&tot, rowbase + rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sctr, c->ld_stage_ctr.p, 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (getenv("VCFXG_LD_DEBUG")) {  // (with a VCFXG_LD_EXPT & 256 build: the sparse kernel's half counts)
        uint64_t dbg[3] = {0, 0, 0};
        (void)hipMemcpy(dbg, P<unsigned long long>(c->ld_stage_ctr) + 4, 24, hipMemcpyDeviceToHost);
        fprintf(stderr, "ld_sparse: halves %llu, with tables %llu, prefilter candidates %llu\n",
                (unsigned long long)dbg[0], (unsigned long long)dbg[1], (unsigned long long)dbg[2]);
    }
    const uint64_t np = tot;
    const bool staged = stg.temp && (sctr[2] & 0xFFFFFFFFull) == 0;  // staged, no overflow
    c->ld_temp_cap = std::max<uint64_t>(c->ld_temp_cap, sctr[0] + sctr[0] / 4);
    r = ensure(c, c->ld_pairs, sizeof(vcfxg::LdPair) * (np + 1));
    if (!r) r = ensure(c, c->rowlen, 8 * (np + 1));
    if (!r) r = ensure(c, c->rowoff, 8 * (np + 1));
    if (r) return r;
    prof_begin(c, "ld_emit");
    if (staged)
        HIPCHK(c, vcfxg::launch_ld_scatter(P<vcfxg::LdQuarter>(c->ld_quarters), P<unsigned long long>(c->ld_stage_ctr),
                                           sctr[1], a, P<uint16_t>(c->ld_cnt), offs,
                                           P<vcfxg::LdPair>(c->ld_temp), P<vcfxg::LdPair>(c->ld_pairs), c->stream));
    else {
        HIPCHK(c, vcfxg::launch_ld_fast(2, P<uint8_t>(c->ld_Gp), P<vcfxg::LdFast>(c->ld_fast), cid, a, fbl, nfast,
                                        P<uint16_t>(c->ld_cnt), offs, P<vcfxg::LdPair>(c->ld_pairs),
                                        vcfxg::LdStage{}, c->stream));
        HIPCHK(c, vcfxg::launch_ld_sparse(2, P<uint8_t>(c->ld_Gp), spa, cid, a, sbl, nsp, P<uint16_t>(c->ld_cnt), offs,
                                          P<vcfxg::LdPair>(c->ld_pairs), vcfxg::LdStage{}, c->stream));
    }
    prof_end(c, "ld_emit");
    prof_begin(c, "ld_emit_gen");
    HIPCHK(c, vcfxg::launch_ld_block(2, P<int8_t>(c->ld_Gc), P<vcfxg::LdVar>(c->ld_vars), cid, a, gbl, nbl,
                                     P<uint16_t>(c->ld_cnt), offs, P<vcfxg::LdPair>(c->ld_pairs),
                                     c->stream));
    prof_end(c, "ld_emit_gen");
    prof_begin(c, "ld_emit_mask");
    HIPCHK(c, vcfxg::launch_ld_mask(2, P<uint8_t>(c->ld_Gp), P<uint8_t>(c->ld_Gv), P<uint8_t>(c->ld_Gq),
                                    P<vcfxg::LdVar>(c->ld_vars), cid, a, gbl, nmask, P<uint16_t>(c->ld_cnt), offs,
                                    P<vcfxg::LdPair>(c->ld_pairs), c->stream));
    prof_end(c, "ld_emit_mask");
    HIPCHK(c, vcfxg::launch_ld_pairtext(0, P<vcfxg::LdPair>(c->ld_pairs), np, P<uint64_t>(c->ld_poff), nullptr,
                                        P<uint64_t>(c->rowlen), nullptr, c->stream));
    HIPCHK(c, hipMemsetAsync(P<uint64_t>(c->rowlen) + np, 0, 8, c->stream));
    r = exclusive_scan(c, P<uint64_t>(c->rowlen), P<uint64_t>(c->rowoff), (size_t)np + 1);
    if (r) return r;
    static thread_local uint64_t tb;
    HIPCHK(c, hipMemcpyAsync(&tb, P<uint64_t>(c->rowoff) + np, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    r = ensure(c, c->text, tb + 16);
    if (r) return r;
    prof_begin(c, "ld_text");
    HIPCHK(c, vcfxg::launch_ld_pairtext(1, P<vcfxg::LdPair>(c->ld_pairs), np, P<uint64_t>(c->ld_poff),
                                        P<char>(c->ld_prefix), P<uint64_t>(c->rowoff), P<char>(c->text), c->stream));
    prof_end(c, "ld_text");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = tb;
    c->ld_np = np;
    if (n_pairs) *n_pairs = np;
    if (text_bytes) *text_bytes = tb;
    return VCFXG_OK;
}

int vcfxg_ld_fetch_pairs(vcfxg_ctx *c, uint64_t first, uint64_t count, uint32_t *vi, uint32_t *vj, double *r2) {
    if (!c || first > c->ld_np || count > c->ld_np - first) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<vcfxg::LdPair> h(count);
    HIPCHK(c, hipMemcpyAsync(h.data(), P<vcfxg::LdPair>(c->ld_pairs) + first, sizeof(vcfxg::LdPair) * count,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint64_t k = 0; k < count; ++k) {
        if (vi) vi[k] = h[k].i;
        if (vj) vj[k] = h[k].j;
        if (r2) r2[k] = h[k].r2;
    }
    return VCFXG_OK;
}

int vcfxg_ld_prefixes(vcfxg_ctx *c, char *text, size_t cap, uint64_t *offsets) {
    if (!c) return VCFXG_E_ARG;
    if (cap < c->ld_prefix_bytes) return VCFXG_E_CAP;
    if (c->ld_prefix_bytes && text)
        HIPCHK(c, hipMemcpyAsync(text, c->ld_prefix.p, c->ld_prefix_bytes, hipMemcpyDeviceToHost, c->stream));
    if (offsets)
        HIPCHK(c, hipMemcpyAsync(offsets, c->ld_poff.p, 8 * (c->ld_m + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_ld_matrix(vcfxg_ctx *c, int gate, int printf4, uint64_t *cell_bytes) {
    if (!c) return VCFXG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t M = c->ld_m, BM = vcfxg::kLdBlock;
    std::vector<uint32_t> blocks;
    for (uint64_t J = 0; J * BM < M; J++)
        for (uint64_t I = 0; I <= J; I++) {
            blocks.push_back((uint32_t)I);
            blocks.push_back((uint32_t)J);
        }
    const uint64_t cells = 7ull * M * M;
    int r = ensure(c, c->ld_blocks, 4 * blocks.size() + 8);
    if (!r) r = ensure(c, c->text, cells + 16);
    if (r) return r;
    c->ld_blocks_host.swap(blocks);
    c->ld_plan_dev = nullptr;  // (the streaming lists' device copy is overwritten)
    HIPCHK(c, hipMemcpyAsync(c->ld_blocks.p, c->ld_blocks_host.data(), 4 * c->ld_blocks_host.size(),
                             hipMemcpyHostToDevice, c->stream));
    prof_begin(c, "ld_matrix");
    HIPCHK(c, vcfxg::launch_ld_matrix(P<int8_t>(c->ld_Gc), P<vcfxg::LdVar>(c->ld_vars), M, c->ld_kpad, c->ld_ns, gate,
                                      printf4, P<uint32_t>(c->ld_blocks), (uint32_t)(c->ld_blocks_host.size() / 2),
                                      P<char>(c->text), c->stream));
    prof_end(c, "ld_matrix");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = cells;
    if (cell_bytes) *cell_bytes = cells;
    return VCFXG_OK;
}

}  // extern "C"
