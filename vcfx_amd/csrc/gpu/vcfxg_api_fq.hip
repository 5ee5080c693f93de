// vcfxg_api_fq.hip -- the filter / query tools: VCFX_nonref_filter, VCFX_genotype_query,
// VCFX_record_filter, the fused pipeline, VCFX_missing_detector (it runs the filter / query walk)
// and VCFX_variant_counter (the C ABI of include/vcfx_gpu.h)
#include "vcfxg_ctx.h"
#include "vcfxg_decimal.h"

using namespace vcfxg;

extern "C" {

// parseDiploidAlleles (VCFX_genotype_query.cpp:246-272) incl. its partial assignment on
// failure, then the swap of main :641-645
static void gq_parse_query(const char *q, size_t n, int &qa, int &qb) {
    qa = qb = -1;
    size_t sep = (size_t)-1;
    for (size_t i = 0; i < n; i++)
        if (q[i] == '|' || q[i] == '/') { sep = i; break; }
    if (sep == (size_t)-1 || sep == 0 || sep == n - 1) return;
    if (sep == 1 && q[0] == '.') return;
    unsigned v = 0;
    qa = 0;
    bool ok = true;
    for (size_t i = 0; i < sep && ok; i++) {
        if (q[i] < '0' || q[i] > '9') ok = false;
        else qa = (int)(v = v * 10u + (unsigned)(q[i] - '0'));
    }
    if (ok) {
        if (!(n - sep - 1 == 1 && q[sep + 1] == '.')) {
            v = 0;
            qb = 0;
            for (size_t i = sep + 1; i < n; i++) {
                if (q[i] < '0' || q[i] > '9') break;
                qb = (int)(v = v * 10u + (unsigned)(q[i] - '0'));
            }
        }
    }
    if (qa > qb) std::swap(qa, qb);
}

int vcfxg_nonref_filter(vcfxg_ctx *c, int mode, vcfxg_summary *out) {
    if (!c || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t L = c->n_lines;
    int r = status_buffer(c, L, StatusOwner::other);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    prof_begin(c, "nr_records");
    HIPCHK(c, vcfxg::launch_nr_records(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end),
                                       P<uint64_t>(c->d_nlines), L, mode, P<uint8_t>(c->status),
                                       P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "nr_records");
    static thread_local uint64_t host_cnt[4];
    HIPCHK(c, hipMemcpyAsync(host_cnt, c->counters.p, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = 0;
    if (out) {
        out->n_lines = L;
        out->rows = host_cnt[0];
        out->data_lines = host_cnt[1];
        out->warn_lines = 0;
        out->general_records = host_cnt[3];
        out->text_bytes = 0;
    }
    return VCFXG_OK;
}

int vcfxg_genotype_query(vcfxg_ctx *c, const char *query, size_t qlen, int strict, int strip_cr, vcfxg_summary *out) {
    if (!c || (!query && qlen)) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t L = c->n_lines;
    int r = status_buffer(c, L, StatusOwner::other);
    if (!r) r = ensure(c, c->query, qlen + 1);
    if (!r) r = ensure(c, c->af_meta, vcfxg::af_meta_bytes() * (L + 1));
    if (r) return r;
    int qa = -1, qb = -1;
    if (!strict) gq_parse_query(query, qlen, qa, qb);
    c->query_host.assign(query, qlen);
    if (qlen)
        HIPCHK(c, hipMemcpyAsync(c->query.p, c->query_host.data(), qlen, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    prof_begin(c, "gq_records");
    HIPCHK(c, vcfxg::launch_gq_records(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end),
                                       P<uint64_t>(c->d_nlines), L, strip_cr, P<char>(c->query), (int)qlen, strict,
                                       qa, qb, P<uint8_t>(c->status), P<unsigned long long>(c->counters), c->stream,
                                       nullptr, c->af_meta.p));
    prof_end(c, "gq_records");
    static thread_local uint64_t host_cnt[4];
    HIPCHK(c, hipMemcpyAsync(host_cnt, c->counters.p, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->text_bytes = 0;
    if (out) {
        out->n_lines = L;
        out->rows = host_cnt[0];
        out->data_lines = host_cnt[1];
        out->warn_lines = host_cnt[2];
        out->general_records = host_cnt[3];
        out->text_bytes = 0;
    }
    return VCFXG_OK;
}

static vcfxg::DecRef put_dec(const vcfxg::DecHost &d, std::string &pool) {
    vcfxg::DecRef r;
    r.sign = d.sign;
    r.exp = d.exp;
    r.off = (uint32_t)pool.size();
    r.n = (uint32_t)d.digits.size();
    r.inf = d.inf;
    pool += d.digits;
    return r;
}

// threshold_bounds memoised by the value's bits: the exact decimal expansion of a boundary
// (up to ~750 digits for the subnormal neighbours of 0.0, which every FILTER criterion asks
// for) cost tens of microseconds per call, paid again for every region call with the same
// criteria (a bounded per-thread table; the result is a pure function of the value)
static void cached_threshold_bounds(double t, vcfxg::ThresholdHost &out) {
    static thread_local std::map<uint64_t, vcfxg::ThresholdHost> memo;
    uint64_t key;
    std::memcpy(&key, &t, sizeof key);
    auto it = memo.find(key);
    if (it != memo.end()) {
        out = it->second;
        return;
    }
    vcfxg::threshold_bounds(t, out);
    if (memo.size() >= 64) memo.clear();
    memo.emplace(key, out);
}

static int compile_criteria(vcfxg_ctx *c, const vcfxg_criterion *crit, int n) {
    std::vector<vcfxg::RfCrit> dev((size_t)n);
    std::string pool;
    for (int i = 0; i < n; i++) {
        const vcfxg_criterion &h = crit[i];
        vcfxg::RfCrit &d = dev[(size_t)i];
        std::memset(&d, 0, sizeof d);
        d.target = h.target;
        d.op = h.op;
        d.numeric = h.numeric;
        d.key_off = (uint32_t)pool.size();
        d.key_len = (uint32_t)h.key_len;
        pool.append(h.key ? h.key : "", h.key_len);
        d.str_off = (uint32_t)pool.size();
        d.str_len = (uint32_t)h.str_len;
        pool.append(h.str ? h.str : "", h.str_len);
        vcfxg::ThresholdHost th;
        // FILTER and string INFO criteria never compare numbers: no boundary digits (they
        // would only lengthen the pool the filter walk keeps in registers)
        const bool cmp_num = h.target != vcfxg::RF_FILTER && (h.target != vcfxg::RF_INFO || h.numeric);
        cached_threshold_bounds(cmp_num && h.numeric ? h.value : 0.0, th);
        if (!cmp_num) th.lo.digits.clear(), th.hi.digits.clear();
        d.T.t = h.numeric ? h.value : 0.0;
        d.T.kind = th.kind;
        d.T.lo = put_dec(th.lo, pool);
        d.T.hi = put_dec(th.hi, pool);
        d.T.lo_to_t = th.lo_to_t;
        d.T.hi_to_t = th.hi_to_t;
    }
    int r = ensure(c, c->crit, sizeof(vcfxg::RfCrit) * (size_t)(n + 1));
    if (!r) r = ensure(c, c->pool, pool.size() + 16);
    if (r) return r;
    c->crit_host.assign((const char *)dev.data(), sizeof(vcfxg::RfCrit) * (size_t)n);
    c->pool_host = pool;
    if (n && !(c->crit_dev_p == c->crit.p && c->crit_dev == c->crit_host)) {
        HIPCHK(c, hipMemcpyAsync(c->crit.p, c->crit_host.data(), c->crit_host.size(), hipMemcpyHostToDevice, c->stream));
        c->crit_dev = c->crit_host;
        c->crit_dev_p = c->crit.p;
    }
    if (!pool.empty() && !(c->pool_dev_p == c->pool.p && c->pool_dev == c->pool_host)) {
        HIPCHK(c, hipMemcpyAsync(c->pool.p, c->pool_host.data(), pool.size(), hipMemcpyHostToDevice, c->stream));
        c->pool_dev = c->pool_host;
        c->pool_dev_p = c->pool.p;
    }
    return VCFXG_OK;
}

static int run_rf(vcfxg_ctx *c, const vcfxg_criterion *crit, int n, int and_logic, int keep_cr = 0) {
    int r = status_buffer(c, c->n_lines, StatusOwner::other);
    if (!r) r = compile_criteria(c, crit, n);
    if (r) return r;
    prof_begin(c, "rf_records");
    HIPCHK(c, vcfxg::launch_rf_records(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end),
                                       P<uint64_t>(c->d_nlines), c->n_lines, P<vcfxg::RfCrit>(c->crit), n, and_logic,
                                       P<char>(c->pool), P<uint8_t>(c->status), P<unsigned long long>(c->counters),
                                       c->stream, keep_cr));
    prof_end(c, "rf_records");
    return VCFXG_OK;
}

int vcfxg_record_filter(vcfxg_ctx *c, const vcfxg_criterion *crit, int n, int and_logic, vcfxg_summary *out) {
    return vcfxg_record_filter_ex(c, crit, n, and_logic, 0, out);
}

int vcfxg_record_filter_ex(vcfxg_ctx *c, const vcfxg_criterion *crit, int n, int and_logic, int flags,
                           vcfxg_summary *out) {
    if (!c || n < 0 || (n && !crit) || (flags & ~VCFXG_RF_KEEP_CR)) return VCFXG_E_ARG;
    for (int k = 0; k < n; k++)
        if (crit[k].target < 0 || crit[k].target > vcfxg::RF_QUAL_LENIENT) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    int r = run_rf(c, crit, n, and_logic, (flags & VCFXG_RF_KEEP_CR) ? 1 : 0);
    if (r) return r;
    static thread_local uint64_t host_cnt[2];
    HIPCHK(c, hipMemcpyAsync(host_cnt, c->counters.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = c->n_lines;
        out->rows = host_cnt[0];
        out->data_lines = host_cnt[1];
    }
    return VCFXG_OK;
}

int vcfxg_filter_query(vcfxg_ctx *c, const vcfxg_criterion *crit, int n, int and_logic, const char *query, size_t qlen,
                       int strict, vcfxg_summary *out) {
    if (!c || n < 0 || (n && !crit) || (!query && qlen)) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    int r = run_rf(c, crit, n, and_logic);
    if (!r) r = ensure(c, c->query, qlen + 1);
    if (r) return r;
    int qa = -1, qb = -1;
    if (!strict) gq_parse_query(query, qlen, qa, qb);
    c->query_host.assign(query, qlen);
    if (qlen)
        HIPCHK(c, hipMemcpyAsync(c->query.p, c->query_host.data(), qlen, hipMemcpyHostToDevice, c->stream));
    r = ensure(c, c->af_meta, vcfxg::af_meta_bytes() * (c->n_lines + 1));
    if (r) return r;
    prof_begin(c, "gq_records");
    HIPCHK(c, vcfxg::launch_gq_records(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end),
                                       P<uint64_t>(c->d_nlines), c->n_lines, 1, P<char>(c->query), (int)qlen, strict,
                                       qa, qb, P<uint8_t>(c->status), P<unsigned long long>(c->counters) + 4,
                                       c->stream, P<uint8_t>(c->status), c->af_meta.p));
    prof_end(c, "gq_records");
    static thread_local uint64_t host_cnt[8];
    HIPCHK(c, hipMemcpyAsync(host_cnt, c->counters.p, 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = c->n_lines;
        out->rows = host_cnt[4];        // kept by both stages
        out->data_lines = host_cnt[0];  // kept by record_filter
        out->warn_lines = host_cnt[6];
        out->general_records = host_cnt[7];
    }
    return VCFXG_OK;
}

// record_filter / genotype_query / the fused pipeline over the data region in one pass
// (vcfxg_fq_walk.hip): k_fq_walk reads each chunk's lines once (no separate index sweep), the
// walkers' regions are concatenated in file order (k_fq_compact), k_fq_finish filters the
// lines whose head did not fit the walk's window and counts, k_gq_complex takes the query's
// general lines; ONE host synchronisation reads the counters.  Short lines (the first lines
// average under 512 B), an earlier walk overflow on this input, or VCFXG_FQ_WALK=-1:
// vcfxg_index + the per-tool call, with identical results.
static int fq_region(vcfxg_ctx *c, size_t data_start, int what, const vcfxg_criterion *crit, int n, int and_logic,
                     const char *query, size_t qlen, int strict, int gq_strip_cr, vcfxg_summary *out) {
    if (!c || n < 0 || (n && !crit) || (!query && qlen)) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    new_index(c);
    if (data_start > c->n) data_start = c->n;
    HIPCHK(c, hipSetDevice(c->device));
    const WalkPlan pl = walk_plan(c, data_start);
    // VCFXG_FQ_WALK: -1 never walks, 0 walks long records, any other value records of any length
    const bool walk = pl.nw && c->fq_path >= 0 && (c->fq_path ? !c->walk_overflowed : walk_wanted(c, false));
    if (!walk) {
        note_schedule(c, "fq_two_sweep");
        int r = vcfxg_index(c, data_start, nullptr);
        if (r) return r;
        if (what == vcfxg::kFqRF) return vcfxg_record_filter(c, crit, n, and_logic, out);
        if (what == vcfxg::kFqGQ) return vcfxg_genotype_query(c, query, qlen, strict, gq_strip_cr, out);
        if (what == vcfxg::kFqNR) return vcfxg_nonref_filter(c, gq_strip_cr ? VCFXG_MODE_FILE : VCFXG_MODE_STDIN, out);
        return vcfxg_filter_query(c, crit, n, and_logic, query, qlen, strict, out);
    }
    note_schedule(c, "fq_walk");
    const bool nr = what == vcfxg::kFqNR;  // nonref_filter: the query's walk with its own reducer
    const bool rf = !nr && (what & vcfxg::kFqRF) != 0, gq = nr || (what & vcfxg::kFqGQ) != 0;
    const int64_t lo = pl.lo;
    const uint64_t cap = pl.cap;
    int r = gq ? ensure(c, c->query, qlen + 1) : VCFXG_OK;
    if (!r && rf) r = compile_criteria(c, crit, n);
    if (r) return r;
    int qa = -1, qb = -1;
    if (gq) {
        if (!strict) gq_parse_query(query, qlen, qa, qb);
        c->query_host.assign(query, qlen);
        if (qlen && !(c->query_dev_p == c->query.p && c->query_dev == c->query_host)) {
            HIPCHK(c, hipMemcpyAsync(c->query.p, c->query_host.data(), qlen, hipMemcpyHostToDevice, c->stream));
            c->query_dev = c->query_host;
            c->query_dev_p = c->query.p;
        }
    }
    const char *buf = P<char>(c->input);
    const int strip_cr = rf ? 1 : gq_strip_cr;  // the pipeline's query sees record_filter's output
    const int pool_len = (int)c->pool_host.size();
    const vcfxg::RfArgs ra{P<vcfxg::RfCrit>(c->crit), n, and_logic ? 1 : 0, P<char>(c->pool), pool_len};
    r = fq_walk_to_dense(c, pl, what, strip_cr, ra, P<char>(c->query), (int)qlen, strict, qa, qb, "fq_walk", "fq_rest");
    if (r) return r;
    unsigned long long *cnt = P<unsigned long long>(c->fq_small) + 1;
    unsigned long long *gq_cnt = what == vcfxg::kFqBoth ? cnt + 4 : cnt;
    if (nr)
        HIPCHK(c, vcfxg::launch_nr_complex(buf, lo, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), cap,
                                           strip_cr ? VCFXG_MODE_FILE : VCFXG_MODE_STDIN, P<uint8_t>(c->status), cnt,
                                           c->stream));
    else
        // (a thread per line of the previous call, at most cap: the kernel grid-strides over the
        // device count, so fewer threads than lines is still exact)
        HIPCHK(c, vcfxg::launch_fq_finish(what, buf, lo, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines),
                                          c->fq_lines_hint ? std::min<uint64_t>(cap, c->fq_lines_hint) : cap, ra,
                                          P<uint8_t>(c->status), c->af_meta.p, c->rf_tabs.p, cnt, gq_cnt, c->stream));
    if (gq && !nr)
        HIPCHK(c, vcfxg::launch_gq_complex(buf, lo, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), cap, strip_cr,
                                           P<char>(c->query), (int)qlen, strict, qa, qb, c->af_meta.p,
                                           P<uint8_t>(c->status), gq_cnt,
                                           what == vcfxg::kFqBoth ? P<uint8_t>(c->status) : nullptr, c->stream));
    prof_end(c, "fq_rest");
    uint64_t *host = c->sum_host + 8;  // counters[0..7], lines, overflow (k_fq_done)
    r = fq_walk_done(c);
    if (r) return r;
    c->fq_lines_hint = host[8];
    prof_collect(c);
    if (host[9]) {  // a walker ran out of line slots (short lines): index + the per-tool kernels
        c->walk_overflowed = true;
        return fq_region(c, data_start, what, crit, n, and_logic, query, qlen, strict, gq_strip_cr, out);
    }
    c->data_start = data_start;
    c->n_lines = host[8];
    c->indexed = true;
    c->text_bytes = 0;
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = host[8];
        if (what == vcfxg::kFqBoth) {
            out->rows = host[4];        // kept by both stages
            out->data_lines = host[0];  // kept by record_filter
            out->warn_lines = host[6];
            out->general_records = host[7];
        } else {
            out->rows = host[0];
            out->data_lines = host[1];
            if (nr) out->general_records = host[3];
            else if (gq) {
                out->warn_lines = host[2];
                out->general_records = host[3];
            }
        }
    }
    return VCFXG_OK;
}

int vcfxg_record_filter_region(vcfxg_ctx *c, size_t data_start, const vcfxg_criterion *crit, int n, int and_logic,
                               vcfxg_summary *out) {
    return fq_region(c, data_start, vcfxg::kFqRF, crit, n, and_logic, nullptr, 0, 0, 0, out);
}

int vcfxg_genotype_query_region(vcfxg_ctx *c, size_t data_start, const char *query, size_t qlen, int strict,
                                int strip_cr, vcfxg_summary *out) {
    return fq_region(c, data_start, vcfxg::kFqGQ, nullptr, 0, 0, query, qlen, strict, strip_cr, out);
}

int vcfxg_filter_query_region(vcfxg_ctx *c, size_t data_start, const vcfxg_criterion *crit, int n, int and_logic,
                              const char *query, size_t qlen, int strict, vcfxg_summary *out) {
    return fq_region(c, data_start, vcfxg::kFqBoth, crit, n, and_logic, query, qlen, strict, 1, out);
}
int vcfxg_nonref_filter_region(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out) {
    if (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN) return VCFXG_E_ARG;
    return fq_region(c, data_start, vcfxg::kFqNR, nullptr, 0, 0, "", 0, 0, mode == VCFXG_MODE_FILE ? 1 : 0, out);
}

// VCFX_missing_detector over [data_start, n): for long GT-only records the filter / query walk
// with the missing-allele reducer (one HBM pass; k_md_lines then takes the lines it left and
// the flagged lines' INFO spans), else the line index and k_md_lines on every line
static int md_region_walk(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out) {
    new_index(c);
    HIPCHK(c, hipSetDevice(c->device));
    const WalkPlan pl = walk_plan(c, data_start);
    const int64_t lo = pl.lo;
    const uint64_t cap = pl.cap;
    int r = af_buffers(c, cap, StatusOwner::other);
    if (r) return r;
    const char *buf = P<char>(c->input);
    const vcfxg::RfArgs ra{nullptr, 0, 1, nullptr, 0};
    r = fq_walk_to_dense(c, pl, vcfxg::kFqMD, mode == VCFXG_MODE_FILE ? 1 : 0, ra, nullptr, 0, 0, -1, -1, "md_walk",
                         "md_rest");
    if (r) return r;
    unsigned long long *cnt = P<unsigned long long>(c->fq_small) + 1;
    HIPCHK(c, vcfxg::launch_md_lines(buf, lo, (int64_t)c->n, P<uint64_t>(c->line_end), P<uint64_t>(c->d_nlines), cap,
                                     mode, P<uint8_t>(c->status), P<int32_t>(c->alt), P<int32_t>(c->tot),
                                     cnt, c->stream, 1));
    prof_end(c, "md_rest");
    r = fq_walk_done(c);
    if (r) return r;
    uint64_t h[5] = {c->sum_host[8], c->sum_host[9], c->sum_host[10], c->sum_host[16], c->sum_host[17]};
    prof_collect(c);
    if (h[4] & 0xFFFFFFFFu) {  // a walker ran out of line slots (short lines): no walk
        c->walk_overflowed = true;
        return vcfxg_missing_region(c, data_start, mode, out);
    }
    c->data_start = data_start;
    c->n_lines = h[3];
    c->indexed = true;
    c->text_bytes = 0;
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = h[3];
        out->data_lines = h[0];
        out->rows = h[1];
        out->general_records = h[2];
    }
    return VCFXG_OK;
}

int vcfxg_missing_region(vcfxg_ctx *c, size_t data_start, int mode, vcfxg_summary *out) {
    if (!c || (mode != VCFXG_MODE_FILE && mode != VCFXG_MODE_STDIN)) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    if (data_start > c->n) data_start = c->n;
    // the walk for long GT-only records (VCFXG_FQ_WALK: 1 always, -1 never), as the filter tools
    const bool walk = walk_plan(c, data_start).nw && c->fq_path >= 0 &&
                      (c->fq_path == 1 ? !c->walk_overflowed : walk_wanted(c, true));
    if (walk) return md_region_walk(c, data_start, mode, out);
    uint64_t L = 0;
    int r = vcfxg_index(c, data_start, &L);
    if (r) return r;
    HIPCHK(c, hipSetDevice(c->device));
    r = af_buffers(c, L, StatusOwner::other);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    prof_begin(c, "md_lines");
    HIPCHK(c, vcfxg::launch_md_lines(P<char>(c->input), (int64_t)data_start, (int64_t)c->n, P<uint64_t>(c->line_end),
                                     P<uint64_t>(c->d_nlines), L, mode, P<uint8_t>(c->status), P<int32_t>(c->alt),
                                     P<int32_t>(c->tot), P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "md_lines");
    static thread_local uint64_t cnt[3];
    HIPCHK(c, hipMemcpyAsync(cnt, c->counters.p, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = L;
        out->data_lines = cnt[0];
        out->rows = cnt[1];
        out->general_records = cnt[2];
    }
    return VCFXG_OK;
}

int vcfxg_variant_count(vcfxg_ctx *c, int strip_cr, vcfxg_summary *out) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    HIPCHK(c, hipSetDevice(c->device));
    int r = status_buffer(c, c->n_lines, StatusOwner::other);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 64, c->stream));
    prof_begin(c, "vc_records");
    HIPCHK(c, vcfxg::launch_vc_records(P<char>(c->input), (int64_t)c->data_start, P<uint64_t>(c->line_end),
                                       P<uint64_t>(c->d_nlines), c->n_lines, strip_cr, P<uint8_t>(c->status),
                                       P<unsigned long long>(c->counters), c->stream));
    prof_end(c, "vc_records");
    static thread_local uint64_t host_cnt[2];
    HIPCHK(c, hipMemcpyAsync(host_cnt, c->counters.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_lines = c->n_lines;
        out->rows = host_cnt[0];
        out->warn_lines = host_cnt[1];
    }
    return VCFXG_OK;
}

}  // extern "C"
