// vcfxg_api_bgzf.hip -- device BGZF inflate: staging the compressed stream, the batched member
// launches and vcfxg_ingest_bgzf (the C ABI of include/vcfx_gpu.h)
#include <chrono>

#include "vcfxg_ctx.h"

using namespace vcfxg;

extern "C" {

static_assert(sizeof(vcfxg_bgzf_member) == sizeof(vcfxg::BgzfMember), "BGZF member layout");
constexpr size_t kCompPad = 8192;  // the inflate reader's ring loads run up to 3 KiB past a stream

// VCFX_TIMING=1: "[vcfxg-timing] <what> <ms>" on stderr at the steps of a fresh context's first
// BGZF stage (ms since the library loaded; the host's own phases are hostio.cpp phase())
static void lib_phase(const char *what) {
    static const auto t0 = std::chrono::steady_clock::now();
    static const bool on = getenv("VCFX_TIMING") && atoi(getenv("VCFX_TIMING")) > 0;
    if (!on) return;
    fprintf(stderr, "[vcfxg-timing] %s %.2f ms\n", what,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// (a member holds >= 20 compressed bytes: at most this many members in a stream)
static uint64_t bgz_max_members(size_t comp_total) { return comp_total / 20 + 2; }

// The member tables (members, output offsets, verdicts, the lane order) of a staged stream hold
// `want` members, keeping the first `keep` (the entries the launched batches wrote; every batch
// is complete -- the caller made `stream` wait for them).  Sized at the stage's start for members
// of >= 1 KiB compressed (a genotype VCF's are ~4 KiB): 28 B a member where the worst case
// (20-byte members) would be ~1.4x the compressed bytes; a stream of smaller members stops
// batching (E_CAP) and grows them at the end.
static int bgz_tables(vcfxg_ctx *c, uint64_t want, uint64_t keep) {
    struct Tab {
        DevBuf *b;
        size_t w;
    } t[] = {{&c->bgz_mem, sizeof(vcfxg_bgzf_member)}, {&c->bgz_off, 8}, {&c->bgz_stat, 4}, {&c->bgz_perm, 4}};
    bool need = false;
    for (const Tab &x : t) need = need || x.b->cap < x.w * want;
    if (!need) return VCFXG_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (const Tab &x : t) {
        if (x.b->cap >= x.w * want) continue;
        const int r = regrow(c, *x.b, x.w * want + x.w * want / 8, x.w * keep);
        if (r) return r;
    }
    return VCFXG_OK;
}
static uint64_t bgz_table_members(const vcfxg_ctx *c) { return c->bgz_mem.cap / sizeof(vcfxg_bgzf_member); }

int vcfxg_bgzf_stage(vcfxg_ctx *c, const void *host, size_t n, size_t offset, size_t comp_total) {
    if (!c || (!host && n) || offset > comp_total || n > comp_total - offset) return VCFXG_E_ARG;
    if (!c->ingesting) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    if (offset == 0) {
        static const uint64_t tset = [] {  // (VCFXG_BGZF_TABLE: the members sized for; tests: tiny)
            const char *e = getenv("VCFXG_BGZF_TABLE");
            return e && *e ? std::max<uint64_t>(2, strtoull(e, nullptr, 10)) : (uint64_t)0;
        }();
        const uint64_t mm = std::min<uint64_t>(bgz_max_members(comp_total),
                                               tset ? tset : std::max<uint64_t>(65536, comp_total / 1024));
        lib_phase("bgzf stage: begin");
        int r = ensure(c, c->bgz_in, comp_total + kCompPad);
        lib_phase("bgzf stage: compressed buffer");
        if (!r) r = bgz_tables(c, mm, 0);
        if (!r) r = ensure(c, c->bgz_small, 64);
        if (r) return r;
        lib_phase("bgzf stage: member tables");
        if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        if (!c->bgz_copy_ev) HIPCHK(c, hipEventCreateWithFlags(&c->bgz_copy_ev, hipEventDisableTiming));
        for (int k = 0; k < vcfxg_ctx::kBgzStreams; k++) {
            if (!c->bgz_stream[k]) HIPCHK(c, hipStreamCreateWithFlags(&c->bgz_stream[k], hipStreamNonBlocking));
            if (!c->bgz_ev[k]) HIPCHK(c, hipEventCreateWithFlags(&c->bgz_ev[k], hipEventDisableTiming));
        }
        c->bgz_next = 0;
        lib_phase("bgzf stage: streams");
        // (the first-bad marker and the hand-over count, then the stream's earlier work -- buffers
        // just reallocated, the last call's kernels: every batch is ordered after this event)
        HIPCHK(c, hipMemsetAsync(c->bgz_small.p, 0xFF, 8, c->stream));
        HIPCHK(c, hipMemsetAsync(P<uint8_t>(c->bgz_small) + 8, 0, 56, c->stream));
        HIPCHK(c, hipEventRecord(c->bgz_copy_ev, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->bgz_copy_ev, 0));
        c->bgz_total = comp_total;
        c->bgz_staged = 0;
        c->bgz_launched = 0;
        c->bgz_out = 0;
    }
    if (comp_total != c->bgz_total || offset != c->bgz_staged) return VCFXG_E_ARG;  // (in order)
    if (!n) return VCFXG_OK;
    // the copies on their own stream, so they overlap the inflate batches (vcfxg_bgzf_inflate)
    HIPCHK(c, hipMemcpyAsync(P<uint8_t>(c->bgz_in) + offset, host, n, hipMemcpyHostToDevice, c->copy_stream));
    c->bgz_staged = offset + n;
    if (c->bgz_staged == comp_total)
        HIPCHK(c, hipMemsetAsync(P<uint8_t>(c->bgz_in) + comp_total, 0, kCompPad, c->copy_stream));
    HIPCHK(c, hipEventRecord(c->bgz_copy_ev, c->copy_stream));
    // (the completion marker for vcfxg_ingest_wait: recorded on the copy stream)
    hipEvent_t e = nullptr;
    if (!c->ingest_ev_free.empty()) {
        e = c->ingest_ev_free.back();
        c->ingest_ev_free.pop_back();
    } else {
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIPCHK(c, hipEventRecord(e, c->copy_stream));
    c->ingest_ev.push_back({offset + n, e});
    return VCFXG_OK;
}

// launch the inflate of members [first, first + count) of the staged stream: their table entries
// and output offsets (from the running output count) to the device, k_inflate after the copies
// staged so far
// the token buffer of stream slot k (kBgzStreams: c->stream) for `count` members: at most 69,632 at
// a time (2.3 GB: the bench shard's 65,834 members in one launch), fewer when the device cannot
// spare that (down to 4,096; launches of more members run in pieces); 0 members when even that
// cannot be had (every member then on the wave decoder)
static uint64_t bgz_tokens(vcfxg_ctx *c, int k, uint64_t count, hipStream_t st) {
    DevBuf &b = c->bgz_tok[k];
    const size_t per = (size_t)vcfxg::kTokCap * 4 + 4;  // (the tokens, and a hand-over list entry)
    for (uint64_t want = std::min<uint64_t>(count, 69632);; want /= 2) {
        if (b.cap >= want * per + 4) return want;
        if (b.p) {  // (the stream's earlier batches may still read it)
            if (hipStreamSynchronize(st) != hipSuccess) return 0;
            (void)b.release();
        }
        // (rounded up to 8,192 members: a batch a few members past the last one's size reuses it)
        const uint64_t alloc = std::min<uint64_t>((want + 8191) / 8192 * 8192, std::max<uint64_t>(want, 69632));
        if (b.alloc(alloc * per + 4) == hipSuccess) return want;
        (void)hipGetLastError();
        if (want <= 4096) return 0;
    }
}

// the lane decoder's member order for `count` members: largest compressed first (a counting sort
// on 64-byte buckets: the lanes of a wave then decode similar amounts, and the largest go first)
static std::vector<uint32_t> bgz_order(const vcfxg_bgzf_member *mem, uint64_t count) {
    constexpr uint32_t kB = 1026;  // (src_len <= 65,536 + header slack: buckets of 64 B)
    std::vector<uint32_t> cnt(kB + 1, 0), perm(count);
    auto bucket = [&](uint64_t i) { return kB - 1 - std::min<uint32_t>(mem[i].src_len >> 6, kB - 1); };
    for (uint64_t i = 0; i < count; i++) cnt[bucket(i) + 1]++;
    for (uint32_t b = 0; b < kB; b++) cnt[b + 1] += cnt[b];
    for (uint64_t i = 0; i < count; i++) perm[cnt[bucket(i)]++] = (uint32_t)i;
    return perm;
}

// the lane decoder's side stream and events (created once)
static int bgz_aux(vcfxg_ctx *c) {
    vcfxg::InflateSide &d = c->bgz_side;
    if (!d.aux) HIPCHK(c, hipStreamCreateWithFlags(&d.aux, hipStreamNonBlocking));
    for (hipEvent_t &e : d.ev)
        if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return VCFXG_OK;
}

// the CRC-32 pass's "1 KiB of zeros" basis
static const vcfxg::Crc1k &crc_basis() {
    static const vcfxg::Crc1k z = [] {
        vcfxg::Crc1k b;
        vcfxg::crc32_zero1k_basis(&b);
        return b;
    }();
    return z;
}

// members [first, first + count) of a staged stream: the tables, the inflate and its CRC-32 pass
// on `st` (so the last batch's check does not wait for a pass over every member)
static int bgz_launch(vcfxg_ctx *c, const vcfxg_bgzf_member *mem, uint64_t first, uint64_t count,
                      hipStream_t st, int slot) {
    if (!count) return VCFXG_OK;
    const std::vector<uint32_t> perm = bgz_order(mem, count);
    HIPCHK(c, hipMemcpyAsync(P<uint32_t>(c->bgz_perm) + first, perm.data(), 4 * count, hipMemcpyHostToDevice, st));
    std::vector<uint64_t> off(count);
    uint64_t o = c->bgz_out;
    for (uint64_t i = 0; i < count; i++) {
        off[i] = o;
        o += mem[i].out_len;
    }
    HIPCHK(c, hipMemcpyAsync(P<vcfxg_bgzf_member>(c->bgz_mem) + first, mem, sizeof(vcfxg_bgzf_member) * count,
                             hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(P<uint64_t>(c->bgz_off) + first, off.data(), 8 * count, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamWaitEvent(st, c->bgz_copy_ev, 0));
    const uint64_t tm = bgz_tokens(c, slot, count, st);
    if (int r = bgz_aux(c)) return r;
    for (int which = 0; which < 2; which++)
        HIPCHK(c, vcfxg::launch_inflate(which, P<uint8_t>(c->bgz_in), P<vcfxg::BgzfMember>(c->bgz_mem) + first,
                                        P<uint64_t>(c->bgz_off) + first, count, P<uint8_t>(c->input) + c->n,
                                        P<uint32_t>(c->bgz_stat) + first, P<unsigned long long>(c->bgz_small),
                                        crc_basis(), st, first, P<uint32_t>(c->bgz_tok[slot]), tm,
                                        P<uint32_t>(c->bgz_perm) + first, &c->bgz_side));
    c->bgz_launched = first + count;
    c->bgz_out = o;
    return VCFXG_OK;
}

int vcfxg_bgzf_inflate(vcfxg_ctx *c, const vcfxg_bgzf_member *mem, size_t count) {
    if (!c || (!mem && count)) return VCFXG_E_ARG;
    if (!c->ingesting || !c->bgz_total) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t out = 0;
    for (size_t i = 0; i < count; i++) {
        if (mem[i].src_off > c->bgz_staged || mem[i].src_len > c->bgz_staged - mem[i].src_off || mem[i].src_len < 20 ||
            mem[i].out_len > 65536)
            return VCFXG_E_ARG;  // (not staged yet, or out of range)
        out += mem[i].out_len;
    }
    if (c->bgz_launched + count > bgz_max_members(c->bgz_total)) return VCFXG_E_ARG;
    if (c->bgz_launched + count + 1 > bgz_table_members(c)) return VCFXG_E_CAP;  // (the rest at the end)
    // the output must fit the input buffer as it is (growing it here would move the bytes the
    // launched batches are writing): the rest waits for vcfxg_ingest_bgzf, which grows it
    if (c->n + c->bgz_out + out + kPad > c->input.cap) return VCFXG_E_CAP;
    const int k = c->bgz_next;
    c->bgz_next = (k + 1) % vcfxg_ctx::kBgzStreams;
    int r = bgz_launch(c, mem, c->bgz_launched, count, c->bgz_stream[k], k);
    if (r) return r;
    HIPCHK(c, hipEventRecord(c->bgz_ev[k], c->bgz_stream[k]));
    return VCFXG_OK;
}

int vcfxg_ingest_bgzf(vcfxg_ctx *c, const void *comp, size_t comp_n, const vcfxg_bgzf_member *mem, size_t nm,
                      const char *head, size_t head_n, uint64_t *bad_member) {
    // comp = NULL: the compressed bytes were staged by vcfxg_bgzf_stage (all comp_n of them), and
    // members [0, bgz_launched) were launched by vcfxg_bgzf_inflate (mem[] must begin with them)
    const bool staged = !comp;
    if (!c || (staged && comp_n && (c->bgz_total != comp_n || c->bgz_staged != comp_n)) || (!mem && nm) ||
        (!head && head_n))
        return VCFXG_E_ARG;
    if (!c->ingesting) return VCFXG_E_STATE;
    if (bad_member) *bad_member = ~0ull;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t done = staged ? c->bgz_launched : 0;  // members launched already
    if (done > nm || (staged && nm > bgz_max_members(comp_n))) return VCFXG_E_ARG;
    std::vector<uint64_t> off(nm + 1);
    uint64_t tot = 0;
    for (size_t i = 0; i < nm; i++) {
        // (the kernel reads the header's XLEN and the trailer inside the member)
        if (mem[i].src_off > comp_n || mem[i].src_len > comp_n - mem[i].src_off || mem[i].src_len < 20 ||
            mem[i].out_len > 65536) {
            c->err = "vcfxg_ingest_bgzf: member " + std::to_string(i) + " out of range";
            return VCFXG_E_ARG;
        }
        off[i] = tot;
        tot += mem[i].out_len;
    }
    off[nm] = tot;
    if (staged && done && off[done] != c->bgz_out) return VCFXG_E_ARG;  // (not the launched members)
    if (staged) {
        // every staged copy and every launched batch before anything below (the grow copies the
        // batches' output; the kernels below read the staged bytes)
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->bgz_copy_ev, 0));
        if (done)
            for (int k = 0; k < vcfxg_ctx::kBgzStreams; k++) HIPCHK(c, hipStreamWaitEvent(c->stream, c->bgz_ev[k], 0));
        if (int rt = bgz_tables(c, nm + 1, done)) return rt;  // (more members than the stage sized for)
    }
    if (c->n + tot + kPad > c->input.cap) {  // grow as vcfxg_ingest does (keeping launched output)
        const size_t keep = c->n + (size_t)(staged ? c->bgz_out : 0);
        const int rg = regrow(c, c->input, std::max(c->input.cap * 2, c->n + tot + kPad), keep);
        if (rg) return rg;
    }
    int r = VCFXG_OK;
    if (!staged) {
        r = ensure(c, c->bgz_in, comp_n + kCompPad);
        if (!r) r = ensure(c, c->bgz_mem, sizeof(vcfxg_bgzf_member) * (nm + 1));
        if (!r) r = ensure(c, c->bgz_off, 8 * (nm + 1));
        if (!r) r = ensure(c, c->bgz_stat, 4 * (nm + 1));
        if (!r) r = ensure(c, c->bgz_small, 64);
        if (!r) r = ensure(c, c->bgz_perm, 4 * (nm + 1));
        if (r) return r;
    }
    const vcfxg::Crc1k &z1k = crc_basis();
    if (staged) {
        // the members not launched yet
        prof_begin(c, "bgzf_inflate");
        r = bgz_launch(c, mem + done, done, nm - done, c->stream, vcfxg_ctx::kBgzStreams);
        prof_end(c, "bgzf_inflate");
        if (r) return r;
    } else {
        prof_begin(c, "bgzf_h2d");
        if (comp_n) HIPCHK(c, hipMemcpyAsync(c->bgz_in.p, comp, comp_n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(P<uint8_t>(c->bgz_in) + comp_n, 0, kCompPad, c->stream));
        if (nm) {
            HIPCHK(c, hipMemcpyAsync(c->bgz_mem.p, mem, sizeof(vcfxg_bgzf_member) * nm, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->bgz_off.p, off.data(), 8 * nm, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, hipMemsetAsync(c->bgz_small.p, 0xFF, 8, c->stream));
        HIPCHK(c, hipMemsetAsync(P<uint8_t>(c->bgz_small) + 8, 0, 56, c->stream));
        prof_end(c, "bgzf_h2d");
        const uint64_t tm = bgz_tokens(c, vcfxg_ctx::kBgzStreams, nm, c->stream);
        if (int ra = bgz_aux(c)) return ra;
        const std::vector<uint32_t> perm = bgz_order(mem, nm);
        if (nm) HIPCHK(c, hipMemcpyAsync(c->bgz_perm.p, perm.data(), 4 * nm, hipMemcpyHostToDevice, c->stream));
        prof_begin(c, "bgzf_inflate");
        HIPCHK(c, vcfxg::launch_inflate(0, P<uint8_t>(c->bgz_in), P<vcfxg::BgzfMember>(c->bgz_mem),
                                        P<uint64_t>(c->bgz_off), nm, P<uint8_t>(c->input) + c->n,
                                        P<uint32_t>(c->bgz_stat), P<unsigned long long>(c->bgz_small), z1k, c->stream, 0,
                                        P<uint32_t>(c->bgz_tok[vcfxg_ctx::kBgzStreams]), tm, P<uint32_t>(c->bgz_perm), &c->bgz_side));
        prof_end(c, "bgzf_inflate");
    }
    prof_begin(c, "bgzf_crc32");
    if (!staged)  // (a staged stream's batches checked their own members, bgz_launch)
        HIPCHK(c, vcfxg::launch_inflate(1, P<uint8_t>(c->bgz_in), P<vcfxg::BgzfMember>(c->bgz_mem),
                                        P<uint64_t>(c->bgz_off), nm, P<uint8_t>(c->input) + c->n,
                                        P<uint32_t>(c->bgz_stat), P<unsigned long long>(c->bgz_small), z1k, c->stream));
    prof_end(c, "bgzf_crc32");
    // the first bad member, the hand-over count and its reasons (32-bit words 3..14)
    static thread_local uint64_t small[8];
    static thread_local uint8_t lastb;
    uint64_t &bad = small[0];
    HIPCHK(c, hipMemcpyAsync(small, c->bgz_small.p, 64, hipMemcpyDeviceToHost, c->stream));
    if (tot) HIPCHK(c, hipMemcpyAsync(&lastb, P<uint8_t>(c->input) + c->n + tot - 1, 1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->bgz_total = c->bgz_staged = 0;
    c->bgz_launched = c->bgz_out = 0;
    c->bgz_handed = (uint32_t)small[1];
    if (c->bgz_handed && getenv("VCFX_BGZF_DIAG")) {  // (why the lane decoder handed members over)
        const uint32_t *w = reinterpret_cast<const uint32_t *>(small) + 2;
        fprintf(stderr, "vcfxg: BGZF members handed to the wave decoder: %u (by reason 1-12:", w[0]);
        for (int k = 1; k <= 12; k++) fprintf(stderr, " %u", w[k]);
        fprintf(stderr, ")\n");
    }
    if (bad != ~0ull) {
        uint32_t why = 0;
        (void)hipMemcpy(&why, P<uint32_t>(c->bgz_stat) + bad, 4, hipMemcpyDeviceToHost);
        if (bad_member) *bad_member = bad;
        c->err = "BGZF member " + std::to_string(bad) + " does not inflate (check " + std::to_string(why) + ")";
        c->ingesting = false;
        c->loaded = false;
        c->n = 0;
        return VCFXG_E_DATA;
    }
    if (head_n && c->hints_pending) c->hints_pending = !load_hints(c, head, head_n);
    note_schedule(c, staged ? "bgzf_inflate_staged" : "bgzf_inflate");
    c->n += tot;
    if (tot) c->last_byte = lastb;
    return VCFXG_OK;
}

}  // extern "C"
