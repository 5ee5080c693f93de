// vcfxg_api.hip -- the C ABI (include/vcfx_gpu.h): device context, profiling, device-resident
// input and its line index, the fetch calls, and the helpers every vcfxg_api_*.hip unit uses
// (vcfxg_ctx.h); the tools' calls, sequenced on the context's one HIP stream, are in those units.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <fcntl.h>
#include <unistd.h>

#include "vcfxg_ctx.h"
#include "vcfxg_ld.h"  // (the MFMA self-tests' launchers)

namespace vcfxg {

int fail(vcfxg_ctx *c, hipError_t e, const char *what) {
    if (c) {
        c->err = std::string(what) + ": " + hipGetErrorString(e);
    }
    return e == hipErrorOutOfMemory ? VCFXG_E_NOMEM : VCFXG_E_HIP;
}

int ensure(vcfxg_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return VCFXG_OK;
    size_t nc = bytes < 4096 ? 4096 : bytes + bytes / 8;
    if (b.p) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, b.release());
    }
    HIPCHK(c, b.alloc(nc));
    return VCFXG_OK;
}

int regrow(vcfxg_ctx *c, DevBuf &b, size_t bytes, size_t keep) {
    DevBuf nb;
    HIPCHK(c, nb.alloc(bytes));
    if (keep && b.p) HIPCHK(c, hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, b.release());
    b = std::move(nb);
    return VCFXG_OK;
}

static hipEvent_t prof_event(vcfxg_ctx *c) {
    hipEvent_t e = nullptr;
    if (!c->ev_free.empty()) {
        e = c->ev_free.back();
        c->ev_free.pop_back();
    } else {
        (void)hipEventCreate(&e);
    }
    return e;
}
static bool prof_on(vcfxg_ctx *c, const char *name) {
    return c->profiling && (c->prof_only.empty() || c->prof_only == name);
}
void prof_begin(vcfxg_ctx *c, const char *name) {
    if (!prof_on(c, name)) return;
    hipEvent_t e = prof_event(c);
    (void)hipEventRecord(e, c->stream);
    c->ev_open.push_back({name, e, nullptr});
}
void prof_end(vcfxg_ctx *c, const char *name) {
    if (!prof_on(c, name)) return;
    for (size_t k = c->ev_open.size(); k-- > 0;) {
        if (strcmp(c->ev_open[k].name, name)) continue;
        vcfxg_ctx::ProfRec r = c->ev_open[k];
        c->ev_open.erase(c->ev_open.begin() + k);
        r.b = prof_event(c);
        (void)hipEventRecord(r.b, c->stream);
        c->pending.push_back(r);
        return;
    }
}
// elapsed times of the recorded launches (synchronises with the stream first)
static void prof_harvest(vcfxg_ctx *c) {
    if (c->pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto &r : c->pending) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
            c->ms[r.name] = t;
            auto &a = c->acc[r.name];
            a.first += t;
            a.second += 1;
        }
        c->ev_free.push_back(r.a);
        c->ev_free.push_back(r.b);
    }
    c->pending.clear();
}
// after a call: harvest only when many launches are pending (bounded event pool)
void prof_collect(vcfxg_ctx *c) {
    if (c->pending.size() >= 4096) prof_harvest(c);
}

template <typename InT>
static int scan_of(vcfxg_ctx *c, const InT *in, uint64_t *out, size_t n) {
    size_t tmp = 0;
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, in, out, (int)n, c->stream));
    int r = ensure(c, c->scan_tmp, tmp);
    if (r) return r;
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(c->scan_tmp.p, tmp, in, out, (int)n, c->stream));
    return VCFXG_OK;
}
// (the only unit that instantiates the hipcub scans of plain arrays: LD has its iterator scans)
int exclusive_scan(vcfxg_ctx *c, const uint32_t *in, uint64_t *out, size_t n) { return scan_of(c, in, out, n); }
int exclusive_scan(vcfxg_ctx *c, const uint64_t *in, uint64_t *out, size_t n) { return scan_of(c, in, out, n); }

// the schedule a region call took (vcfxg_last_schedule; VCFXG_SCHEDULE_LOG=path appends one
// line per call: tests check which path sharded ranks and fresh contexts run)
void note_schedule(vcfxg_ctx *c, const char *what) {
    c->last_schedule = what;
    const char *log = getenv("VCFXG_SCHEDULE_LOG");  // (read per call: tests set it in-process)
    if (!log) return;
    const int fd = ::open(log, O_WRONLY | O_APPEND | O_CREAT | O_CLOEXEC, 0644);
    if (fd < 0) return;
    const std::string l = std::string(what) + "\n";
    (void)!::write(fd, l.data(), l.size());
    ::close(fd);
}

// the walk paths' hints from the host bytes of the input's first chunk holding data lines:
// skip '#' lines, then the first data line's '\n' distance from the byte after its 9th tab and
// the mean length of up to 256 lines.  Called on each ingested chunk until one holds data: a
// chunk of '#' lines only that ends at a line end (a shard view's header [0, H), a pipe's head)
// returns false and the next chunk is looked at.  Chunks are read while the caller still owns
// them (a pipe's staging slot is reused after the call).
bool load_hints(vcfxg_ctx *c, const char *h, size_t n) {
    size_t p = 0;
    while (p < n && h[p] == '#') {
        const void *q = memchr(h + p, '\n', n - p);
        if (!q) return true;  // a '#' line cut by the chunk end: no hints
        p = (size_t)((const char *)q - h) + 1;
    }
    if (p >= n) return false;  // header lines only: the data starts in a later chunk
    const size_t first = p;
    int lines = 0;
    while (p < n && lines < 256) {
        const char *q = (const char *)memchr(h + p, '\n', n - p);
        const size_t e = q ? (size_t)(q - h) : n;
        if (lines == 0) {
            int tabs = 0;
            size_t x = p, f8 = 0;
            while (x < e && tabs < 9) {
                const char *t = (const char *)memchr(h + x, '\t', e - x);
                if (!t) break;
                if (tabs == 8) {
                    c->hint_gt_only = (size_t)(t - h) - f8 == 2 && h[f8] == 'G' && h[f8 + 1] == 'T';
                    c->hint_gt_first = (size_t)(t - h) - f8 > 3 && h[f8] == 'G' && h[f8 + 1] == 'T' && h[f8 + 2] == ':';
                }
                x = (size_t)(t - h) + 1;
                tabs++;
                if (tabs == 8) f8 = x;
            }
            if (tabs == 9) c->hint_span = (int64_t)(e - x);
        }
        lines++;
        p = e + 1;
    }
    if (lines) c->hint_line = (int64_t)((std::min(p, n) - first) / (size_t)lines);
    // the walkers' chunk: 128 KiB, or about 12 records (rounded up to 64 KiB, at most 4 MiB) for
    // records over 16 KiB: each walker's two backward boundary scans read about one record, so
    // long records want longer chunks (GT:AD:DP, 30 KB records: 128 KiB 5.03 ms, 512 KiB 4.76,
    // 1 MiB 5.10; r03 sweep; r05, XCD-contiguous walker blocks: 256 KiB 3.73 ms, 384 KiB 3.65,
    // 512 KiB 3.69, 768 KiB 3.89).  VCFXG_WALK_CHUNK overrides.
    if (!c->walk_chunk_forced)
        c->walk_chunk = c->hint_line > 16 * 1024
                            ? std::min<int64_t>(((12 * c->hint_line + 65535) / 65536) * 65536, 4 << 20)
                            : 128 * 1024;
    return true;
}

}  // namespace vcfxg

using namespace vcfxg;

extern "C" {

const char *vcfxg_version(void) { return "vcfx_amd 0.1 (gfx950)"; }

int vcfxg_device_count(int *n) {
    int k = 0;
    if (hipGetDeviceCount(&k) != hipSuccess) k = 0;
    if (n) *n = k;
    return VCFXG_OK;
}

int vcfxg_open(int device, vcfxg_ctx **out) {
    if (!out) return VCFXG_E_ARG;
    *out = nullptr;
    int k = 0;
    if (hipGetDeviceCount(&k) != hipSuccess || k <= 0 || device < 0 || device >= k) return VCFXG_E_NODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return VCFXG_E_NODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return VCFXG_E_NODEV;
    vcfxg_ctx *c = new vcfxg_ctx();
    c->device = device;
    c->n_cu = prop.multiProcessorCount;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return VCFXG_E_HIP;
    }
    int r = ensure(c, c->d_nlines, 64);
    if (!r) r = ensure(c, c->counters, 64);
    if (r) {
        vcfxg_close(c);
        return r;
    }
    *out = c;
    return VCFXG_OK;
}

// (the device made current and the stream drained here, the buffers freed by their owners when the
// context is deleted at the end)
void vcfxg_close(vcfxg_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->sum_host) (void)hipHostFree(c->sum_host);
    for (auto &pe : c->ingest_ev) (void)hipEventDestroy(pe.second);
    for (hipEvent_t e : c->ingest_ev_free) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_free) (void)hipEventDestroy(e);
    for (auto &r : c->pending) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto &r : c->ev_open) (void)hipEventDestroy(r.a);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (int k = 0; k < vcfxg_ctx::kBgzStreams; k++) {
        if (c->bgz_stream[k]) (void)hipStreamDestroy(c->bgz_stream[k]);
        if (c->bgz_ev[k]) (void)hipEventDestroy(c->bgz_ev[k]);
    }
    if (c->bgz_copy_ev) (void)hipEventDestroy(c->bgz_copy_ev);
    if (c->bgz_side.aux) (void)hipStreamDestroy(c->bgz_side.aux);
    for (hipEvent_t e : c->bgz_side.ev)
        if (e) (void)hipEventDestroy(e);
    delete c;
}

uint64_t vcfxg_device_bytes_live(void) { return DevBuf::live.load(); }

const char *vcfxg_last_error(const vcfxg_ctx *c) { return c ? c->err.c_str() : "no context"; }
void *vcfxg_stream(vcfxg_ctx *c) { return c ? (void *)c->stream : nullptr; }

int vcfxg_set_profiling(vcfxg_ctx *c, int enable) {
    if (!c) return VCFXG_E_ARG;
    c->profiling = enable != 0;
    return VCFXG_OK;
}

int vcfxg_set_profiling_only(vcfxg_ctx *c, const char *kernel) {
    if (!c) return VCFXG_E_ARG;
    c->prof_only = kernel ? kernel : "";
    return VCFXG_OK;
}

int vcfxg_kernel_ms(vcfxg_ctx *c, const char *kernel, float *ms) {
    if (!c || !kernel || !ms) return VCFXG_E_ARG;
    prof_harvest(c);
    auto it = c->ms.find(kernel);
    if (it == c->ms.end()) return VCFXG_E_STATE;
    *ms = it->second;
    return VCFXG_OK;
}

int vcfxg_kernel_stats(vcfxg_ctx *c, const char *kernel, double *total_ms, uint64_t *launches) {
    if (!c || !kernel) return VCFXG_E_ARG;
    prof_harvest(c);
    auto it = c->acc.find(kernel);
    if (total_ms) *total_ms = it == c->acc.end() ? 0.0 : it->second.first;
    if (launches) *launches = it == c->acc.end() ? 0 : it->second.second;
    return VCFXG_OK;
}

int vcfxg_reset_kernel_stats(vcfxg_ctx *c) {
    if (!c) return VCFXG_E_ARG;
    prof_harvest(c);
    c->acc.clear();
    return VCFXG_OK;
}

static void reset_hints(vcfxg_ctx *c) {
    c->hint_span = 0;
    c->hint_line = 0;
    c->hint_gt_only = false;
    c->hint_gt_first = false;
    c->walk_overflowed = false;
    c->dose_head_failed = false;
    c->ph_head_failed = false;
    if (!c->walk_chunk_forced) c->walk_chunk = 128 * 1024;
}

int vcfxg_load_host(vcfxg_ctx *c, const char *host, size_t n) {
    if (!c || (!host && n)) return VCFXG_E_ARG;
    int r = vcfxg_ingest_begin(c, n);
    if (!r) r = vcfxg_ingest(c, host, n, 1);
    return r;
}

int vcfxg_ingest_begin(vcfxg_ctx *c, size_t size_hint) {
    if (!c) return VCFXG_E_ARG;
    new_index(c);
    HIPCHK(c, hipSetDevice(c->device));
    // (a staged BGZF stream abandoned before vcfxg_ingest_bgzf may still have copies and inflate
    // batches in flight on their own streams: they finish before the input is written again)
    if (c->copy_stream) HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    for (int k = 0; k < vcfxg_ctx::kBgzStreams; k++)
        if (c->bgz_stream[k]) HIPCHK(c, hipStreamSynchronize(c->bgz_stream[k]));
    if (c->bgz_side.aux) HIPCHK(c, hipStreamSynchronize(c->bgz_side.aux));
    c->bgz_total = c->bgz_staged = 0;
    // (a hint past half of the memory the input could take -- free memory plus its buffer now --
    // is cut to that half: the walk's, LD's and the inflate's buffers keep the rest, and the
    // ingest grows the buffer if the bytes need more)
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && size_hint > (fr + c->input.cap) / 2)
        size_hint = (fr + c->input.cap) / 2;
    int r = ensure(c, c->input, size_hint + kPad);
    if (r) return r;
    c->loaded = false;
    c->indexed = false;
    c->n = 0;
    c->ingesting = true;
    reset_hints(c);
    c->hints_pending = true;
    return VCFXG_OK;
}

static int ingest_mark(vcfxg_ctx *c, size_t upto);

int vcfxg_ingest(vcfxg_ctx *c, const char *host, size_t n, int is_final_chunk) {
    if (!c || (!host && n)) return VCFXG_E_ARG;
    if (!c->ingesting) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n + n + kPad > c->input.cap) {
        // grow: a larger buffer, the bytes so far copied on the device
        const int r = regrow(c, c->input, std::max(c->input.cap * 2, c->n + n + kPad), c->n);
        if (r) return r;
    }
    // pageable host memory: the runtime's staged DMA runs at the PCIe rate (measured
    // 50-56 GB/s on MI355X, tools/microbench/h2d_ingest.cpp), asynchronous to the caller
    // up to its staging depth
    if (n) HIPCHK(c, hipMemcpyAsync(static_cast<char *>(c->input.p) + c->n, host, n, hipMemcpyHostToDevice, c->stream));
    if (n && !is_final_chunk) {  // completion marker for vcfxg_ingest_wait
        int r = ingest_mark(c, c->n + n);
        if (r) return r;
    }
    if (n && c->hints_pending) c->hints_pending = !load_hints(c, host, n);
    c->n += n;
    if (n) c->last_byte = (unsigned char)host[n - 1];
    if (!is_final_chunk) return VCFXG_OK;
    if (!c->n) c->last_byte = -1;
    HIPCHK(c, hipMemsetAsync(static_cast<char *>(c->input.p) + c->n, 0, kPad, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &pe : c->ingest_ev) c->ingest_ev_free.push_back(pe.second);
    c->ingest_ev.clear();
    c->hints_pending = false;
    c->ingesting = false;
    c->loaded = true;
    c->indexed = false;
    return VCFXG_OK;
}

// a completion marker for vcfxg_ingest_wait at stream offset `upto`
static int ingest_mark(vcfxg_ctx *c, size_t upto) {
    hipEvent_t e = nullptr;
    if (!c->ingest_ev_free.empty()) {
        e = c->ingest_ev_free.back();
        c->ingest_ev_free.pop_back();
    } else {
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIPCHK(c, hipEventRecord(e, c->stream));
    c->ingest_ev.push_back({upto, e});
    return VCFXG_OK;
}

int vcfxg_ingest_wait(vcfxg_ctx *c, size_t upto) {
    if (!c) return VCFXG_E_ARG;
    size_t k = 0;
    while (k < c->ingest_ev.size() && c->ingest_ev[k].first <= upto) k++;
    if (k == 0) return VCFXG_OK;
    HIPCHK(c, hipEventSynchronize(c->ingest_ev[k - 1].second));
    for (size_t i = 0; i < k; i++) c->ingest_ev_free.push_back(c->ingest_ev[i].second);
    c->ingest_ev.erase(c->ingest_ev.begin(), c->ingest_ev.begin() + (long)k);
    return VCFXG_OK;
}

int vcfxg_count_byte(vcfxg_ctx *c, uint64_t from, int byte, uint64_t *count) {
    if (!c || !count || byte < 0 || byte > 255) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    HIPCHK(c, hipSetDevice(c->device));
    *count = 0;
    if (from >= c->n) return VCFXG_OK;
    int r = ensure(c, c->byte_cnt, 8);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->byte_cnt.p, 0, 8, c->stream));
    prof_begin(c, "count_byte");
    HIPCHK(c, vcfxg::launch_count_byte(P<uint8_t>(c->input), from, c->n, (uint8_t)byte,
                                       P<unsigned long long>(c->byte_cnt), c->stream));
    prof_end(c, "count_byte");
    static thread_local uint64_t h;
    HIPCHK(c, hipMemcpyAsync(&h, c->byte_cnt.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    *count = h;
    return VCFXG_OK;
}

int vcfxg_host_alloc(vcfxg_ctx *c, size_t n, void **out) {
    if (!c || !out) return VCFXG_E_ARG;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipHostMalloc(out, n ? n : 1, hipHostMallocDefault));
    return VCFXG_OK;
}

void vcfxg_host_free(vcfxg_ctx *c, void *p) {
    if (c && p) (void)hipHostFree(p);
}

int vcfxg_input_fetch(vcfxg_ctx *c, uint64_t offset, size_t n, void *host) {
    if (!c || (!host && n)) return VCFXG_E_ARG;
    if (!c->loaded) return VCFXG_E_STATE;
    if (offset > c->n || n > c->n - offset) return VCFXG_E_ARG;
    if (!n) return VCFXG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host, static_cast<const char *>(c->input.p) + offset, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

const void *vcfxg_input_device_ptr(vcfxg_ctx *c) { return c && c->loaded ? c->input.p : nullptr; }

int vcfxg_index(vcfxg_ctx *c, size_t data_start, uint64_t *n_lines) {
    if (!c) return VCFXG_E_ARG;
    new_index(c);
    if (!c->loaded) return VCFXG_E_STATE;
    if (data_start > c->n) data_start = c->n;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t lo = (int64_t)data_start, hi = (int64_t)c->n;
    const int64_t nc = vcfxg::idx_wchunks(lo, hi);
    int r = ensure(c, c->idx_counts, sizeof(uint32_t) * (size_t)(nc + 1));
    if (!r) r = ensure(c, c->idx_offs, sizeof(uint64_t) * (size_t)(nc + 1));
    if (!r) r = ensure(c, c->idx_pos, sizeof(uint64_t) * (size_t)nc * vcfxg::idx_pos_cap() + 64);
    if (r) return r;
    const char *buf = P<char>(c->input);
    unsigned *overflow = reinterpret_cast<unsigned *>(P<uint64_t>(c->idx_pos) + (size_t)nc * vcfxg::idx_pos_cap());
    HIPCHK(c, hipMemsetAsync(overflow, 0, 8, c->stream));
    prof_begin(c, "line_count");
    HIPCHK(c, vcfxg::launch_idx_count(buf, lo, hi, P<uint32_t>(c->idx_counts), P<uint64_t>(c->idx_pos), overflow,
                                      c->stream));
    prof_end(c, "line_count");
    HIPCHK(c, hipMemsetAsync(P<uint32_t>(c->idx_counts) + nc, 0, sizeof(uint32_t), c->stream));
    r = exclusive_scan(c, P<uint32_t>(c->idx_counts), P<uint64_t>(c->idx_offs), (size_t)nc + 1);
    if (r) return r;
    static thread_local uint64_t total;
    static thread_local unsigned ovf;
    HIPCHK(c, hipMemcpyAsync(&total, P<uint64_t>(c->idx_offs) + nc, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&ovf, overflow, sizeof ovf, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool tail = hi > lo && c->last_byte != '\n';
    const uint64_t nl = total + (tail ? 1 : 0);
    r = ensure(c, c->line_end, sizeof(uint64_t) * (size_t)(nl + 1));
    if (r) return r;
    if (ovf) {  // some chunk has more newlines than the scratch holds: the emit sweep
        prof_begin(c, "line_emit");
        HIPCHK(c, vcfxg::launch_idx_emit(buf, lo, hi, P<uint64_t>(c->idx_offs), P<uint64_t>(c->line_end), c->stream));
        prof_end(c, "line_emit");
    } else {
        prof_begin(c, "line_compact");
        HIPCHK(c, vcfxg::launch_nl_compact(lo, hi, P<uint32_t>(c->idx_counts), P<uint64_t>(c->idx_offs),
                                           P<uint64_t>(c->idx_pos), P<uint64_t>(c->line_end), c->stream));
        prof_end(c, "line_compact");
    }
    static thread_local uint64_t tail_end, nl_host;
    tail_end = (uint64_t)hi;
    nl_host = nl;
    if (tail)
        HIPCHK(c, hipMemcpyAsync(P<uint64_t>(c->line_end) + total, &tail_end, sizeof(uint64_t), hipMemcpyHostToDevice,
                                 c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_nlines.p, &nl_host, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->data_start = data_start;
    c->n_lines = nl;
    c->indexed = true;
    if (n_lines) *n_lines = nl;
    return VCFXG_OK;
}

int vcfxg_line_ends(vcfxg_ctx *c, uint64_t first, uint64_t count, uint64_t *out) {
    if (!c || (!out && count)) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    if (first + count > c->n_lines) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    HIPCHK(c, hipMemcpyAsync(out, P<uint64_t>(c->line_end) + first, count * sizeof(uint64_t), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_selftest_mfma_i8(vcfxg_ctx *c, int *mismatches) {
    if (!c || !mismatches) return VCFXG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int8_t> A(32 * 32), B(32 * 32);
    for (int i = 0; i < 32 * 32; i++) {
        A[i] = (int8_t)((i * 7 + 3) % 5 - 2);
        B[i] = (int8_t)((i * 11 + 1) % 7 - 3);
    }
    int r = ensure(c, c->scan_tmp, 8192);
    if (r) return r;
    char *d = P<char>(c->scan_tmp);
    HIPCHK(c, hipMemcpyAsync(d, A.data(), 1024, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + 1024, B.data(), 1024, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, vcfxg::launch_mfma_i8_selftest((int8_t *)d, (int8_t *)(d + 1024), (int *)(d + 2048), c->stream));
    std::vector<int> C(32 * 32);
    HIPCHK(c, hipMemcpyAsync(C.data(), d + 2048, 4096, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int bad = 0;
    for (int i = 0; i < 32; i++)
        for (int j = 0; j < 32; j++) {
            int s = 0;
            for (int k = 0; k < 32; k++) s += A[i * 32 + k] * B[j * 32 + k];
            bad += s != C[i * 32 + j];
        }
    *mismatches = bad;
    return VCFXG_OK;
}

int vcfxg_selftest_mfma_fp4(vcfxg_ctx *c, int *mismatches) {
    if (!c || !mismatches) return VCFXG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    // dosages 0..2 in a 32x64 A and an asymmetric 32x64 B, packed e2m1 two per byte
    std::vector<int> A(32 * 64), B(32 * 64);
    for (int i = 0; i < 32 * 64; i++) {
        A[i] = (i * 7 + 3) % 3;
        B[i] = (i * 11 + i / 64 + 1) % 3;
    }
    std::vector<uint8_t> Ap(1024), Bp(1024);
    for (int i = 0; i < 1024; i++) {
        Ap[i] = (uint8_t)((2 * A[2 * i]) | ((2 * A[2 * i + 1]) << 4));
        Bp[i] = (uint8_t)((2 * B[2 * i]) | ((2 * B[2 * i + 1]) << 4));
    }
    int r = ensure(c, c->scan_tmp, 8192);
    if (r) return r;
    char *d = P<char>(c->scan_tmp);
    HIPCHK(c, hipMemcpyAsync(d, Ap.data(), 1024, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + 1024, Bp.data(), 1024, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, vcfxg::launch_mfma_f4_selftest((uint8_t *)d, (uint8_t *)(d + 1024), (float *)(d + 2048), c->stream));
    std::vector<float> C(32 * 32);
    HIPCHK(c, hipMemcpyAsync(C.data(), d + 2048, 4096, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int bad = 0;
    for (int i = 0; i < 32; i++)
        for (int j = 0; j < 32; j++) {
            int sum = 0;
            for (int k = 0; k < 64; k++) sum += A[i * 64 + k] * B[j * 64 + k];
            bad += (float)sum != C[i * 32 + j];
        }
    *mismatches = bad;
    return VCFXG_OK;
}

int vcfxg_fetch_text(vcfxg_ctx *c, char *host, size_t cap) {
    if (!c || (!host && c->text_bytes)) return VCFXG_E_ARG;
    if (cap < c->text_bytes) return VCFXG_E_CAP;
    if (!c->text_bytes) return VCFXG_OK;
    HIPCHK(c, hipMemcpyAsync(host, c->text.p, c->text_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_shard_cuts(const char *data, size_t n, size_t lo, int world, uint64_t *cuts) {
    if ((!data && n) || world < 1 || !cuts || lo > n) return VCFXG_E_ARG;
    cuts[0] = lo;
    for (int i = 1; i < world; i++) {
        size_t p = lo + (size_t)((unsigned __int128)(n - lo) * (unsigned)i / (unsigned)world);
        if (p < cuts[i - 1]) p = cuts[i - 1];
        if (p > lo && p < n && data[p - 1] != '\n') {
            const void *nl = memchr(data + p, '\n', n - p);
            p = nl ? (size_t)((const char *)nl - data) + 1 : n;
        }
        cuts[i] = p < n ? p : n;
    }
    cuts[world] = n;
    return VCFXG_OK;
}

const char *vcfxg_last_schedule(const vcfxg_ctx *c) { return c ? c->last_schedule : ""; }
int vcfxg_last_af_depth(const vcfxg_ctx *c, int *rolling) {
    if (rolling) *rolling = c && c->last_af_roll ? 1 : 0;
    return c ? c->last_af_depth : 0;
}
int vcfxg_last_walk_layout(const vcfxg_ctx *c, int64_t out[8]) {
    if (!c || !out) return 0;
    const vcfxg::WalkLayout &l = c->last_walk_layout;
    out[0] = l.C;
    out[1] = l.Cs;
    out[2] = l.K1 == vcfxg::kWalkAllRounds ? -1 : (int64_t)l.K1;
    out[3] = l.grid;
    out[4] = l.nw;
    out[5] = c->last_walk_resident;
    out[6] = c->last_walk_layout_kind.div;
    out[7] = c->last_walk_layout_kind.g;
    return c->last_walk_layout_kind.kind;
}
uint64_t vcfxg_bgzf_handed_over(const vcfxg_ctx *c) { return c ? c->bgz_handed : 0; }

int vcfxg_fetch_text_range(vcfxg_ctx *c, uint64_t offset, size_t n, void *host) {
    if (!c || (!host && n)) return VCFXG_E_ARG;
    if (offset > c->text_bytes || n > c->text_bytes - offset) return VCFXG_E_ARG;
    if (!n) return VCFXG_OK;
    HIPCHK(c, hipMemcpyAsync(host, P<char>(c->text) + offset, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

int vcfxg_fetch_lines(vcfxg_ctx *c, uint64_t first, uint64_t count, int32_t *alt, int32_t *total, uint8_t *status) {
    if (!c) return VCFXG_E_ARG;
    if (!c->indexed) return VCFXG_E_STATE;
    DENSE(c);
    if (first + count > c->n_lines) return VCFXG_E_ARG;
    if (!count) return VCFXG_OK;
    if (alt) HIPCHK(c, hipMemcpyAsync(alt, P<int32_t>(c->alt) + first, 4 * count, hipMemcpyDeviceToHost, c->stream));
    if (total) HIPCHK(c, hipMemcpyAsync(total, P<int32_t>(c->tot) + first, 4 * count, hipMemcpyDeviceToHost, c->stream));
    if (status) HIPCHK(c, hipMemcpyAsync(status, P<uint8_t>(c->status) + first, count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VCFXG_OK;
}

}  // extern "C"
