// emit.h -- ordered pass-through of input lines to an fd with writev, merging runs of
// consecutive lines that are contiguous in the (mmap'd / buffered) input.  Pass-through
// tools (record_filter, genotype_query, ld matrix) write kept records straight from the
// host copy of the input; only per-line decisions come back from the device.
// Below it, the one reader of input bytes "wherever they live" (the host prefix, a shard view's
// tail, the device): input_copy, LineSource (a pinned window), LineWalk (the lines of an index in
// order with their statuses) and Lines (the header lines of an input before it is indexed).
#pragma once
#include <errno.h>
#include <sys/uio.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "hostio.h"

namespace vcfxh {

struct LineEmitter {
    const char *base, *end;
    int fd;
    std::vector<iovec> iov;
    const char *rs = nullptr, *re = nullptr;
    LineEmitter(const char *b, size_t n, int f) : base(b), end(b + n), fd(f) { iov.reserve(1024); }
    ~LineEmitter() { finish(); }
    // [ls, le) followed by "\n"
    void line(const char *ls, const char *le) {
        if (le < end && *le == '\n') extend(ls, le + 1);
        else {
            extend(ls, le);
            close_run();
            push((const char *)"\n", 1);
        }
    }
    // [s, e) as it is (no newline added)
    void bytes(const char *s, const char *e) { extend(s, e); }
    void raw(const char *p, size_t n) {
        close_run();
        push(p, n);
    }
    void finish() {
        close_run();
        drain();
    }
    // write everything pending, then take a new base buffer (a moved input window)
    void rebase(const char *b, size_t n) {
        finish();
        base = b;
        end = b + n;
    }

   private:
    void extend(const char *s, const char *e) {
        if (rs && re == s) re = e;
        else {
            close_run();
            rs = s;
            re = e;
        }
    }
    void close_run() {
        if (rs && re > rs) push(rs, (size_t)(re - rs));
        rs = re = nullptr;
    }
    void push(const char *p, size_t n) {
        iov.push_back({const_cast<char *>(p), n});
        if (iov.size() >= 512) drain();
    }
    void drain() {
        size_t i = 0;
        while (i < iov.size()) {
            int cnt = (int)std::min<size_t>(iov.size() - i, 512);
            ssize_t k = ::writev(fd, &iov[i], cnt);
            if (k < 0) {
                if (errno == EINTR) continue;
                break;
            }
            size_t left = (size_t)k;
            while (i < iov.size() && left >= iov[i].iov_len) left -= iov[i++].iov_len;
            if (left && i < iov.size()) {
                iov[i].iov_base = (char *)iov[i].iov_base + left;
                iov[i].iov_len -= left;
            }
        }
        iov.clear();
    }
};

// Input bytes [a, b) copied to dst: from the host prefix, a shard view's tail, and (the rest of a
// device-only input, loaded on g) the device.  A vcfxg status.
inline int input_copy(const Input &in, vcfxg_ctx *g, uint64_t a, uint64_t b, char *dst) {
    if (a < in.host_n && a < b) {
        const uint64_t e = std::min<uint64_t>(b, in.host_n);
        memcpy(dst, in.p + a, (size_t)(e - a));
        dst += e - a;
        a = e;
    }
    if (a >= b) return VCFXG_OK;
    if (in.tail) {
        memcpy(dst, in.tail + (a - in.host_n), (size_t)(b - a));
        return VCFXG_OK;
    }
    return vcfxg_input_fetch(g, a, (size_t)(b - a), dst);
}

// Host pointers to the lines of an input's data region, in order, for the pass-through tools.
// A host-resident input (file mapping, `< file`, a host-copied pipe) is addressed in place.
// A device-only stdin stream (Input::host_n < n: the bytes past the header were streamed to
// the device without a host copy) is read back through a pinned window of >= 64 MiB
// (vcfxg_input_fetch, ~50 GB/s; window_bytes()); the emitter writes out what it holds before the window
// moves, so every pointer it keeps stays valid.
struct LineSource {
    const Input &in;
    vcfxg_ctx *g;
    LineEmitter &em;
    char *win = nullptr;
    size_t win_cap = 0;
    uint64_t w0 = 0, w1 = 0;  // window = input bytes [w0, w1)
    bool ok = true;
    LineSource(const Input &i, vcfxg_ctx *ctx, LineEmitter &e) : in(i), g(ctx), em(e) {}
    ~LineSource() {
        if (!win) return;
        em.finish();  // the emitter may still point into the window
        vcfxg_host_free(g, win);
    }
    bool device_only() const { return in.host_n < in.n && !in.tail; }
    bool in_tail = false;
    // bytes [a, b) of the input, plus the byte at b when b < n (the line's newline); nullptr
    // (and ok = false) when the pinned window cannot be allocated or filled: the caller stops
    // at that line and reports the error, writing nothing from it
    const char *at(uint64_t a, uint64_t b) {
        if (in.tail && a >= in.host_n) {  // a shard view: the record range elsewhere in the mapping
            if (!in_tail) {
                em.rebase(in.tail, in.n - in.host_n);
                in_tail = true;
            }
            return in.tail + (a - in.host_n);
        }
        if (!device_only()) return in.p + a;
        const uint64_t need = std::min<uint64_t>(b + 1, in.n);
        if (a >= w0 && need <= w1 && win) return win + (a - w0);
        const size_t want = (size_t)std::max<uint64_t>(window_bytes(), need - a);
        em.finish();  // the emitter may point into the old window: write it out first
        if (want > win_cap) {
            if (win) vcfxg_host_free(g, win);
            win = nullptr;
            if (vcfxg_host_alloc(g, want, (void **)&win) != VCFXG_OK) {
                ok = false;
                win = nullptr;
                win_cap = 0;
                w0 = w1 = 0;
                return nullptr;
            }
            win_cap = want;
        }
        const uint64_t e = std::min<uint64_t>(in.n, a + win_cap);
        if (vcfxg_input_fetch(g, a, (size_t)(e - a), win) != VCFXG_OK) {
            ok = false;  // the window's bytes are stale: nothing may be written from them
            w0 = w1 = 0;
            return nullptr;
        }
        w0 = a;
        w1 = e;
        em.rebase(win, (size_t)(e - a));
        return win;
    }
    // input bytes [a, b) to the emitter as they are (the device part window by window); false
    // after a failed fetch (ok = false)
    bool put(uint64_t a, uint64_t b) {
        if (a < in.host_n && a < b) {
            const uint64_t e = std::min<uint64_t>(b, in.host_n);
            em.bytes(in.p + a, in.p + e);
            a = e;
        }
        if (a < b && in.tail) {
            em.bytes(in.tail + (a - in.host_n), in.tail + (b - in.host_n));
            a = b;
        }
        const uint64_t step = std::max<uint64_t>(window_bytes(), 2) - 1;  // (at() adds the byte at e)
        while (a < b) {
            const uint64_t e = std::min<uint64_t>(b, a + step);
            const char *q = at(a, e);
            if (!q) return false;
            em.bytes(q, q + (e - a));
            a = e;
        }
        return true;
    }
};

// "statuses of lines [first, first + count) of the current index into st": false after a failed
// (and reported) device call.  A caller that needs more per line (the missing detector's INFO
// spans) fetches it for the same block in here.
using LineStatusFn = std::function<bool(uint64_t first, uint64_t count, uint8_t *st)>;
// the per-line statuses of the record tools (vcfxg_fetch_lines)
inline LineStatusFn line_status(vcfxg_ctx *g, int err_fd) {
    return [g, err_fd](uint64_t first, uint64_t count, uint8_t *st) {
        return gpu_ok(g, vcfxg_fetch_lines(g, first, count, nullptr, nullptr, st), "fetch_lines", err_fd);
    };
}

// The lines of the current index (nl of them, made from input byte `start` on) in order with their
// statuses, for a tool that writes some of them through a LineEmitter:
//     LineWalk w(in, g, em, start, nl, err_fd, status);
//     while (w.next()) { ... w.v ...; const char *a = w.bytes(); if (!a) break; ... }
//     if (!w.finish()) return false;
// Line ends and statuses come from the device in blocks of kBlock lines.  A line's bytes are read
// (LineSource: in place, or through the window) only when bytes() is called.
struct LineWalk {
    static constexpr uint64_t kBlock = 1u << 20;
    LineSource src;
    int err_fd;
    LineStatusFn status;  // (empty: the caller looks at no status)
    uint64_t nl, next_a, i = 0, b0 = 0;  // i lines given out; the block held is lines [b0, b0 + ends.size())
    std::vector<uint64_t> ends;
    std::vector<uint8_t> st;
    bool failed = false;  // a block's fetch failed (reported)
    uint64_t a = 0, b = 0;  // the current line: input bytes [a, b), its '\n' (if any) at b
    uint8_t v = 0;          // its status
    size_t k = 0;           // its place in the block the status callable last filled
    LineWalk(const Input &in, vcfxg_ctx *g, LineEmitter &em, uint64_t start, uint64_t n_lines, int efd,
             LineStatusFn s)
        : src(in, g, em), err_fd(efd), status(std::move(s)), nl(n_lines), next_a(start) {}
    bool next() {
        if (failed || !src.ok || i >= nl) return false;
        if (i == b0 + ends.size()) {
            b0 = i;
            const uint64_t c = std::min(kBlock, nl - i);
            ends.resize(c);
            st.assign(c, 0);
            if (!gpu_ok(src.g, vcfxg_line_ends(src.g, b0, c, ends.data()), "line_ends", err_fd) ||
                (status && !status(b0, c, st.data()))) {
                failed = true;
                return false;
            }
        }
        k = (size_t)(i - b0);
        a = next_a;
        b = ends[k];
        v = st[k];
        next_a = b + 1;
        i++;
        return true;
    }
    size_t len() const { return (size_t)(b - a); }
    // the current line's bytes [p, p + len()), and its '\n' at p[len()] when it has one; nullptr
    // after a failed fetch: the walk has ended, nothing may be written from this line
    const char *bytes() { return src.at(a, b); }
    // after the loop: everything written out; false after a failure (a failed line fetch is
    // reported here as input_fetch)
    bool finish() {
        src.em.finish();
        if (failed) return false;
        return src.ok || gpu_ok(src.g, VCFXG_E_HIP, "input_fetch", err_fd);
    }
};

// line l of the current index (made from input byte `start` on) without its '\n', copied
inline bool line_copy(const Input &in, vcfxg_ctx *g, uint64_t start, uint64_t l, std::string &line, int err_fd) {
    uint64_t ends[2] = {0, 0};
    if (!gpu_ok(g, vcfxg_line_ends(g, l ? l - 1 : 0, l ? 2 : 1, ends), "line_ends", err_fd)) return false;
    const uint64_t a = l ? ends[0] + 1 : start, b = l ? ends[1] : ends[0];
    line.resize((size_t)(b - a));
    return b == a || gpu_ok(g, input_copy(in, g, a, b, &line[0]), "input_fetch", err_fd);
}

// The input's lines in order, before an index exists (the header part).  The host holds bytes
// [0, host_n) and a shard view's tail; a device-only input (a pipe read without a host copy, BGZF
// inflated on the device) keeps the rest in HBM, from where the header lines past host_n are
// fetched 64 KiB at a time.
struct Lines {
    const Input &in;
    int err_fd;
    vcfxg_ctx *g = nullptr;
    bool failed = false;
    std::string ext;  // the current line when it is not whole in one host range
    Lines(const Input &i, int e) : in(i), err_fd(e) {}
    bool device() {
        if (g) return true;
        g = gpu(err_fd);
        if (!g || !load_input(g, in, err_fd)) {
            failed = true;
            return false;
        }
        return true;
    }
    // the line at pos: [ls, le) without its '\n', next = the following line's start; false at
    // the end (or after a device error: failed)
    bool at(size_t pos, const char *&ls, const char *&le, size_t &next) {
        if (pos >= in.n) return false;
        // in place: within the host range that holds pos, input bytes [r0, r1) at rp (the host
        // prefix, or a view's tail)
        const bool in_tail = in.tail && pos >= in.host_n;
        const size_t r0 = in_tail ? in.host_n : 0, r1 = in_tail ? in.n : in.host_n;
        const char *rp = in_tail ? in.tail : in.p;
        if (pos < r1) {
            const char *nl = (const char *)memchr(rp + (pos - r0), '\n', r1 - pos);
            if (nl || r1 == in.n) {
                ls = rp + (pos - r0);
                le = nl ? nl : rp + (r1 - r0);
                next = nl ? r0 + (size_t)(nl - rp) + 1 : in.n;
                return true;
            }
        }
        if (!in.tail && !device()) return false;
        ext.clear();
        size_t p = pos;
        while (p < in.n) {
            const size_t k = std::min<size_t>(65536, in.n - p), o = ext.size();
            ext.resize(o + k);
            if (!gpu_ok(g, input_copy(in, g, p, p + k, &ext[o]), "input_fetch", err_fd)) {
                failed = true;
                return false;
            }
            const void *nl = memchr(ext.data() + o, '\n', k);
            p += k;
            if (nl) {
                ext.resize((size_t)((const char *)nl - ext.data()));
                ls = ext.data();
                le = ls + ext.size();
                next = pos + ext.size() + 1;
                return true;
            }
        }
        ls = ext.data();
        le = ls + ext.size();
        next = in.n;
        return true;
    }
};

}  // namespace vcfxh
