// tools.h -- in-process entry points of the VCFX_<tool> drop-ins (libvcfx_tools.so).
// Each has the tool's exact CLI contract; binaries are thin main()s over these, and tests
// call them in-process to reuse one GPU context across many cases.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <getopt.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "hostio.h"

#include "vcfx_tools.h"

// VCFX_inbreeding_calculator's entry (run/main, VCFX_inbreeding_calculator.cpp:855-905); reached
// through vcfx_tool_main and the executable
extern "C" int vcfx_tool_inbreeding_calculator(int argc, char **argv, int in_fd, int out_fd, int err_fd);

namespace vcfxh {

// compiled record_filter criterion (FilterCriterion, VCFX_record_filter.h:37-44)
struct Criterion {
    std::string name, str;
    int op = 0, target = 0;
    bool numeric = false;
    double value = 0.0;
};
bool compile_filter(const std::string &all, std::vector<Criterion> &out, Out &err);
// the drop-ins' help texts (the library interfaces' printHelp)
const char *rf_help_text();
const char *gq_help_text();
std::vector<vcfxg_criterion> to_abi(const std::vector<Criterion> &cs);

// getopt_long prints its diagnostics on the C stderr stream; route them to the tool's
// err fd (identical text to the reference's getopt messages).
// getopt_long's state (optind, optarg) and the stderr swap are process-wide: the argument
// phase of the tools is serialised (the ranks of an in-process multi-GPU run parse at once).
std::recursive_mutex &getopt_mutex();
struct GetoptStderr {
    Out &err;
    std::unique_lock<std::recursive_mutex> lk;
    FILE *saved = nullptr, *mem = nullptr;
    char *buf = nullptr;
    size_t len = 0;
    explicit GetoptStderr(Out &e) : err(e), lk(getopt_mutex()) {
        fflush(stderr);
        mem = open_memstream(&buf, &len);
        saved = stderr;
        stderr = mem;
    }
    int next = 0;  // optind when the argument phase ended (read it, not optind, afterwards)
    void done() {
        if (lk.owns_lock()) next = optind;
        if (mem) {
            fflush(mem);
            stderr = saved;
            fclose(mem);
            mem = nullptr;
            if (len) err.put(buf, len);
            free(buf);
            buf = nullptr;
        }
        if (lk.owns_lock()) lk.unlock();
    }
    ~GetoptStderr() { done(); }
};

// The input's lines in order.  The host holds bytes [0, host_n); a device-only input (a pipe
// read without a host copy, BGZF inflated on the device) keeps the rest in HBM, from where the
// header lines past host_n are fetched 64 KiB at a time.
struct Lines {
    const Input &in;
    int err_fd;
    vcfxg_ctx *g = nullptr;
    bool failed = false;
    std::string ext;  // the current line when it is not whole on the host
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
        if (pos < in.host_n) {
            const char *nl = (const char *)memchr(in.p + pos, '\n', in.host_n - pos);
            if (nl || in.host_n == in.n) {
                ls = in.p + pos;
                le = nl ? nl : in.p + in.n;
                next = nl ? (size_t)(nl - in.p) + 1 : in.n;
                return true;
            }
        }
        if (!device()) return false;
        ext.clear();
        size_t p = pos;
        while (p < in.n) {
            const size_t k = std::min<size_t>(65536, in.n - p), o = ext.size();
            ext.resize(o + k);
            if (!gpu_ok(g, vcfxg_input_fetch(g, p, k, &ext[o]), "input_fetch", err_fd)) {
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
