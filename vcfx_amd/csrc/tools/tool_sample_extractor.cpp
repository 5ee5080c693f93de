// VCFX_sample_extractor drop-in: the reference CLI (VCFX_sample_extractor.cpp:344-413, main
// :554-560) on top of vcfxg_sample_extract.  The host reads the lines up to the first "#CHROM"
// line (the selection: which columns are kept, the warnings for the names not found, the
// rewritten header line) and the device rewrites every line after it, in blocks of
// VCFXG_SX_BLOCK lines; the host prints the skipped lines' warnings from the per-line statuses.
// File mode (extractSamplesMmap :186-339) selects once; stdin mode (extractSamples :441-544)
// selects again at every later "#CHROM" line, where the device range is split.
#include <ctype.h>
#include <getopt.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_set>
#include <vector>

#include "emit.h"
#include "hostio.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// displayHelp :415-436
const char *kHelp =
    "VCFX_sample_extractor: Subset a VCF to a chosen set of samples.\n\n"
    "Usage:\n"
    "  VCFX_sample_extractor --samples \"Sample1,Sample2\" [options] [input.vcf]\n"
    "  VCFX_sample_extractor --samples \"Sample1,Sample2\" < input.vcf > output.vcf\n\n"
    "Options:\n"
    "  -h, --help              Print this help.\n"
    "  -s, --samples <LIST>    Comma or space separated list of sample names.\n"
    "  -i, --input FILE        Input VCF file (uses fast memory-mapped I/O)\n\n"
    "Performance:\n"
    "  File input (-i) uses memory-mapped I/O for 10-20x faster processing.\n"
    "  Features include:\n"
    "  - SIMD-optimized line scanning (AVX2/SSE2 on x86_64)\n"
    "  - Zero-copy field extraction\n"
    "  - 1MB output buffering\n\n"
    "Description:\n"
    "  Reads #CHROM line to identify sample columns. Keeps only user-specified samples.\n"
    "  Rewrites #CHROM line with that subset. For each variant data line, we keep only the\n"
    "  chosen sample columns. If a sample isn't found in the header, logs a warning.\n\n"
    "Example:\n"
    "  VCFX_sample_extractor --samples \"IndivA,IndivB\" -i input.vcf > subset.vcf\n";

const char kWarnPre[] = "Warning: data line encountered before #CHROM => skipping.\n";
const char kWarnShort[] = "Warning: line has <8 columns => skipping.\n";
const char kWarnNoSamples[] = "Warning: data line with no sample columns => skipping.\n";

struct Selection {
    const std::vector<std::string> &samples;
    std::unordered_set<std::string> set;
    std::vector<uint32_t> cols;  // the kept columns' field numbers, ascending
    explicit Selection(const std::vector<std::string> &s) : samples(s), set(s.begin(), s.end()) {}

    // The "#CHROM" line [ls, le): the kept columns, a warning per requested name that no column
    // has, and the line with its first nine fields and the kept names (:229-270, :466-496).
    // stdin mode: a line of fewer than nine fields passes through and keeps nothing.
    void chrom(const char *ls, const char *le, bool stdin_mode, bool write, Out &out, Out &err) {
        std::vector<std::pair<const char *, const char *>> f;
        for (const char *p = ls;;) {
            const char *t = (const char *)memchr(p, '\t', (size_t)(le - p));
            f.emplace_back(p, t ? t : le);
            if (!t) break;
            p = t + 1;
        }
        cols.clear();
        if (stdin_mode && f.size() < 9) {
            if (write) {
                out.put(ls, (size_t)(le - ls));
                out.putc('\n');
            }
            return;
        }
        std::unordered_set<std::string> kept;
        for (size_t i = 9; i < f.size(); i++) {
            std::string name(f[i].first, f[i].second);
            if (set.count(name)) {
                cols.push_back((uint32_t)i);
                kept.insert(std::move(name));
            }
        }
        for (const auto &s : samples)
            if (!kept.count(s)) err.put("Warning: sample '" + s + "' not found in header.\n");
        if (!write) return;
        for (size_t i = 0; i < 9 && i < f.size(); i++) {
            if (i) out.putc('\t');
            out.put(f[i].first, (size_t)(f[i].second - f[i].first));
        }
        for (uint32_t c : cols) {
            out.putc('\t');
            out.put(f[c].first, (size_t)(f[c].second - f[c].first));
        }
        out.putc('\n');
    }
};

void warn_lines(const std::vector<uint8_t> &st, Out &err) {
    for (uint8_t s : st) {
        if (s == VCFXG_SX_SHORT) err.put(kWarnShort, sizeof kWarnShort - 1);
        else if (s == VCFXG_SX_NO_SAMPLES) err.put(kWarnNoSamples, sizeof kWarnNoSamples - 1);
        else if (s == VCFXG_SX_PRE) err.put(kWarnPre, sizeof kWarnPre - 1);
    }
}

// The lines from byte `start` on, rewritten by the device with the selection S (made by a
// "#CHROM" line before them).
bool run_device(Lines &L, size_t start, bool stdin_mode, Selection &S, Out &out, Out &err) {
    if (!L.device()) return false;
    vcfxg_ctx *g = L.g;
    phase("input resident in HBM");
    uint64_t nl = 0;
    if (!gpu_ok(g, vcfxg_index(g, start, &nl), "index", err.fd)) return false;
    phase("index");
    std::vector<uint8_t> st;
    vcfxg_summary s;
    // one call: lines [l, l + s.n_lines) and their statuses (when some line needs the host)
    auto extract = [&](uint64_t l, uint64_t end) {
        vcfxg_sx_params P{S.cols.data(), (uint64_t)S.cols.size(), stdin_mode ? VCFXG_MODE_STDIN : VCFXG_MODE_FILE, 1};
        if (!gpu_ok(g, vcfxg_sample_extract(g, l, end, &P, &s), "sample_extract", err.fd)) return false;
        st.assign(s.warn_lines ? (size_t)s.n_lines : 0, 0);
        return st.empty() || gpu_ok(g, vcfxg_fetch_lines(g, l, s.n_lines, nullptr, nullptr, st.data()), "fetch_lines", err.fd);
    };
    for (uint64_t l = 0; l < nl;) {
        if (!extract(l, nl)) return false;
        const size_t k = (size_t)(std::find(st.begin(), st.end(), (uint8_t)VCFXG_SX_CHROM) - st.begin());
        if (k < st.size()) {
            // stdin mode selects again at this line (:466-496): the lines before it with the
            // selection so far, then the line itself on the host
            if (k > 0) {
                if (!extract(l, l + k) || !write_device_text(g, s.text_bytes, out, err.fd)) return false;
                warn_lines(st, err);
            }
            const uint64_t at = l + k;
            std::string line;
            if (!line_copy(L.in, g, start, at, line, err.fd)) return false;
            S.chrom(line.data(), line.data() + line.size(), true, true, out, err);
            l = at + 1;
            continue;
        }
        if (!write_device_text(g, s.text_bytes, out, err.fd)) return false;
        warn_lines(st, err);
        l += s.n_lines;
    }
    phase("lines written");
    return true;
}

// extractSamplesMmap :186-339 (stdin_mode false) / extractSamples :441-544: the lines up to the
// first "#CHROM" line on the host, the rest on the device
bool run(const Input &in, bool stdin_mode, const std::vector<std::string> &samples, Out &out, Out &err) {
    if (in.n == 0) return true;
    Lines L(in, err.fd);
    Selection S(samples);
    const bool write = !view_skip_header();  // (a multi-GPU rank > 0: rank 0 writes the header part)
    size_t pos = 0, next = 0;
    const char *ls, *le;
    bool found = false;
    while (!found && L.at(pos, ls, le, next)) {
        size_t len = (size_t)(le - ls);
        if (!stdin_mode && len && ls[len - 1] == '\r') len--;
        if (len == 0) {
            if (write) out.putc('\n');
        } else if (ls[0] == '#') {
            if (is_chrom_line(ls, len)) {
                found = true;
                S.chrom(ls, ls + len, stdin_mode, write, out, err);
            } else if (write) {
                out.put(ls, len);
                out.putc('\n');
            }
        } else {
            err.put(kWarnPre, sizeof kWarnPre - 1);
        }
        pos = next;
    }
    if (L.failed) return false;
    phase("header parsed");
    if (!found || pos >= in.n) return true;
    err.flush();
    shard_records_begin(err);
    return run_device(L, pos, stdin_mode, S, out, err);
}

}  // namespace

extern "C" int vcfx_tool_sample_extractor(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_sample_extractor version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // run :344-413
    if (argc == 1) {
        out.put(kHelp);
        return 0;
    }
    bool help = false;
    std::vector<std::string> samples;
    std::string input;
    static struct option lo[] = {{"help", no_argument, nullptr, 'h'},
                                 {"samples", required_argument, nullptr, 's'},
                                 {"input", required_argument, nullptr, 'i'},
                                 {nullptr, 0, nullptr, 0}};
    GetoptStderr gs(err);
    optind = 0;
    int opt;
    while ((opt = getopt_long(argc, argv, "hs:i:", lo, nullptr)) != -1) {
        if (opt == 'h') help = true;
        else if (opt == 's') {  // whitespace-separated tokens, each split at commas, trimmed, empties dropped
            const char *p = optarg;
            while (*p) {
                while (*p && isspace((unsigned char)*p)) p++;
                const char *e = p;
                while (*e && !isspace((unsigned char)*e)) e++;
                while (p < e) {
                    const char *c = (const char *)memchr(p, ',', (size_t)(e - p));
                    const char *f = c ? c : e;
                    if (f > p) samples.emplace_back(p, f);
                    p = c ? c + 1 : e;
                }
            }
        } else if (opt == 'i') input = optarg;
        else help = true;
    }
    gs.done();
    if (input.empty() && gs.next < argc) input = argv[gs.next];
    if (help) {
        out.put(kHelp);
        return 0;
    }
    if (samples.empty()) {
        err.put("Error: must specify at least one sample with --samples.\n");
        return 1;
    }
    Input in;
    in.gzip_ok = true;      // .vcf.gz / BGZF input is inflated (VCFX_GZIP=0: off)
    in.bgzf_device = true;  // BGZF members inflated on the device (the records stay there)
    phase("start");
    if (!input.empty() && input != "-") {
        if (!in.open_file(input.c_str())) {
            err.put("Error: Cannot open file: " + input + "\n");
            return 1;
        }
        if (!in.decompress(err.fd)) return 1;
        return run(in, false, samples, out, err) ? 0 : 1;
    }
    in.read_fd(in_fd, /*host_copy=*/false);  // only the header lines are needed on the host
    if (!in.decompress(err.fd)) return 1;
    phase("stdin read");
    return run(in, true, samples, out, err) ? 0 : 1;
}
