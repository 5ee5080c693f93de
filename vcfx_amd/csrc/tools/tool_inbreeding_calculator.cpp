// VCFX_inbreeding_calculator drop-in: the reference CLI (VCFX_inbreeding_calculator.cpp:359-450,
// 855-905) on top of vcfxg_inbreeding_region.  The host parses the header lines -- file mode
// (calculateInbreedingMmap :473-524) reads every leading "#CHROM" line and appends its names,
// stdin mode (calculateInbreedingStdin :689-716) takes the first '#' line that holds "#CHROM"
// and ignores what comes before it -- and the device does the rest: the genotype codes of every
// record, the per-record table, the per-sample chain in record order and the rows.  The host
// writes the column header, and the "NA" rows when no record was used.
#include <getopt.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <string_view>
#include <vector>

#include "emit.h"
#include "hostio.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// displayHelp :359-390
const char *kHelp =
    "VCFX_inbreeding_calculator: Compute individual inbreeding coefficients (F)\n"
    "based on biallelic sites in a VCF.\n\n"
    "Usage:\n"
    "  VCFX_inbreeding_calculator [options] [input.vcf]\n"
    "  VCFX_inbreeding_calculator [options] < input.vcf\n\n"
    "Options:\n"
    "  -i, --input FILE          Input VCF file (uses memory-mapping for best performance)\n"
    "  -q, --quiet               Suppress informational messages\n"
    "  -h, --help                Show this help.\n"
    "  --freq-mode <mode>        'excludeSample' (default) or 'global'\n"
    "  --skip-boundary           Skip boundary freq sites. By default, they are used.\n"
    "  --count-boundary-as-used  If also skipping boundary, still increment usedCount.\n\n"
    "Description:\n"
    "  Reads a VCF in a single pass, ignoring multi-allelic lines (ALT with commas).\n"
    "  For each biallelic variant, we parse each sample's genotype code:\n"
    "       0/0 => 0,   0/1 => 1,   1/1 => 2, else => -1 (ignored)\n\n"
    "  Then, depending on --freq-mode:\n"
    "    * excludeSample => Each sample excludes its own genotype when computing p.\n"
    "    * global        => Compute a single global p from all samples' genotypes.\n\n"
    "  The --skip-boundary option, if set, ignores boundary freq p=0 or p=1.\n"
    "    BUT if you also specify --count-boundary-as-used, those boundary sites\n"
    "    increment usedCount (forcing F=1) without contributing to sumExp.\n\n"
    "  If sumExp=0 for a sample but usedCount>0, we output F=1.\n"
    "  If usedCount=0, we output NA.\n\n"
    "Performance:\n"
    "  Uses memory-mapped I/O and SIMD for ~20x speedup over stdin mode.\n"
    "  When a file is provided directly, uses mmap for faster processing.\n\n"
    "Example:\n"
    "  VCFX_inbreeding_calculator -i input.vcf > inbreeding.txt\n"
    "  VCFX_inbreeding_calculator < input.vcf > inbreeding.txt\n";

const char *kHeader = "Sample\tInbreedingCoefficient\n";

struct Args {
    const char *input = nullptr;
    int freq_mode = 0;
    bool skip_boundary = false, count_boundary = false, quiet = false;
};

// the rows of the device, or "<name>\tNA" per sample when no record was used (:634-643)
bool run_device(const Input &in, Lines &L, size_t data_start, int mode, const Args &A,
                const std::vector<std::string> &names, Out &out, Out &err) {
    out.put(kHeader);
    uint64_t used = 0;
    std::string text;
    if (data_start < in.n) {
        if (!L.device()) return false;
        phase("input resident in HBM");
        std::string cat;
        std::vector<uint64_t> off(names.size() + 1, 0);
        for (size_t i = 0; i < names.size(); i++) {
            cat += names[i];
            off[i + 1] = cat.size();
        }
        vcfxg_ib_params P;
        P.n_samples = (uint32_t)names.size();
        P.names = cat.data();
        P.name_off = off.data();
        P.freq_mode = A.freq_mode;
        P.skip_boundary = A.skip_boundary;
        P.count_boundary_as_used = A.count_boundary;
        vcfxg_summary s;
        if (!gpu_ok(L.g, vcfxg_inbreeding_region(L.g, data_start, mode, &P, &s), "inbreeding_region", err.fd))
            return false;
        phase("inbreeding_region");
        used = s.rows;
        if (used) {
            text.resize(s.text_bytes);
            if (!gpu_ok(L.g, vcfxg_fetch_text(L.g, &text[0], text.size()), "fetch", err.fd)) return false;
        }
    }
    if (!used) {
        if (!A.quiet) err.put("No biallelic variants found.\n");
        for (const std::string &n : names) out.put(n + "\tNA\n");
        return true;
    }
    out.put(text);
    return true;
}

// calculateInbreedingMmap :456-664
bool run_file(const Input &in, const Args &A, Out &out, Out &err) {
    if (in.n == 0) {
        err.put("Error: Empty file.\n");
        out.put(kHeader);
        return true;
    }
    Lines L(in, err.fd);
    std::vector<std::string> names;
    bool found = false;
    size_t pos = 0, next = 0, data_start = in.n;
    const char *ls, *le;
    while (L.at(pos, ls, le, next)) {
        size_t len = (size_t)(le - ls);
        if (len && ls[len - 1] == '\r') len--;
        if (len && ls[0] != '#') {  // the first data line
            data_start = pos;
            break;
        }
        if (len >= 6 && memcmp(ls, "#CHROM", 6) == 0) {  // (every leading one: the names are appended)
            found = true;
            const char *f = ls, *fe = ls + len;
            for (int idx = 0; f < fe; idx++) {
                const char *t = (const char *)memchr(f, '\t', (size_t)(fe - f));
                if (!t) t = fe;
                if (idx >= 9) {
                    size_t k = (size_t)(t - f);
                    if (k && f[k - 1] == '\r') k--;
                    names.emplace_back(f, k);
                }
                f = t + 1;
            }
        }
        pos = next;
    }
    if (L.failed) return false;
    phase("header parsed");
    if (!found || names.empty()) {
        err.put("Error: No #CHROM line or no samples found.\n");
        out.put(kHeader);
        return true;
    }
    return run_device(in, L, data_start, VCFXG_MODE_FILE, A, names, out, err);
}

// calculateInbreedingStdin :670-822
bool run_stdin(const Input &in, const Args &A, Out &out, Out &err) {
    Lines L(in, err.fd);
    std::vector<std::string> names;
    bool found = false;
    size_t pos = 0, next = 0, data_start = in.n;
    const char *ls, *le;
    while (L.at(pos, ls, le, next)) {
        size_t len = (size_t)(le - ls);
        if (len && ls[len - 1] == '\r') len--;
        if (len && ls[0] == '#' && std::string_view(ls, len).find("#CHROM") != std::string_view::npos) {
            found = true;
            const char *f = ls, *fe = ls + len;
            for (int idx = 0;; idx++) {  // split_tabs: a trailing empty field counts
                const char *t = (const char *)memchr(f, '\t', (size_t)(fe - f));
                if (idx >= 9) names.emplace_back(f, (size_t)((t ? t : fe) - f));
                if (!t) break;
                f = t + 1;
            }
            data_start = next;
            break;
        }
        pos = next;
    }
    if (L.failed) return false;
    phase("header parsed");
    if (!found || names.empty()) {
        out.put(kHeader);
        err.put(!found ? "Error: No #CHROM line found.\n" : "Error: No sample columns found.\n");
        return true;
    }
    return run_device(in, L, data_start, VCFXG_MODE_STDIN, A, names, out, err);
}

}  // namespace

extern "C" int vcfx_tool_inbreeding_calculator(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_inbreeding_calculator version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // parseArgs :392-450
    Args A;
    bool help = false;
    static struct option lo[] = {{"help", no_argument, nullptr, 'h'},
                                 {"input", required_argument, nullptr, 'i'},
                                 {"quiet", no_argument, nullptr, 'q'},
                                 {"freq-mode", required_argument, nullptr, 0},
                                 {"skip-boundary", no_argument, nullptr, 0},
                                 {"count-boundary-as-used", no_argument, nullptr, 0},
                                 {nullptr, 0, nullptr, 0}};
    GetoptStderr gs(err);
    optind = 0;
    int opt, li = 0;
    std::string warn;
    while ((opt = getopt_long(argc, argv, "hi:q", lo, &li)) != -1) {
        if (opt == 'i') A.input = optarg;
        else if (opt == 'q') A.quiet = true;
        else if (opt == 'h') help = true;
        else if (opt == 0) {
            const std::string name = lo[li].name;
            if (name == "freq-mode") {
                if (!strcmp(optarg, "global")) A.freq_mode = 1;
                else if (!strcmp(optarg, "excludeSample")) A.freq_mode = 0;
                else  // (std::cerr is unbuffered: the warning comes after getopt's earlier messages)
                    fprintf(stderr, "Warning: unrecognized freq-mode='%s'. Using 'excludeSample' by default.\n", optarg);
            } else if (name == "skip-boundary") A.skip_boundary = true;
            else if (name == "count-boundary-as-used") A.count_boundary = true;
        } else help = true;
    }
    gs.done();
    if (!A.input && gs.next < argc) A.input = argv[gs.next];
    if (help) {
        out.put(kHelp);
        return 0;
    }
    Input in;
    in.gzip_ok = true;      // .vcf.gz / BGZF input is inflated (VCFX_GZIP=0: off)
    in.bgzf_device = true;  // BGZF members inflated on the device (the records stay there)
    if (A.input) {
        phase("start");
        if (!in.open_file(A.input)) {
            err.put(std::string("Error: Cannot open file: ") + A.input + "\n");
            return 1;
        }
        if (!A.quiet) err.put(std::string("Processing ") + A.input + " (" + std::to_string(reported_size(in)) + " bytes)...\n");
        err.flush();
        if (!in.decompress(err.fd)) return 1;
        return run_file(in, A, out, err) ? 0 : 1;
    }
    phase("start");
    in.read_fd(in_fd, /*host_copy=*/false);  // only the header lines are needed on the host
    if (!in.decompress(err.fd)) return 1;
    phase("stdin read");
    return run_stdin(in, A, out, err) ? 0 : 1;
}
