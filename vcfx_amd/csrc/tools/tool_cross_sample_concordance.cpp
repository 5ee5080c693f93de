// VCFX_cross_sample_concordance drop-in: the reference CLI
// (VCFX_cross_sample_concordance.cpp:359-411, 731-750) on top of vcfxg_concordance_region.
// The host reads the header: file mode (calculateConcordanceMmapParallel :445-475) parses EVERY
// "#CHROM" line of the file before any record, each appending its selected columns -- the first
// one on the host, the later ones listed by the device (vcfxg_chrom_lines) and fetched -- and
// drops the data lines before the first; stdin mode (calculateConcordance :622-642) takes the
// first and keeps a '\r' in the last name.  The selection becomes one multiplicity per sample
// column.  The device counts each record's valid and distinct genotype keys and writes the rows,
// in file mode at the places the reference's T worker blocks give them.
#include <getopt.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "emit.h"
#include "hostio.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// displayHelp :324-344
const char *kHelp =
    "VCFX_cross_sample_concordance: Check variant concordance across multiple samples.\n\n"
    "Usage:\n"
    "  VCFX_cross_sample_concordance [options] < input.vcf > concordance_results.txt\n"
    "  VCFX_cross_sample_concordance -i input.vcf > concordance_results.txt\n\n"
    "Options:\n"
    "  -i, --input FILE        Input VCF file (uses mmap for best performance)\n"
    "  -s, --samples LIST      Comma-separated list of samples to check\n"
    "  -t, --threads N         Number of processing threads (default: auto)\n"
    "  -q, --quiet             Suppress summary statistics to stderr\n"
    "  -h, --help              Display this help message and exit\n\n"
    "Description:\n"
    "  Reads a multi-sample VCF, normalizes each sample's genotype\n"
    "  (including multi-allelic variants), and determines if all samples that\n"
    "  have a parseable genotype are in complete agreement.\n\n"
    "Performance:\n"
    "  Uses multi-threaded parallel processing with memory-mapped I/O\n"
    "  and early-termination optimization for extreme performance.\n\n"
    "Example:\n"
    "  VCFX_cross_sample_concordance -i input.vcf -t 8 > results.tsv\n";

const char *kHeader = "CHROM\tPOS\tID\tREF\tALT\tNum_Samples\tUnique_Normalized_Genotypes\tConcordance_Status\n";
const char *kNoChrom = "Error: VCF header with #CHROM not found.\n";

struct Args {
    const char *input = nullptr;
    std::unordered_set<std::string> want;
    int threads = 0;
    bool quiet = false;
};

std::string summary(const uint64_t *t) {
    return "Total Variants with >=1 parseable genotype: " + std::to_string(t[0] + t[1]) +
           "\n   Concordant (all same genotype): " + std::to_string(t[0]) +
           "\n   Discordant (>=2 distinct genotypes): " + std::to_string(t[1]) +
           "\nVariants with no parseable genotypes (skipped): " + std::to_string(t[2]) + "\n";
}

// the device call, the rows and the totals
bool run_device(Lines &L, size_t data_start, int mode, uint32_t ns, const std::vector<uint32_t> &mult, uint64_t T,
                Out &out, Out &err, uint64_t *totals) {
    vcfxg_cc_params P;
    P.n_samples = ns;
    P.mult = mult.empty() ? nullptr : mult.data();
    P.n_mult = mult.size();
    P.threads = T;
    vcfxg_summary s;
    if (!gpu_ok(L.g, vcfxg_concordance_region(L.g, data_start, mode, &P, &s), "concordance_region", err.fd))
        return false;
    phase("concordance_region");
    if (!gpu_ok(L.g, vcfxg_concordance_totals(L.g, totals), "concordance_totals", err.fd)) return false;
    if (s.text_bytes && !write_device_text(L.g, s.text_bytes, out, err.fd)) return false;
    phase("rows written");
    return true;
}

// one "#CHROM" line [ls, le) of the file mode (:452-468): the tab loop's fields (a trailing tab
// opens none) from the tenth on, each selected one counted at its column
void add_chrom_line(const char *ls, const char *le, const Args &A, std::vector<uint32_t> &mult) {
    int col = 0;
    for (const char *f = ls; f < le; col++) {
        const char *t = (const char *)memchr(f, '\t', (size_t)(le - f));
        if (!t) t = le;
        if (col >= 9 && (A.want.empty() || A.want.count(std::string(f, (size_t)(t - f))))) {
            if (mult.size() < (size_t)col - 8) mult.resize((size_t)col - 8, 0u);
            mult[(size_t)col - 9]++;
        }
        f = t < le ? t + 1 : le;
    }
}

// calculateConcordanceMmapParallel :416-593
int run_file(const Input &in, const Args &A, Out &out, Out &err) {
    if (in.n == 0) return 0;  // an empty file: no output at all
    Lines L(in, err.fd);
    std::vector<uint32_t> mult;
    bool found = false;
    size_t pos = 0, next = 0, data_start = in.n;
    const char *ls, *le;
    while (L.at(pos, ls, le, next)) {
        size_t len = (size_t)(le - ls);
        if (len && ls[len - 1] == '\r') len--;
        if (len >= 6 && memcmp(ls, "#CHROM", 6) == 0) {
            found = true;
            add_chrom_line(ls, ls + len, A, mult);
            data_start = next;
            break;
        }
        pos = next;
    }
    if (L.failed) return 1;
    phase("header parsed");
    if (!found) {
        err.put(kNoChrom);
        return 1;
    }
    // the later "#CHROM" lines, wherever they stand
    if (data_start < in.n) {
        if (!L.device()) return 1;
        phase("input resident in HBM");
        uint64_t k = 0;
        std::vector<uint64_t> starts(16);
        if (!gpu_ok(L.g, vcfxg_chrom_lines(L.g, data_start, starts.data(), starts.size(), &k), "chrom_lines", err.fd))
            return 1;
        if (k > starts.size()) {
            starts.resize(k);
            if (!gpu_ok(L.g, vcfxg_chrom_lines(L.g, data_start, starts.data(), starts.size(), &k), "chrom_lines", err.fd))
                return 1;
        }
        for (uint64_t i = 0; i < k; i++) {
            if (!L.at((size_t)starts[i], ls, le, next)) return 1;
            size_t len = (size_t)(le - ls);
            if (len && ls[len - 1] == '\r') len--;
            add_chrom_line(ls, ls + len, A, mult);
        }
        phase("later #CHROM lines");
    }
    if (mult.empty() && !A.want.empty()) err.put("Warning: none of the requested samples were found in the VCF header.\n");
    out.put(kHeader);
    uint64_t t[4] = {0, 0, 0, 0};
    if (data_start < in.n && !run_device(L, data_start, VCFXG_MODE_FILE, 0, mult, (uint64_t)A.threads, out, err, t))
        return 1;
    if (!t[3]) {  // no data lines (:490-495)
        if (!A.quiet) err.put("Total Variants with >=1 parseable genotype: 0\n");
        return 0;
    }
    if (!A.quiet)
        err.put(summary(t) + "Threads used: " + std::to_string(std::min<uint64_t>((uint64_t)A.threads, t[3])) + "\n");
    return 0;
}

// calculateConcordance :598-724
int run_stdin(const Input &in, const Args &A, Out &out, Out &err) {
    out.put(kHeader);
    Lines L(in, err.fd);
    std::vector<std::string> names;
    bool found = false;
    size_t pos = 0, next = 0, data_start = in.n;
    const char *ls, *le;
    while (L.at(pos, ls, le, next)) {
        const size_t len = (size_t)(le - ls);
        if (len >= 6 && memcmp(ls, "#CHROM", 6) == 0) {
            found = true;
            const char *f = ls;
            for (int idx = 0;; idx++) {  // split_tabs: a trailing empty field counts
                const char *t = (const char *)memchr(f, '\t', (size_t)(le - f));
                if (idx >= 9) names.emplace_back(f, (size_t)((t ? t : le) - f));
                if (!t) break;
                f = t + 1;
            }
            data_start = next;
            break;
        }
        pos = next;
    }
    if (L.failed) return 1;
    phase("header parsed");
    if (!found) {
        err.put(kNoChrom);
        return 0;
    }
    std::vector<uint32_t> mult;
    if (!A.want.empty()) {
        mult.assign(names.size(), 0u);
        for (size_t i = 0; i < names.size(); i++) mult[i] = A.want.count(names[i]) ? 1u : 0u;
    } else
        mult.assign(names.size(), 1u);
    uint64_t t[4] = {0, 0, 0, 0};
    if (data_start < in.n) {
        if (!L.device()) return 1;
        phase("input resident in HBM");
        if (!run_device(L, data_start, VCFXG_MODE_STDIN, (uint32_t)names.size(), mult, 0, out, err, t)) return 1;
    }
    if (!A.quiet) err.put(summary(t));
    return 0;
}

}  // namespace

extern "C" int vcfx_tool_cross_sample_concordance(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_cross_sample_concordance version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // parseArguments :359-411
    Args A;
    bool stop = false;
    static struct option lo[] = {{"help", no_argument, nullptr, 'h'},
                                 {"input", required_argument, nullptr, 'i'},
                                 {"samples", required_argument, nullptr, 's'},
                                 {"threads", required_argument, nullptr, 't'},
                                 {"quiet", no_argument, nullptr, 'q'},
                                 {nullptr, 0, nullptr, 0}};
    GetoptStderr gs(err);
    optind = 0;
    int opt;
    while (!stop && (opt = getopt_long(argc, argv, "hi:s:t:q", lo, nullptr)) != -1) {
        if (opt == 'i') A.input = optarg;
        else if (opt == 's') {  // (empty names are kept)
            const std::string s = optarg;
            size_t a = 0, b;
            while ((b = s.find(',', a)) != std::string::npos) {
                A.want.insert(s.substr(a, b - a));
                a = b + 1;
            }
            A.want.insert(s.substr(a));
        } else if (opt == 't') A.threads = atoi(optarg);
        else if (opt == 'q') A.quiet = true;
        else {  // -h inside a group: the help; an unknown option: getopt's message; exit code 0
            if (opt == 'h') out.put(kHelp);
            stop = true;
        }
    }
    gs.done();
    if (stop) return 0;
    if (!A.input && gs.next < argc) A.input = argv[gs.next];
    if (A.threads <= 0) {
        A.threads = (int)std::thread::hardware_concurrency();
        if (A.threads <= 0) A.threads = 4;
    }
    Input in;
    in.gzip_ok = true;      // .vcf.gz / BGZF input is inflated (VCFX_GZIP=0: off)
    in.bgzf_device = true;  // BGZF members inflated on the device (the records stay there)
    if (A.input) {
        phase("start");
        if (!in.open_file(A.input)) {
            err.put(std::string("Error: Cannot open file ") + A.input + "\n");
            return 1;
        }
        if (!in.decompress(err.fd)) return 1;
        return run_file(in, A, out, err);
    }
    phase("start");
    in.read_fd(in_fd, /*host_copy=*/false);  // only the header lines are needed on the host
    if (!in.decompress(err.fd)) return 1;
    phase("stdin read");
    return run_stdin(in, A, out, err);
}
