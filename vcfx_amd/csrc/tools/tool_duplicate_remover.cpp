// VCFX_duplicate_remover drop-in: the reference CLI (VCFX_duplicate_remover.cpp:31-86, main
// :393-399) on top of vcfxg_dedup.  The device decides every line (vcfxg_index from offset 0, so
// '#' and empty lines are classified wherever they stand); the host writes the header and kept
// lines in input order from the bytes it holds (or fetched from the device for an input that
// lives only there), adjacent written lines as one range, and one warning per line with fewer
// than four tabs.  File mode (processFileMmap :226-382) and stdin mode (removeDuplicates :182-214)
// differ in POS and in empty ALT tokens (vcfx_gpu.h); the reference's stderr is not interleaved
// with its stdout in any observable way, so the warnings follow the lines.
#include <getopt.h>
#include <string.h>

#include <string>
#include <vector>

#include "emit.h"
#include "hostio.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// displayHelp :88-108
const char *kHelp =
    "VCFX_duplicate_remover: Remove duplicate variants from VCF files.\n\n"
    "Usage:\n"
    "  VCFX_duplicate_remover [options] [input.vcf]\n"
    "  VCFX_duplicate_remover [options] < input.vcf > output.vcf\n\n"
    "Options:\n"
    "  -i, --input FILE    Input VCF file (uses mmap for best performance)\n"
    "  -q, --quiet         Suppress warning messages\n"
    "  -h, --help          Display this help message and exit\n\n"
    "Description:\n"
    "  Removes duplicate variants from a VCF file based on the combination of\n"
    "  chromosome, position, REF, and ALT alleles. For multi-allelic records, the\n"
    "  ALT field is normalized by sorting the comma-separated alleles so that the\n"
    "  ordering does not affect duplicate detection.\n\n"
    "Performance:\n"
    "  When using -i/--input, the tool uses memory-mapped I/O for\n"
    "  ~10-20x faster processing of large files.\n\n"
    "Example:\n"
    "  VCFX_duplicate_remover -i input.vcf > unique_variants.vcf\n"
    "  VCFX_duplicate_remover < input.vcf > unique_variants.vcf\n";

const char kWarn[] = "Warning: Skipping invalid VCF line.\n";

bool run(const Input &in, bool stdin_mode, bool quiet, Out &out, Out &err) {
    if (in.n == 0) return true;  // (an empty file: no output at all, :243-246)
    Lines L(in, err.fd);
    if (!L.device()) return false;
    vcfxg_ctx *g = L.g;
    phase("input resident in HBM");
    uint64_t nl = 0;
    if (!gpu_ok(g, vcfxg_index(g, 0, &nl), "index", err.fd)) return false;
    phase("index");
    const vcfxg_dd_params P{0};
    vcfxg_summary s;
    if (!gpu_ok(g, vcfxg_dedup(g, stdin_mode ? VCFXG_MODE_STDIN : VCFXG_MODE_FILE, &P, &s), "dedup", err.fd)) return false;
    phase("dedup");
    out.flush();
    LineEmitter em(in.p, in.host_n, out.fd);  // (adjacent written lines leave as one range)
    LineWalk w(in, g, em, 0, nl, err.fd, [&](uint64_t first, uint64_t count, uint8_t *st) {
        return gpu_ok(g, vcfxg_dedup_status(g, first, count, st), "dedup_status", err.fd);
    });
    while (w.next()) {
        if (w.v != VCFXG_DD_KEPT && w.v != VCFXG_DD_HEADER) continue;
        const char *a = w.bytes();
        if (!a) break;
        em.line(a, a + w.len());  // (a final line without '\n' gets one)
    }
    if (!w.finish()) return false;
    phase("lines written");
    if (!quiet)
        for (uint64_t i = 0; i < s.warn_lines; i++) err.put(kWarn, sizeof kWarn - 1);
    return true;
}

}  // namespace

extern "C" int vcfx_tool_duplicate_remover(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_duplicate_remover version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // run :31-86
    bool help = false, quiet = false;
    const char *input = nullptr;
    static struct option lo[] = {{"help", no_argument, nullptr, 'h'},
                                 {"input", required_argument, nullptr, 'i'},
                                 {"quiet", no_argument, nullptr, 'q'},
                                 {nullptr, 0, nullptr, 0}};
    GetoptStderr gs(err);
    optind = 0;
    int opt;
    while ((opt = getopt_long(argc, argv, "hi:q", lo, nullptr)) != -1) {
        if (opt == 'i') input = optarg;
        else if (opt == 'q') quiet = true;
        else help = true;  // -h inside a group, an unknown option (getopt's message on stderr)
    }
    gs.done();
    if (!input && gs.next < argc) input = argv[gs.next];
    if (help) {
        out.put(kHelp);
        return 0;
    }
    Input in;
    in.gzip_ok = true;      // .vcf.gz / BGZF input is inflated (VCFX_GZIP=0: off)
    in.bgzf_device = true;  // BGZF members inflated on the device (the lines are fetched from there)
    phase("start");
    if (input) {
        if (!in.open_file(input)) {
            err.put(std::string("Error: Cannot open file: ") + input + "\n");
            return 1;
        }
        if (!in.decompress(err.fd)) return 1;
        return run(in, false, quiet, out, err) ? 0 : 1;
    }
    in.read_fd(in_fd);
    if (!in.decompress(err.fd)) return 1;
    phase("stdin read");
    return run(in, true, quiet, out, err) ? 0 : 1;
}
