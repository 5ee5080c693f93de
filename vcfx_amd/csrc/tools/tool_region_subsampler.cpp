// VCFX_region_subsampler drop-in: the reference CLI (VCFX_region_subsampler.cpp: run :254-324, main
// :574-580) on top of vcfxg_regions_load and vcfxg_region_filter.  The host parses the BED (rs_host.h,
// loadRegions :344-381) and uploads it as flat arrays; the device sorts it, decides every line
// (vcfxg_index from offset 0, so '#' and empty lines are classified wherever they stand) and the host
// writes the empty, '#' and inside lines in input order from the bytes it holds (or fetched from the
// device for an input that lives only there), adjacent written lines as one range, and one warning
// per rejected line in line order.  File mode (processVCFMmap :427-517) and stdin mode (processVCF
// :519-564) differ in the column rule, in POS and in what -q silences (vcfx_gpu.h); the reference's
// stderr is not interleaved with its stdout in any observable way.
#include <fcntl.h>
#include <getopt.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "emit.h"
#include "hostio.h"
#include "rs_host.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// displayHelp :326-342
const char *kHelp =
    "VCFX_region_subsampler: Keep only variants whose (CHROM,POS) is in a set of regions.\n\n"
    "Usage:\n"
    "  VCFX_region_subsampler -b FILE -i input.vcf > out.vcf\n"
    "  VCFX_region_subsampler --region-bed FILE < input.vcf > out.vcf\n\n"
    "Options:\n"
    "  -h, --help             Show help.\n"
    "  -b, --region-bed FILE  BED file listing multiple regions.\n"
    "  -i, --input FILE       Input VCF file (uses mmap for better performance).\n"
    "  -q, --quiet            Suppress warnings.\n\n"
    "Description:\n"
    "  Reads the BED, which is <chrom> <start> <end> in 0-based. This tool converts\n"
    "  them to 1-based [start+1 .. end]. Then merges intervals per chrom.\n"
    "  Then only lines in the VCF that fall in those intervals for that CHROM are printed.\n\n"
    "Example:\n"
    "  VCFX_region_subsampler --region-bed myregions.bed -i input.vcf > out.vcf\n";

const char kWarnEarly[] = "Warning: data line encountered before #CHROM => skipping.\n";
const char kWarnShortFile[] = "Warning: line has insufficient columns => skipping.\n";
const char kWarnShortStdin[] = "Warning: line has <8 columns => skipping.\n";
const char kWarnPos[] = "Warning: invalid POS => skipping.\n";

// the BED's bytes; false when it cannot be opened (a directory opens and reads as nothing, as the
// reference's ifstream does)
bool read_bed(const char *path, std::string &text) {
    const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return false;
    char buf[65536];
    for (;;) {
        const ssize_t k = ::read(fd, buf, sizeof buf);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) break;
        text.append(buf, (size_t)k);
    }
    ::close(fd);
    return true;
}

bool run(const Input &in, const RsBed &bed, bool stdin_mode, bool quiet, Out &out, Out &err) {
    if (in.n == 0) return true;  // (an empty input: no output at all, :433-435)
    Lines L(in, err.fd);
    if (!L.device()) return false;
    vcfxg_ctx *g = L.g;
    phase("input resident in HBM");
    uint64_t nl = 0;
    if (!gpu_ok(g, vcfxg_index(g, 0, &nl), "index", err.fd)) return false;
    phase("index");
    const vcfxg_rs_params P{0};
    if (!gpu_ok(g,
                vcfxg_regions_load(g, bed.names.data(), bed.name_off.data(), bed.n_chrom(), bed.chrom_id.data(),
                                   bed.start1.data(), bed.end.data(), bed.chrom_id.size(), &P),
                "regions_load", err.fd))
        return false;
    phase("regions");
    vcfxg_summary s;
    if (!gpu_ok(g, vcfxg_region_filter(g, stdin_mode ? VCFXG_MODE_STDIN : VCFXG_MODE_FILE, &s), "region_filter", err.fd))
        return false;
    phase("region filter");
    out.flush();
    const bool warn = stdin_mode || !quiet;  // (-q silences the file mode only)
    const char *w_short = stdin_mode ? kWarnShortStdin : kWarnShortFile;
    const size_t n_short = stdin_mode ? sizeof kWarnShortStdin - 1 : sizeof kWarnShortFile - 1;
    LineEmitter em(in.p, in.host_n, out.fd);  // (adjacent written lines leave as one range)
    LineWalk w(in, g, em, 0, nl, err.fd, [&](uint64_t first, uint64_t count, uint8_t *st) {
        return gpu_ok(g, vcfxg_region_status(g, first, count, st), "region_status", err.fd);
    });
    while (w.next()) {
        if (w.v == VCFXG_RS_EMPTY || w.v == VCFXG_RS_HEADER || w.v == VCFXG_RS_IN) {
            const char *a = w.bytes();
            if (!a) break;
            em.line(a, a + w.len());  // (a final line without '\n' gets one)
        } else if (warn && w.v != VCFXG_RS_OUT) {
            if (w.v == VCFXG_RS_EARLY) err.put(kWarnEarly, sizeof kWarnEarly - 1);
            else if (w.v == VCFXG_RS_SHORT) err.put(w_short, n_short);
            else err.put(kWarnPos, sizeof kWarnPos - 1);
        }
    }
    if (!w.finish()) return false;
    phase("lines written");
    return true;
}

}  // namespace

extern "C" int vcfx_tool_region_subsampler(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_region_subsampler version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // run :254-324 (a positional argument is ignored: stdin is read)
    bool help = false, quiet = false;
    const char *input = nullptr, *bed_path = nullptr;
    static struct option lo[] = {{"help", no_argument, nullptr, 'h'},
                                 {"region-bed", required_argument, nullptr, 'b'},
                                 {"input", required_argument, nullptr, 'i'},
                                 {"quiet", no_argument, nullptr, 'q'},
                                 {nullptr, 0, nullptr, 0}};
    GetoptStderr gs(err);
    optind = 0;
    int opt;
    while ((opt = getopt_long(argc, argv, "hb:i:q", lo, nullptr)) != -1) {
        if (opt == 'b') bed_path = optarg;
        else if (opt == 'i') input = optarg;
        else if (opt == 'q') quiet = true;
        else help = true;  // -h inside a group, an unknown option (getopt's message on stderr)
    }
    gs.done();
    if (help) {
        out.put(kHelp);
        return 0;
    }
    if (!bed_path || !*bed_path) {
        err.put("Error: Must specify --region-bed <FILE>.\n");
        out.put(kHelp);
        return 1;
    }
    // the BED is loaded before the input is touched: its messages come first
    RsBed bed;
    {
        std::string text;
        if (!read_bed(bed_path, text)) {
            err.put(std::string("Error: cannot open BED ") + bed_path + "\n");
            err.put(std::string("Error: failed to load regions from ") + bed_path + "\n");
            return 1;
        }
        bed.parse(text.data(), text.size());
    }
    if (!bed.warnings.empty()) err.put(bed.warnings);
    Input in;
    in.gzip_ok = true;      // .vcf.gz / BGZF input is inflated (VCFX_GZIP=0: off)
    in.bgzf_device = true;  // BGZF members inflated on the device (the lines are fetched from there)
    phase("start");
    if (input && *input) {
        if (!in.open_file(input)) {
            err.put(std::string("Error: failed to process input file: ") + input + "\n");
            return 1;
        }
        if (!in.decompress(err.fd)) return 1;
        return run(in, bed, false, quiet, out, err) ? 0 : 1;
    }
    in.read_fd(in_fd);
    if (!in.decompress(err.fd)) return 1;
    phase("stdin read");
    return run(in, bed, true, quiet, out, err) ? 0 : 1;
}
