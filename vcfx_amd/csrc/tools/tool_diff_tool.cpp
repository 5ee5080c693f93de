// VCFX_diff_tool drop-in: the reference CLI (VCFX_diff_tool.cpp: displayHelp :143-163, run :705-761,
// main :766-783) on top of vcfxg_diff.  Both files become one device text (df_host.h: file 1, a
// '\n' if it lacks its last one, file 2), indexed from offset 0; the device decides every line,
// writes each data line's key text CHROM:POS:REF:sorted ALT and gathers each side's keys
// (vcfxg_diff_text, block by block); the host writes the two header lines and each block as one
// range.  No input line is written, so the tool reads none back.
// Order: -s / --assume-sorted prints what the reference prints, byte for byte.  In the default
// mode the reference prints each side in the iteration order of its C++ library's unordered_set;
// this tool prints each side IN INPUT ORDER OF THE KEY'S FIRST LINE in that file: the header lines
// and the set of lines of each side are the reference's.  -q changes nothing observable there or
// here.  .vcf.gz / BGZF files are inflated on the host (VCFX_GZIP=0: off), an extension the other
// drop-ins make too.  Outside the domain (-s only): a POS or natural-order digit prefix of more than
// 18 digits.
#include <getopt.h>
#include <string.h>

#include <string>

#include "df_host.h"
#include "hostio.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// displayHelp :143-163
const char *kHelp =
    "VCFX_diff_tool: Compare two VCF files and identify differences.\n\n"
    "Usage:\n"
    "  VCFX_diff_tool --file1 <file1.vcf> --file2 <file2.vcf> [options]\n\n"
    "Options:\n"
    "  -h, --help                Display this help message and exit\n"
    "  -a, --file1 <file1.vcf>   Specify the first VCF file\n"
    "  -b, --file2 <file2.vcf>   Specify the second VCF file\n"
    "  -s, --assume-sorted       Assume inputs are sorted by (CHROM, POS).\n"
    "                            Enables streaming mode with O(1) memory.\n"
    "  -n, --natural-chr         Use natural chromosome ordering (chr1 < chr2 < chr10)\n"
    "  -q, --quiet               Suppress warning messages\n\n"
    "Modes:\n"
    "  Default mode:     Loads both files into memory (works with unsorted files)\n"
    "  Streaming mode:   Two-pointer merge diff with O(1) memory (requires sorted input)\n\n"
    "Performance:\n"
    "  Uses memory-mapped I/O with SIMD-accelerated parsing for ~20-50x speedup.\n\n"
    "Example:\n"
    "  VCFX_diff_tool --file1 file1.vcf --file2 file2.vcf\n"
    "  VCFX_diff_tool -a sorted1.vcf -b sorted2.vcf --assume-sorted\n";

bool open_input(Input &in, const std::string &path, Out &err) {
    in.gzip_ok = true;  // .vcf.gz / BGZF input is inflated on the host (VCFX_GZIP=0: off)
    if (!in.open_file(path.c_str())) {
        err.put("Error: Unable to open file " + path + "\n");
        return false;
    }
    return in.decompress(err.fd);
}

void header(Out &out, const char *lead, const std::string &path) {
    out.put(lead);
    out.put(path);
    out.put(":\n");
}

// diffInMemoryMmap :333-404 / diffStreamingMmap :409-506 over the two opened files
bool run(const Input &a, const Input &b, const std::string &path1, const std::string &path2, bool sorted, bool natural,
         Out &out, Out &err) {
    uint64_t unique[2] = {0, 0};
    vcfxg_ctx *g = nullptr;
    if (a.n || b.n) {
        g = gpu(err.fd);
        if (!g) return false;
        a.join_populate();
        b.join_populate();
        DfJoin J;
        J.make(a.p, a.n, b.p, b.n);
        int rc = vcfxg_ingest_begin(g, (size_t)J.total);
        for (int i = 0; i < J.chunks && !rc; i++) rc = vcfxg_ingest(g, J.chunk[i].p, J.chunk[i].n, J.chunk[i].final_chunk);
        if (!gpu_ok(g, rc, "load", err.fd)) return false;
        phase("inputs resident in HBM");
        uint64_t nl = 0;
        if (!gpu_ok(g, vcfxg_index(g, 0, &nl), "index", err.fd)) return false;
        phase("index");
        const vcfxg_df_params P{J.second_start, sorted ? 1 : 0, natural ? 1 : 0, 0};
        vcfxg_summary s;
        uint64_t counts[8];
        if (!gpu_ok(g, vcfxg_diff(g, &P, &s), "diff", err.fd) || !gpu_ok(g, vcfxg_diff_counts(g, counts), "diff_counts", err.fd))
            return false;
        phase("diff");
        unique[0] = counts[0];
        unique[1] = counts[1];
    }
    for (int side = 0; side < 2; side++) {
        header(out, side ? "\nVariants unique to " : "Variants unique to ", side ? path2 : path1);
        const bool ok = write_text_blocks(
            unique[side],
            [&](uint64_t first, uint64_t *taken, uint64_t *bytes) {
                return gpu_ok(g, vcfxg_diff_text(g, side, first, taken, bytes), "diff_text", err.fd);
            },
            [&](uint64_t bytes) { return write_device_text(g, bytes, out, err.fd); });
        if (!ok) return false;
    }
    phase("keys written");
    return true;
}

}  // namespace

extern "C" int vcfx_tool_diff_tool(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    (void)in_fd;  // (the tool reads no stdin)
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_diff_tool version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // run :705-761
    bool help = false, sorted = false, natural = false;
    std::string path1, path2;
    static struct option lo[] = {{"help", no_argument, nullptr, 'h'},           {"file1", required_argument, nullptr, 'a'},
                                 {"file2", required_argument, nullptr, 'b'},    {"assume-sorted", no_argument, nullptr, 's'},
                                 {"natural-chr", no_argument, nullptr, 'n'},    {"quiet", no_argument, nullptr, 'q'},
                                 {nullptr, 0, nullptr, 0}};
    GetoptStderr gs(err);
    optind = 0;
    int opt;
    while ((opt = getopt_long(argc, argv, "ha:b:snq", lo, nullptr)) != -1) {
        if (opt == 'a') path1 = optarg;
        else if (opt == 'b') path2 = optarg;
        else if (opt == 's') sorted = true;
        else if (opt == 'n') natural = true;
        else if (opt == 'q') continue;  // (quiet_: read by no live path)
        else help = true;  // -h inside a group, an unknown option (getopt's message on stderr)
    }
    gs.done();
    if (help || path1.empty() || path2.empty()) {
        out.put(kHelp);
        return help ? 0 : 1;
    }
    phase("start");
    Input a, b;
    if (!open_input(a, path1, err) || !open_input(b, path2, err)) return 1;
    return run(a, b, path1, path2, sorted, natural, out, err) ? 0 : 1;
}
