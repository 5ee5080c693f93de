// VCFX_multiallelic_splitter drop-in: the reference CLI (VCFX_multiallelic_splitter.cpp:153-204,
// main :788-795) on top of vcfxg_multiallelic_split.  The host reads the lines up to the first
// "#CHROM" line or the first data line (the ##INFO / ##FORMAT table) and writes them; the device
// decides every line after that and writes the rows of the lines it splits, block by block; the
// host walks each block's lines in order, header and copied lines as ranges of the input and a
// split line's rows from the device text.  File mode (processFileMmap :422-646) drops empty lines
// and, without a "#CHROM" line before the first data line, copies the rest as it is; stdin mode
// (splitMultiAllelicVariants :652-758) writes empty lines and splits wherever a data line stands.
#include <getopt.h>
#include <string.h>

#include <string>
#include <vector>

#include "emit.h"
#include "hostio.h"
#include "ms_host.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// displayHelp :206-224
const char *kHelp =
    "VCFX_multiallelic_splitter: Split multi-allelic variants into multiple lines.\n\n"
    "Usage:\n"
    "  VCFX_multiallelic_splitter [options] [input.vcf]\n"
    "  VCFX_multiallelic_splitter [options] < input.vcf > output.vcf\n\n"
    "Options:\n"
    "  -i, --input FILE    Input VCF file (uses mmap for best performance)\n"
    "  -q, --quiet         Suppress warning messages\n"
    "  -h, --help          Display this help message and exit\n\n"
    "Description:\n"
    "  Splits multi-allelic variants into multiple lines, rewriting GT/AD/PL\n"
    "  and other Number=A/R/G fields for each split variant.\n\n"
    "Performance:\n"
    "  When using -i/--input, the tool uses memory-mapped I/O for\n"
    "  ~15x faster processing of large files.\n\n"
    "Example:\n"
    "  VCFX_multiallelic_splitter -i input.vcf > split.vcf\n"
    "  VCFX_multiallelic_splitter < input.vcf > split.vcf\n";

// printHelp :764-774 (what --help / -h as a whole argument print)
const char *kCommonHelp =
    "VCFX_multiallelic_splitter:\n"
    "  Splits multi-allelic variants into multiple lines, rewriting GT/AD/PL.\n"
    "Usage:\n"
    "  VCFX_multiallelic_splitter [options] < input.vcf > output.vcf\n"
    "  VCFX_multiallelic_splitter -i input.vcf > output.vcf\n"
    "Options:\n"
    "  -i, --input FILE    Input VCF file (uses mmap for best performance)\n"
    "  -q, --quiet         Suppress warnings\n"
    "  --help, -h          Show this help\n";

// the lines from byte `start` on: the device's statuses and rows, the host's copies
bool run_device(Lines &L, size_t start, bool stdin_mode, const std::vector<MsDecl> &decls, Out &out, Out &err) {
    if (!L.device()) return false;
    vcfxg_ctx *g = L.g;
    const Input &in = L.in;
    phase("input resident in HBM");
    uint64_t nl = 0;
    if (!gpu_ok(g, vcfxg_index(g, start, &nl), "index", err.fd)) return false;
    phase("index");
    const std::vector<vcfxg_ms_entry> table = ms_entries(decls);
    const vcfxg_ms_params P{table.data(), (uint64_t)table.size(), stdin_mode ? VCFXG_MODE_STDIN : VCFXG_MODE_FILE};
    out.flush();
    char *text = nullptr;  // the block's rows (pinned; grows)
    size_t text_cap = 0;
    std::vector<uint64_t> off;
    uint64_t a = start;  // the first byte of line l
    bool ok = true;
    for (uint64_t l = 0; ok && l < nl;) {
        vcfxg_summary s;
        if (!(ok = gpu_ok(g, vcfxg_multiallelic_split(g, l, nl, &P, &s), "multiallelic_split", err.fd))) break;
        off.resize((size_t)s.n_lines + 1);
        if (!(ok = gpu_ok(g, vcfxg_ms_line_ranges(g, l, s.n_lines, off.data()), "ms_line_ranges", err.fd))) break;
        if (s.text_bytes > text_cap) {
            if (text) vcfxg_host_free(g, text);
            text = nullptr;
            text_cap = (size_t)s.text_bytes + (size_t)(s.text_bytes >> 2);
            if (!(ok = gpu_ok(g, vcfxg_host_alloc(g, text_cap, (void **)&text), "host_alloc", err.fd))) break;
        }
        if (!(ok = gpu_ok(g, vcfxg_fetch_text_range(g, 0, (size_t)s.text_bytes, text), "fetch_text", err.fd))) break;
        LineEmitter em(in.p, in.host_n, out.fd);
        LineWalk w(in, g, em, a, l + s.n_lines, err.fd, line_status(g, err.fd));
        w.i = w.b0 = l;  // (the walk starts at this block's first line)
        ms_write_block(w, em, stdin_mode, off.data(), text);
        ok = w.finish();
        a = w.next_a;
        l += s.n_lines;
    }
    if (text) vcfxg_host_free(g, text);
    phase("lines written");
    return ok;
}

bool run(const Input &in, bool stdin_mode, Out &out, Out &err) {
    if (in.n == 0) return true;  // (an empty file: no output at all, :439-442)
    Lines L(in, err.fd);
    std::vector<MsDecl> decls;
    size_t pos = 0, next = 0;
    const char *ls, *le;
    bool chrom = false;
    while (L.at(pos, ls, le, next)) {
        const size_t len = (size_t)(le - ls);
        if (len && ls[0] != '#') break;  // a data line before "#CHROM"
        if (len) {
            out.put(ls, len);
            out.putc('\n');
            if (len >= 2 && ls[1] == '#') ms_parse_header_line(ls, len, decls);
            chrom = is_chrom_line(ls, len);
        } else if (stdin_mode) {
            out.putc('\n');
        }
        pos = next;
        if (chrom) break;
    }
    if (L.failed) return false;
    phase("header parsed");
    if (pos >= in.n) return true;
    if (!stdin_mode && !chrom) {
        // no "#CHROM" line: the rest as it is, every line with its '\n' (:513-528)
        if (in.host_n < in.n && !in.tail && !L.device()) return false;
        out.flush();
        char last = 0;
        if (!gpu_ok(L.g, input_copy(in, L.g, in.n - 1, in.n, &last), "input_fetch", err.fd)) return false;
        LineEmitter em(in.p, in.host_n, out.fd);
        LineSource src(in, L.g, em);
        if (!src.put(pos, in.n)) return gpu_ok(L.g, VCFXG_E_HIP, "input_fetch", err.fd);
        if (last != '\n') em.raw("\n", 1);
        em.finish();
        return true;
    }
    return run_device(L, pos, stdin_mode, decls, out, err);
}

}  // namespace

extern "C" int vcfx_tool_multiallelic_splitter(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kCommonHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_multiallelic_splitter version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // run :153-204
    bool help = false;
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
        else if (opt != 'q') help = true;  // -h inside a group, an unknown option (getopt's message on stderr)
    }                                      // (-q: the tool never warns)
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
        return run(in, false, out, err) ? 0 : 1;
    }
    in.read_fd(in_fd);
    if (!in.decompress(err.fd)) return 1;
    phase("stdin read");
    return run(in, true, out, err) ? 0 : 1;
}
