// VCFX_field_extractor drop-in: the reference CLI (VCFX_field_extractor.cpp: main :709-773, file mode
// extractFieldsMmap :319-505, stdin mode extractFields :654-702) on top of vcfxg_fields_load / _scan /
// _text.  The host parses the field list and, when a field names a sample, reads the lines up to the
// first "#CHROM" line for the names (fx_host.h); the device decides every line and every cell
// (vcfxg_index from offset 0, so '#' and empty lines are classified wherever they stand) and writes the
// rows; the host prints the header row and the rows through a pinned window over the device's text.
// A field 'S' with no digits, or with a value outside int, kills the reference (std::stoi): here it is
// a one-line error and exit 1 before any input is read.
#include <getopt.h>
#include <string.h>

#include <string>
#include <vector>

#include "emit.h"
#include "fx_host.h"
#include "hostio.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// printHelp :510-533
const char *kHelp =
    "VCFX_field_extractor\n"
    "Usage: VCFX_field_extractor --fields \"FIELD1,FIELD2,...\" [OPTIONS] [input.vcf]\n\n"
    "Description:\n"
    "  Extracts specified fields from each VCF record. Fields can be:\n"
    "    - Standard fields: CHROM, POS, ID, REF, ALT, QUAL, FILTER, INFO\n"
    "    - Subkeys in INFO (e.g. DP, AF, ANN). These are extracted from the INFO column.\n"
    "    - Sample subfields: e.g. SampleName:GT or S2:DP, referencing the second sample's DP.\n"
    "      You can use sample name as it appears in #CHROM line, or 'S' plus 1-based sample index.\n"
    "If a requested field is not found or invalid, '.' is output.\n\n"
    "Options:\n"
    "  --fields, -f   Comma-separated list of fields to extract\n"
    "  --input, -i    Input VCF file (uses fast memory-mapped I/O)\n"
    "  --help, -h     Show this help message\n\n"
    "Performance:\n"
    "  File input (-i) uses memory-mapped I/O for 10-20x faster processing.\n"
    "  Features include:\n"
    "  - SIMD-optimized line scanning (AVX2/SSE2 on x86_64)\n"
    "  - Zero-copy field extraction\n"
    "  - 1MB output buffering\n"
    "  - Direct INFO key lookup without full parsing\n\n"
    "Example:\n"
    "  VCFX_field_extractor --fields \"CHROM,POS,ID,REF,ALT,DP,Sample1:GT\" -i input.vcf > out.tsv\n";

bool run(const Input &in, const std::vector<std::string> &fields, bool stdin_mode, Out &out, Out &err) {
    out.put(fx_header_row(fields));
    if (in.n == 0) return true;
    Lines L(in, err.fd);
    // the names of the first "#CHROM" line, wherever it stands (read only when a field needs them)
    std::unordered_map<std::string, uint32_t> names;
    uint64_t names_from = ~0ull;
    if (fx_needs_names(fields, stdin_mode)) {
        size_t pos = 0, next = 0;
        const char *ls, *le;
        while (L.at(pos, ls, le, next)) {
            size_t n = (size_t)(le - ls);
            if (!stdin_mode && n && ls[n - 1] == '\r') n--;
            if (fx_is_chrom(ls, n)) {
                fx_names(ls, n, names);
                names_from = (uint64_t)pos + 1;  // (the lines that start after this one's first byte)
                break;
            }
            pos = next;
        }
        if (L.failed) return false;
        phase("header parsed");
    }
    std::vector<vcfxg_fx_col> cols;
    std::string pool;
    fx_build(fields, names, stdin_mode, cols, pool);
    if (!L.device()) return false;
    vcfxg_ctx *g = L.g;
    phase("input resident in HBM");
    uint64_t nl = 0;
    if (!gpu_ok(g, vcfxg_index(g, 0, &nl), "index", err.fd)) return false;
    phase("index");
    if (!gpu_ok(g,
                vcfxg_fields_load(g, cols.data(), (uint32_t)cols.size(), pool.data(), (uint32_t)pool.size(),
                                  stdin_mode ? VCFXG_MODE_STDIN : VCFXG_MODE_FILE),
                "fields_load", err.fd))
        return false;
    vcfxg_summary s;
    if (!gpu_ok(g, vcfxg_fields_scan(g, names_from, &s), "fields_scan", err.fd)) return false;
    phase("cells");
    if (!gpu_ok(g, vcfxg_fields_text(g, &s), "fields_text", err.fd)) return false;
    phase("text on the device");
    const uint64_t text = s.text_bytes;
    bool ok = true;
    if (text) {
        const size_t cap = (size_t)std::min<uint64_t>(text, std::max<size_t>(window_bytes(), 1));
        char *win = nullptr;
        if (!gpu_ok(g, vcfxg_host_alloc(g, cap, (void **)&win), "host_alloc", err.fd)) return false;
        for (uint64_t a = 0; ok && a < text;) {
            const uint64_t e = std::min<uint64_t>(text, a + cap);
            if (!(ok = gpu_ok(g, vcfxg_fetch_text_range(g, a, (size_t)(e - a), win), "fetch_text", err.fd))) break;
            out.put(win, (size_t)(e - a));
            out.flush();  // (the window is reused)
            a = e;
        }
        vcfxg_host_free(g, win);
    }
    out.flush();
    phase("rows written");
    return ok;
}

}  // namespace

extern "C" int vcfx_tool_field_extractor(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_field_extractor version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // main :714-765: every -f appends; -h and an unknown option end in the help with 0
    bool help = false;
    std::vector<std::string> fields;
    const char *input = nullptr;
    static struct option lo[] = {{"help", no_argument, nullptr, 'h'},
                                 {"fields", required_argument, nullptr, 'f'},
                                 {"input", required_argument, nullptr, 'i'},
                                 {nullptr, 0, nullptr, 0}};
    GetoptStderr gs(err);
    optind = 0;
    int opt;
    while ((opt = getopt_long(argc, argv, "hf:i:", lo, nullptr)) != -1) {
        if (opt == 'f') fx_split_fields(optarg, fields);
        else if (opt == 'i') input = optarg;
        else help = true;
    }
    gs.done();
    if ((!input || !*input) && gs.next < argc) input = argv[gs.next];
    if (help) {
        out.put(kHelp);
        return 0;
    }
    if (fields.empty()) {
        err.put("No fields specified. Use --fields or -f to specify.\nUse --help for usage.\n");
        return 1;
    }
    const int bad = fx_first_bad_field(fields);
    if (bad >= 0) {
        err.put("Error: invalid sample index in field '" + fields[(size_t)bad] + "'\n");
        return 1;
    }
    Input in;
    in.gzip_ok = true;      // .vcf.gz / BGZF input is inflated (VCFX_GZIP=0: off)
    in.bgzf_device = true;  // BGZF members inflated on the device (the names are fetched from there)
    phase("start");
    if (input && *input && strcmp(input, "-") != 0) {
        if (!in.open_file(input)) {
            err.put(std::string("Error: Cannot open file: ") + input + "\n");
            return 1;
        }
        if (!in.decompress(err.fd)) return 1;
        if (in.n == 0) return 0;  // (an empty file: not even the header row, :327)
        return run(in, fields, false, out, err) ? 0 : 1;
    }
    in.read_fd(in_fd);
    if (!in.decompress(err.fd)) return 1;
    phase("stdin read");
    return run(in, fields, true, out, err) ? 0 : 1;
}
