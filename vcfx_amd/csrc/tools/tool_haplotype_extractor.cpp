// VCFX_haplotype_extractor drop-in: the reference CLI (VCFX_haplotype_extractor.cpp: main :826-911, the
// four readers :581-819) on top of vcfxg_haplotype_scan / _blocks / _text.  The host reads the lines
// before the first data line (the first "#CHROM" line names the samples) and answers inputs that hold
// no data line, or no header before it, by itself.  The device then decides every line: status, POS,
// member, block, first flipping sample.  The host prints the header row, the warnings in line order
// (CHROM's bytes from the line it holds) and, under -c -d, the debug stream that the device's block
// decisions and flip indices drive (hx_host.h); the rows leave through a pinned window over the
// device's text.  Batch and streaming mode print the same bytes whenever a header exists.
#include <getopt.h>
#include <string.h>

#include <string>
#include <vector>

#include "emit.h"
#include "hostio.h"
#include "hx_host.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// printHelp :237-261
const char *kHelp =
    "VCFX_haplotype_extractor\n"
    "Usage: VCFX_haplotype_extractor [OPTIONS] [input.vcf]\n\n"
    "Options:\n"
    "  -h, --help                 Display this help message and exit.\n"
    "  -i, --input FILE           Input VCF file (uses fast memory-mapped I/O).\n"
    "  -b, --block-size <int>     Maximum distance for grouping consecutive variants (default 100000).\n"
    "  -c, --check-phase-consistency  If set, try a minimal check across variants.\n"
    "  -s, --streaming            Enable streaming mode: output blocks immediately when complete.\n"
    "                             Uses O(block_size) memory instead of O(total_variants).\n"
    "  -q, --quiet                Suppress warning messages.\n"
    "  -d, --debug                Output verbose debug information.\n\n"
    "Description:\n"
    "  Extracts phased haplotype blocks from genotype data in a VCF file. "
    "It reconstructs haplotypes for each sample by analyzing phased genotype fields.\n\n"
    "Performance:\n"
    "  File input (-i): Uses memory-mapped I/O for 50-100x faster processing.\n"
    "  Streaming mode:  Outputs blocks immediately when complete. Enables\n"
    "                   processing of arbitrarily large files with bounded memory.\n\n"
    "Examples:\n"
    "  ./VCFX_haplotype_extractor -i phased.vcf > haplotypes.tsv\n"
    "  ./VCFX_haplotype_extractor -b 50000 < phased.vcf > haplotypes.tsv\n"
    "  ./VCFX_haplotype_extractor -s -i large_phased.vcf > haplotypes.tsv\n"
    "  ./VCFX_haplotype_extractor -s -b 10000 -i phased.vcf > haplotypes.tsv\n";

const char kWarnShort[] = "Warning: skipping invalid VCF line (<10 fields)\n";
const char kWarnPos[] = "Warning: invalid POS => skip variant\n";

struct Opts {
    int block_size = 100000;
    bool check = false, streaming = false, quiet = false, debug = false;
};

// the lines from byte `start` on (the first data line)
bool run_device(Lines &L, size_t start, bool stdin_mode, const Opts &o, const std::vector<std::string> &names, Out &out,
                Out &err) {
    if (!L.device()) return false;
    vcfxg_ctx *g = L.g;
    const Input &in = L.in;
    phase("input resident in HBM");
    uint64_t nl = 0;
    if (!gpu_ok(g, vcfxg_index(g, start, &nl), "index", err.fd)) return false;
    phase("index");
    const vcfxg_hx_params P{stdin_mode ? VCFXG_MODE_STDIN : VCFXG_MODE_FILE, (uint32_t)names.size(), o.block_size, o.check};
    vcfxg_summary s;
    if (!gpu_ok(g, vcfxg_haplotype_scan(g, &P, &s), "haplotype_scan", err.fd)) return false;
    phase("scan and segmentation");
    out.put(hx_header_row(names));
    // the warnings (and the -c -d stream) in line order
    const bool dbg = o.check && o.debug;
    if (!o.quiet || dbg) {
        std::vector<int64_t> pos;
        std::vector<uint64_t> block;
        std::vector<uint32_t> flip;
        LineEmitter em(in.p, in.host_n, out.fd);  // (the window's owner: nothing is written through it)
        LineWalk w(in, g, em, start, nl, err.fd, [&](uint64_t first, uint64_t count, uint8_t *st) {
            pos.resize((size_t)count);
            block.resize((size_t)count);
            flip.resize((size_t)count);
            return gpu_ok(g, vcfxg_haplotype_lines(g, first, count, st, pos.data(), nullptr, block.data(), flip.data()),
                          "haplotype_lines", err.fd);
        });
        std::string text, prev;
        std::vector<std::pair<uint32_t, uint32_t>> pg, cg;
        uint64_t prev_block = ~0ull;
        while (w.next()) {
            text.clear();
            if (w.v == VCFXG_HX_SHORT) {
                if (!o.quiet) text.assign(kWarnShort, sizeof kWarnShort - 1);
            } else if (w.v == VCFXG_HX_BADPOS) {
                if (!o.quiet) text.assign(kWarnPos, sizeof kWarnPos - 1);
            } else if (w.v == VCFXG_HX_UNPHASED && !o.quiet) {
                const char *a = w.bytes();
                if (!a) break;
                hx_warn_unphased(a, hx_strip(a, w.len()), pos[w.k], text);
            } else if (w.v == VCFXG_HX_MEMBER && dbg) {
                const char *a = w.bytes();
                if (!a) break;
                const size_t n = hx_strip(a, w.len());
                if (!hx_gts(a, n, names.size(), cg)) cg.clear();
                // the pair was examined when it stayed in the block, or left it through a flip
                if (prev_block != ~0ull && (block[w.k] == prev_block || flip[w.k] < names.size()))
                    hx_debug_pair(prev.data(), pg, a, cg, flip[w.k], text);
                prev.assign(a, n);
                pg.swap(cg);
                prev_block = block[w.k];
            }
            if (!text.empty()) err.put(text);
        }
        if (!w.finish()) return false;
        err.flush();
        phase("warnings");
    }
    if (!gpu_ok(g, vcfxg_haplotype_blocks(g, &s), "haplotype_blocks", err.fd)) return false;
    if (!gpu_ok(g, vcfxg_haplotype_text(g, &s), "haplotype_text", err.fd)) return false;
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

bool run(const Input &in, bool stdin_mode, const Opts &o, Out &out, Out &err) {
    Lines L(in, err.fd);
    std::vector<std::string> names;
    size_t pos = 0, next = 0;
    const char *ls, *le;
    bool chrom = false;
    while (L.at(pos, ls, le, next)) {
        const size_t len = (size_t)(le - ls);
        const HxHead h = hx_head_line(ls, len, stdin_mode);
        if (h == kHxData) break;
        if (h == kHxChrom && !chrom) {
            chrom = true;
            if (!hx_names(ls, hx_strip(ls, len), names)) {  // :273-276
                err.put("Error: VCF header does not contain sample columns.\n");
                return false;
            }
        }
        pos = next;
    }
    if (L.failed) return false;
    phase("header parsed");
    if (pos >= in.n) {  // no data line
        if (chrom) out.put(hx_header_row(names));
        else if (!o.streaming) out.put("CHROM\tSTART\tEND\n");
        return true;
    }
    if (!chrom) {
        err.put("Error: no #CHROM header found before data.\n");
        return false;
    }
    return run_device(L, pos, stdin_mode, o, names, out, err);
}

}  // namespace

extern "C" int vcfx_tool_haplotype_extractor(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_haplotype_extractor version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // main :838-880: -h ends the run with 0, an unknown option with 1, both after the help
    Opts o;
    int stop = -1;
    const char *input = nullptr;
    std::string bad_b;
    static struct option lo[] = {{"help", no_argument, nullptr, 'h'},
                                 {"input", required_argument, nullptr, 'i'},
                                 {"block-size", required_argument, nullptr, 'b'},
                                 {"check-phase-consistency", no_argument, nullptr, 'c'},
                                 {"streaming", no_argument, nullptr, 's'},
                                 {"quiet", no_argument, nullptr, 'q'},
                                 {"debug", no_argument, nullptr, 'd'},
                                 {nullptr, 0, nullptr, 0}};
    GetoptStderr gs(err);
    optind = 0;
    int opt;
    while (stop < 0 && (opt = getopt_long(argc, argv, "hi:b:csqd", lo, nullptr)) != -1) {
        if (opt == 'i') input = optarg;
        else if (opt == 'b') {
            // (std::stoi throws here and the reference dies: the drop-in says why and returns 1)
            if (!hx_stoi(optarg, o.block_size)) {
                bad_b = optarg;
                stop = 2;
            }
        } else if (opt == 'c') o.check = true;
        else if (opt == 's') o.streaming = true;
        else if (opt == 'q') o.quiet = true;
        else if (opt == 'd') o.debug = true;
        else stop = opt == 'h' ? 0 : 1;
    }
    gs.done();
    if (stop == 2) {
        err.put("Error: invalid block size: " + bad_b + "\n");
        return 1;
    }
    if (stop >= 0) {
        out.put(kHelp);
        return stop;
    }
    if ((!input || !*input) && gs.next < argc) input = argv[gs.next];
    Input in;
    in.gzip_ok = true;      // .vcf.gz / BGZF input is inflated (VCFX_GZIP=0: off)
    in.bgzf_device = true;  // BGZF members inflated on the device (the lines are fetched from there)
    phase("start");
    if (input && *input) {
        if (!in.open_file(input)) {
            err.put(std::string("Error: could not open file: ") + input + "\n");
            return 1;
        }
        if (!in.decompress(err.fd)) return 1;
        if (in.n == 0) {  // :588-591
            err.put("Error: empty file\n");
            return 1;
        }
        return run(in, false, o, out, err) ? 0 : 1;
    }
    in.read_fd(in_fd);
    if (!in.decompress(err.fd)) return 1;
    phase("stdin read");
    return run(in, true, o, out, err) ? 0 : 1;
}
