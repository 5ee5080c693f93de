// VCFX_merger drop-in: the reference CLI (VCFX_merger.cpp: run :94-148, displayHelp :150-173, main
// :355-361) on top of vcfxg_merge.  Every opened file becomes part of one device text (mg_host.h:
// the files in list order, a '\n' after one that lacks its last), indexed from offset 0; the device
// decides every line, orders the written ones (the header block, then the kept lines by key) and
// gathers them (vcfxg_merge_text, block by block); the host writes each block as one range and
// prints stderr in list order: a file's open failure, or (default mode) one warning per malformed
// line of it, from the per-file counts.
// Equal keys: this tool is stable: lines with equal keys come out in (file list order, line order),
// and under -s the earliest file among equal heads is popped.  The reference leaves equal keys to
// std::sort and to its heap: the outputs are byte-identical whenever no two kept lines (under -s on
// unsorted files: no two least heads) share a key, and otherwise differ only inside runs of equal
// keys.  .vcf.gz / BGZF files are inflated on the host (VCFX_GZIP=0: read as text, as the reference
// does), the diff tool's choice.  Outside the domain: -n with a CHROM digit run of more than 18
// digits (the reference then compares uninitialised values).
#include <getopt.h>
#include <string.h>
#include <sys/stat.h>

#include <memory>
#include <string>
#include <vector>

#include "hostio.h"
#include "mg_host.h"
#include "tools.h"

using namespace vcfxh;

namespace {

// displayHelp :150-173
const char *kHelp =
    "VCFX_merger: Merge multiple VCF files by variant position.\n\n"
    "Usage:\n"
    "  VCFX_merger --merge file1.vcf,file2.vcf,... [options]\n\n"
    "Options:\n"
    "  -m, --merge          Comma-separated list of VCF files to merge\n"
    "  -s, --assume-sorted  Assume input files are already sorted (enables streaming\n"
    "                       merge with O(num_files) memory for large files)\n"
    "  -n, --natural-chr    Use natural chromosome order (chr1 < chr2 < chr10)\n"
    "  -h, --help           Display this help message and exit\n\n"
    "Description:\n"
    "  By default, loads all variants into memory and sorts them. This works for\n"
    "  small to medium files but may run out of memory for very large files.\n\n"
    "  With --assume-sorted, uses streaming K-way merge that only keeps one line\n"
    "  per input file in memory. This enables merging files larger than RAM.\n"
    "  Input files MUST be sorted by (CHROM, POS) for correct results.\n\n"
    "Examples:\n"
    "  # Default mode (loads all into memory, sorts)\n"
    "  VCFX_merger --merge sample1.vcf,sample2.vcf > merged.vcf\n\n"
    "  # Streaming mode for large pre-sorted files\n"
    "  VCFX_merger --merge sorted1.vcf,sorted2.vcf --assume-sorted > merged.vcf\n\n"
    "  # With natural chromosome ordering\n"
    "  VCFX_merger --merge f1.vcf,f2.vcf --assume-sorted -n > merged.vcf\n";

struct File {
    std::string name;
    std::unique_ptr<Input> in;  // null: it could not be opened
    uint64_t bad = 0;
};

// an ifstream opens a directory and reads no line from it
bool is_directory(const std::string &path) {
    struct stat st;
    return stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

// mergeVCFInMemory :176-254 / mergeVCFStreaming :257-345 over the opened files
bool run(std::vector<File> &files, bool sorted, bool natural, Out &out, Out &err) {
    MgJoin J;
    std::vector<size_t> opened;  // the joined files' places in `files`
    for (size_t i = 0; i < files.size(); i++)
        if (files[i].in) {
            files[i].in->join_populate();
            J.add(files[i].in->p, files[i].in->n);
            opened.push_back(i);
        }
    J.finish();
    if (J.total) {  // (nothing opened, or only empty files: no output at all)
        vcfxg_ctx *g = gpu(err.fd);
        if (!g) return false;
        int rc = vcfxg_ingest_begin(g, (size_t)J.total);
        for (size_t i = 0; i < J.chunk.size() && !rc; i++) rc = vcfxg_ingest(g, J.chunk[i].p, J.chunk[i].n, J.chunk[i].final_chunk);
        if (!gpu_ok(g, rc, "load", err.fd)) return false;
        phase("inputs resident in HBM");
        uint64_t nl = 0;
        if (!gpu_ok(g, vcfxg_index(g, 0, &nl), "index", err.fd)) return false;
        phase("index");
        const vcfxg_mg_params P{J.start.data(), (uint32_t)J.files(), sorted ? 1 : 0, natural ? 1 : 0};
        vcfxg_summary s;
        if (!gpu_ok(g, vcfxg_merge(g, &P, &s), "merge", err.fd)) return false;
        phase("merge");
        const bool ok = write_text_blocks(
            s.rows,
            [&](uint64_t first, uint64_t *taken, uint64_t *bytes) {
                return gpu_ok(g, vcfxg_merge_text(g, first, taken, bytes), "merge_text", err.fd);
            },
            [&](uint64_t bytes) { return write_device_text(g, bytes, out, err.fd); });
        if (!ok) return false;
        phase("lines written");
        if (s.warn_lines && !sorted) {
            std::vector<uint64_t> first_line(J.files() + 1), bad(J.files());
            if (!gpu_ok(g, vcfxg_merge_files(g, first_line.data(), bad.data()), "merge_files", err.fd)) return false;
            for (size_t k = 0; k < opened.size(); k++) files[opened[k]].bad = bad[k];
        }
    }
    for (const File &f : files) {
        if (!f.in) {
            err.put("Failed to open file: " + f.name + "\n");
            continue;
        }
        const std::string warn = "Warning: skipping malformed line in " + f.name + "\n";
        for (uint64_t k = 0; k < f.bad; k++) err.put(warn);
    }
    return true;
}

}  // namespace

extern "C" int vcfx_tool_merger(int argc, char **argv, int in_fd, int out_fd, int err_fd) {
    (void)in_fd;  // (the tool reads no stdin)
    Out out(out_fd), err(err_fd);
    // vcfx::handle_common_flags (vcfx_core.h:57-62)
    if (flag_present(argc, argv, "--help", "-h")) {
        out.put(kHelp);
        return 0;
    }
    if (flag_present(argc, argv, "--version", "-v")) {
        out.put("VCFX_merger version " VCFX_VERSION_STR "\n");
        return 0;
    }
    // run :94-148
    bool help = false, sorted = false, natural = false;
    std::vector<std::string> names;
    static struct option lo[] = {{"merge", required_argument, nullptr, 'm'},
                                 {"assume-sorted", no_argument, nullptr, 's'},
                                 {"natural-chr", no_argument, nullptr, 'n'},
                                 {"help", no_argument, nullptr, 'h'},
                                 {nullptr, 0, nullptr, 0}};
    GetoptStderr gs(err);
    optind = 0;
    int opt;
    while ((opt = getopt_long(argc, argv, "m:snh", lo, nullptr)) != -1) {
        if (opt == 'm') mg_split(optarg, names);
        else if (opt == 's') sorted = true;
        else if (opt == 'n') natural = true;
        else help = true;  // -h inside a group, an unknown option (getopt's message on stderr)
    }
    gs.done();
    if (help || names.empty()) {
        out.put(kHelp);
        return 0;
    }
    phase("start");
    std::vector<File> files;
    for (const std::string &name : names) {
        File f;
        f.name = name;
        std::unique_ptr<Input> in(new Input);
        in->gzip_ok = true;  // .vcf.gz / BGZF input is inflated on the host (VCFX_GZIP=0: read as text)
        if (is_directory(name)) {
            in->p = "";
            in->n = 0;
            f.in = std::move(in);
        } else if (in->open_file(name.c_str())) {
            if (!in->decompress(err.fd)) return 1;
            f.in = std::move(in);
        }
        files.push_back(std::move(f));
    }
    // (the reference returns 0 whatever happened to its files; 1 here means the device failed)
    return run(files, sorted, natural, out, err) ? 0 : 1;
}
