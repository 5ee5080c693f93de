"""CPU checks of the VCFX_fasta_converter build: the engine library exports its entry points, the
tools library exports the tool's entry (declared in include/vcfx_tools.h), the executable is there,
the dispatcher answers help, version, argument errors and inputs without a column without a device,
the multi-GPU plan runs the tool on one context, and the kernels compile for gfx950 without
scratch."""
import ctypes
import os
import re
import subprocess

from tests import _fasta_converter_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL


def test_gpu_lib_exports_the_converter():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_fasta_scan", "vcfxg_fasta_status", "vcfxg_fasta_begin", "vcfxg_fasta"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    assert hasattr(engine.Engine, "fasta_scan") and hasattr(engine.Engine, "fasta")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name, value in (("VCFXG_FA_EMPTY", R.EMPTY), ("VCFXG_FA_COLUMN", R.COLUMN), ("VCFXG_FA_SKIPPED", R.SKIPPED),
                        ("VCFXG_FA_HEADER", R.HEADER), ("VCFXG_FA_CHROM", R.CHROM), ("VCFXG_FA_LINE", R.LINE),
                        ("VCFXG_FA_TILE_SAMPLES", R.TILE_SAMPLES), ("VCFXG_FA_TILE_COLUMNS", R.TILE_COLUMNS),
                        ("VCFXG_FA_TABLE", R.TABLE)):
        assert re.search(r"#define %s %d\n" % (name, value), hdr), name
    assert "vcfxg_fa_params" in hdr
    assert ctypes.sizeof(engine.FaParams) == 40 and ctypes.sizeof(engine.Summary) == 48
    assert TOOL in TOOLS


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_fasta_converter")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_fasta_converter;" in hdr


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


NO_DEVICE = ([TOOL, "--help"], [TOOL, "-h"], [TOOL, "--version"], [TOOL, "-v"], [TOOL, "-qh"], [TOOL, "--bogus"],
             [TOOL, "-i", "does/not/exist.vcf"], [TOOL, "-q", "does/not/exist.vcf"], [TOOL, "-x", "-y", "-i", "f"],
             [TOOL, "-i"], [TOOL, "--input"], [TOOL, "--quiet=1"], [TOOL, "-i", "fasta_converter/empty.vcf"],
             [TOOL, "fasta_converter/empty.vcf", "-q"],
             # inputs that end before any line is a column
             [TOOL, "-i", "fasta_converter/header_only.vcf"], [TOOL, "fasta_converter/hash_lines_only.vcf"],
             [TOOL, "-i", "fasta_converter/no_final_newline_header.vcf"])


def test_dispatch_knows_the_tool_without_a_device():
    """help, version, argument errors, an unreadable and an empty file, header-only input, and the
    stdin data line before "#CHROM": the reference's bytes"""
    for argv in NO_DEVICE:
        assert tools.run(argv, cwd=R.GOLDEN) == R.run(argv, cwd=R.GOLDEN), argv
    assert tools.run([TOOL, "--help"])[0] == R.HELP == tools.run([TOOL, "-qh"])[0]
    assert tools.run([TOOL, "-x", "-y"])[1].count(b"invalid option") == 1  # the first bad option ends the run
    assert tools.run([TOOL, "-i", "does/not/exist.vcf"], cwd=R.GOLDEN) == (b"", b"Error: Cannot open does/not/exist.vcf\n", 1)
    by = {c["name"]: c for c in R.load_cases()}
    for name in ("help", "help_short", "help_in_group", "help_prefix", "version", "version_short", "bad_long",
                 "bad_short_stdin", "two_bad_options", "missing_argument", "missing_argument_long", "missing_file",
                 "missing_file_positional_quiet", "quiet_with_value", "empty.vcf__file", "empty.vcf__stdin",
                 "header_only.vcf__file", "header_only.vcf__stdin", "hash_lines_only.vcf__pos", "only_newlines.vcf__stdin",
                 "data_before_chrom.vcf__stdin", "data_before_chrom.vcf__quiet_stdin", "data_only.vcf__stdin"):
        c = by[name]
        assert tools.run(c["argv"], R.case_stdin(c), cwd=R.GOLDEN) == (c["stdout"], c["stderr"], c["rc"]), name
    assert by["data_before_chrom.vcf__stdin"]["stderr"] == R.NO_CHROM


def test_executable_answers_without_a_device():
    for argv in NO_DEVICE[:8] + NO_DEVICE[12:16]:
        r = subprocess.run(argv, executable=tool_binary(TOOL), capture_output=True, cwd=R.GOLDEN, timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == R.run(argv, cwd=R.GOLDEN), argv


def test_empty_stdin_needs_no_device():
    assert tools.run([TOOL], b"") == (b"", b"", 0) == R.run([TOOL], b"")
    assert tools.run([TOOL, "-q"], b"") == (b"", b"", 0)
    assert tools.run([TOOL], b"\n##x\n\n") == (b"", b"", 0) == R.run([TOOL], b"\n##x\n\n")
    assert tools.run([TOOL], b"##x\n1\t2\n") == (b"", R.NO_CHROM, 0) == R.run([TOOL], b"##x\n1\t2\n")


def test_shard_plan_is_one_context(tmp_path):
    path = tmp_path / "in.vcf"
    path.write_bytes(R.gen_vcf(1, 50, 3))
    for argv in ([TOOL, "-i", str(path)], [TOOL, "-q", str(path)], [TOOL]):
        assert tools.shard_plan(argv, 2)[0] == 1  # unsharded: every row holds every record


# per kernel (VGPRs, occupancy in waves per SIMD) as hipcc 's resource-usage remarks gave them when
# the kernels were written; the test holds the build to them from both sides
MEASURED = {"k_fa_scan": (34, 8), "k_fa_bases": (47, 8), "k_fa_transpose": (25, 8)}


def test_kernels_compile_without_scratch(tmp_path):
    """every k_fa_* kernel as the compiler builds it for gfx950: no scratch, no spilled VGPRs, no
    spilled SGPRs, and the register count and occupancy measured when they were written; the bases
    kernel keeps its allele table in registers (no LDS of its own)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "fa.o"),
                        os.path.join(src, "vcfxg_fa.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = r.stderr.decode()
    names = set(re.findall(r"Function Name: _ZN5vcfxg\d+(k_fa_\w+?)E", text))
    assert names == set(MEASURED), names
    lds = {}
    for kernel, (vgprs, occupancy) in MEASURED.items():
        k = text.index("Function Name: _ZN5vcfxg%d%sE" % (len(kernel), kernel))
        vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|"
                               r"LDS Size \[bytes/block\]): (\w+)", text[k:k + 3000])[:6])
        assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0" and vals["SGPRs Spill"] == "0", \
            (kernel, vals)
        assert int(vals["VGPRs"]) == vgprs and int(vals["Occupancy [waves/SIMD]"]) == occupancy, (kernel, vals)
        lds[kernel] = int(vals["LDS Size [bytes/block]"])
    assert lds == {"k_fa_scan": 192, "k_fa_bases": 0, "k_fa_transpose": R.TILE_SAMPLES * (R.TILE_COLUMNS + R.TILE_COLUMNS // R.LINE)}
