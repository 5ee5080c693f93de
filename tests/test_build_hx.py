"""CPU checks of the VCFX_haplotype_extractor build: the engine library exports its entry points, the
header's constants are the restatement's, the tools library exports the tool's entry, the executable is
there, the dispatcher answers help, version, argument errors, an unreadable or empty file, an empty
stdin, a "#CHROM" line without samples and a data line before "#CHROM" without a device, the multi-GPU
plan runs the tool on one context, and the kernels compile for gfx950 without scratch or spilled
registers, within the registers and at the occupancy DESIGN records."""
import ctypes
import os
import re
import subprocess

from tests import _haplotype_extractor_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL
D = "haplotype_extractor/"
CASES = {c["name"]: c for c in R.load_cases()}


def test_gpu_lib_exports_the_entry_points():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_haplotype_scan", "vcfxg_haplotype_blocks", "vcfxg_haplotype_text", "vcfxg_haplotype_lines",
                 "vcfxg_haplotype_table"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    for name in ("haplotype_scan", "haplotype_blocks", "haplotype_text"):
        assert hasattr(engine.Engine, name)
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name, value in (("VCFXG_HX_EMPTY", R.EMPTY), ("VCFXG_HX_HEADER", R.HEADER), ("VCFXG_HX_SHORT", R.SHORT),
                        ("VCFXG_HX_BADPOS", R.BADPOS), ("VCFXG_HX_NOGT", R.NOGT), ("VCFXG_HX_UNPHASED", R.UNPHASED),
                        ("VCFXG_HX_MEMBER", R.MEMBER), ("VCFXG_HX_TILE_MEMBERS", R.TILE_MEMBERS),
                        ("VCFXG_HX_TILE_SAMPLES", R.TILE_SAMPLES)):
        assert re.search(r"#define %s %d\n" % (name, value), hdr), name
    assert "vcfxg_hx_params" in hdr and ctypes.sizeof(engine.HxParams) == 24


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_haplotype_extractor")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_haplotype_extractor;" in hdr
    assert TOOL in TOOLS


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


NO_DEVICE = ("help", "help_short", "help_with_input", "help_in_group", "help_prefix", "version", "version_short", "bad_long",
             "bad_short", "bad_short_stdin", "two_bad_options", "missing_argument", "missing_argument_b",
             "missing_argument_long", "quiet_with_value", "missing_file", "missing_file_positional_stream",
             "empty.vcf__file", "empty.vcf__stream_file", "empty.vcf__stdin", "empty.vcf__stream_stdin",
             "empty.vcf__check_debug_file", "no_samples.vcf__file", "no_samples.vcf__stdin", "no_samples.vcf__stream_stdin",
             "data_first.vcf__file", "data_first.vcf__stream_file", "data_first.vcf__stdin", "cr_only_first.vcf__stdin",
             "cr_only_first.vcf__stream_stdin", "header_only.vcf__file", "header_only.vcf__stdin",
             "header_only.vcf__stream_file", "no_header.vcf__file", "no_header.vcf__stream_file", "no_header.vcf__stdin",
             "no_header.vcf__stream_stdin", "only_newlines.vcf__file", "only_newlines.vcf__stream_stdin",
             "block_m1_header_only", "block_m100000_header_only")


def want(c):
    return c["stdout"], c["stderr"], c["rc"]


def test_dispatch_knows_the_tool_without_a_device():
    """these cases need no device: the reference's bytes"""
    for name in NO_DEVICE:
        c = CASES[name]
        assert tools.run(c["argv"], R.case_stdin(c), cwd=R.GOLDEN) == want(c), name


def test_executable_answers_without_a_device():
    for name in NO_DEVICE[:24]:
        c = CASES[name]
        r = subprocess.run(c["argv"], executable=tool_binary(TOOL), input=R.case_stdin(c), capture_output=True, cwd=R.GOLDEN,
                           timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == want(c), name


def test_a_block_size_stoi_rejects_is_an_error_not_an_abort():
    """the reference dies on std::stoi's exception; the drop-in prints one line and returns 1"""
    for b in ("x", "", "-", "2147483648", "-2147483649", "99999999999999999999"):
        for argv in ([TOOL, "-b", b, "-i", D + "small.vcf"], [TOOL, "--block-size=" + b]):
            out, err, rc = tools.run(argv, cwd=R.GOLDEN)
            assert (out, rc) == (b"", 1) and err.count(b"\n") == 1 and err.startswith(b"Error: "), argv
            assert (out, err, rc) == R.run(argv, cwd=R.GOLDEN)
    r = subprocess.run([TOOL, "-b", "x"], executable=tool_binary(TOOL), capture_output=True, timeout=60)
    assert (r.stdout, r.returncode) == (b"", 1) and r.stderr == R.bad_block_size("x")


def test_shard_plan_is_one_context(tmp_path):
    path = tmp_path / "in.vcf"
    path.write_bytes(R.gen_blocks(3, 4, [5, 70, 2]))
    for argv in ([TOOL, "-i", str(path)], [TOOL, "-s", "-c", str(path)], [TOOL, "-b", "5"]):
        assert tools.shard_plan(argv, 2)[0] == 1  # the block state runs along the lines: not sharded


# (kernel, VGPRs at most, waves per SIMD at least): DESIGN "Haplotype extraction", the build's figures
KERNELS = (("k_hx_scan", 32, 8), ("k_hx_members", 16, 8), ("k_hx_break", 56, 8), ("k_hx_blocks", 16, 8),
           ("k_hx_tileILb0EE", 16, 8), ("k_hx_tileILb1EE", 16, 8), ("k_hx_carry", 16, 8), ("k_hx_rows", 24, 8),
           ("k_hx_heads", 32, 8), ("k_hx_emit", 32, 4))


def test_kernels_compile_without_scratch(tmp_path):
    """every kernel of vcfxg_hx.hip as the compiler builds it for gfx950: no scratch, no spilled VGPRs, no
    spilled SGPRs (resource remarks only)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "hx.o"),
                        os.path.join(src, "vcfxg_hx.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = r.stderr.decode()
    assert text.count("Function Name: _ZN5vcfxg") == len(KERNELS)  # (every kernel of the file is listed above)
    for kernel, max_vgprs, min_occ in KERNELS:
        base = kernel.split("I")[0] if "ILb" in kernel else kernel
        k = text.index("Function Name: _ZN5vcfxg%d%s" % (len(base), kernel))
        vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\w+)",
                               text[k:k + 3000])[:5])
        assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0" and vals["SGPRs Spill"] == "0", \
            (kernel, vals)
        assert int(vals["VGPRs"]) <= max_vgprs and int(vals["Occupancy [waves/SIMD]"]) >= min_occ, (kernel, vals)
