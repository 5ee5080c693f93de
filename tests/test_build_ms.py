"""CPU checks of the VCFX_multiallelic_splitter build: the engine library exports its entry points,
the tools library exports the tool's entry (declared in include/vcfx_tools.h), the executable is
there, the dispatcher answers help, version and argument errors without a device, the multi-GPU
plan runs the tool on one context, and the kernels compile for gfx950 without scratch."""
import ctypes
import os
import re
import subprocess

from tests import _multiallelic_splitter_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL


def test_gpu_lib_exports_the_split():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_multiallelic_split", "vcfxg_ms_line_ranges"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    assert hasattr(engine.Engine, "multiallelic_split")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name, value in (("VCFXG_MS_EMPTY", R.EMPTY), ("VCFXG_MS_COPY", R.COPY), ("VCFXG_MS_SPLIT", R.SPLIT),
                        ("VCFXG_MS_HEADER", R.HEADER), ("VCFXG_MS_INFO", R.INFO), ("VCFXG_MS_FORMAT", R.FORMAT),
                        ("VCFXG_MS_NUM_OTHER", R.NUM_OTHER), ("VCFXG_MS_NUM_A", R.NUM_A), ("VCFXG_MS_NUM_R", R.NUM_R),
                        ("VCFXG_MS_NUM_G", R.NUM_G), ("VCFXG_MS_KEYS_LDS", R.KEYS_LDS), ("VCFXG_MS_TABLE_LDS", R.TABLE_LDS)):
        assert re.search(r"#define %s %d\n" % (name, value), hdr), name
    assert "vcfxg_ms_params" in hdr and "vcfxg_ms_entry" in hdr
    assert ctypes.sizeof(engine.MsEntry) == 16 and ctypes.sizeof(engine.MsParams) == 24


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_multiallelic_splitter")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_multiallelic_splitter;" in hdr


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


NO_DEVICE = ([TOOL, "--help"], [TOOL, "-h"], [TOOL, "--version"], [TOOL, "-v"], [TOOL, "-qh"], [TOOL, "--bogus"],
             [TOOL, "-i", "does/not/exist.vcf"], [TOOL, "-q", "does/not/exist.vcf"], [TOOL, "-x", "-i", "f"],
             [TOOL, "-i"], [TOOL, "--input"], [TOOL, "--quiet=1"], [TOOL, "-i", "multiallelic_splitter/empty.vcf"],
             [TOOL, "multiallelic_splitter/empty.vcf", "-q"],
             # file mode without a "#CHROM" line before the data: copied as it is, on the host
             [TOOL, "-i", "multiallelic_splitter/no_chrom.vcf"], [TOOL, "multiallelic_splitter/data_only.vcf"],
             [TOOL, "-i", "multiallelic_splitter/hash_lines_only.vcf"], [TOOL, "-i", "multiallelic_splitter/only_newlines.vcf"],
             [TOOL, "-i", "multiallelic_splitter/header_only.vcf"])


def test_dispatch_knows_the_tool_without_a_device():
    """both help texts, version, argument errors, an unreadable and an empty file, and inputs that
    end before any line reaches the device: the reference's bytes"""
    for argv in NO_DEVICE:
        assert tools.run(argv, cwd=R.GOLDEN) == R.run(argv, cwd=R.GOLDEN), argv
    assert tools.run([TOOL, "--help"])[0] == R.COMMON_HELP != R.HELP == tools.run([TOOL, "-qh"])[0]
    assert tools.run([TOOL, "-i", "does/not/exist.vcf"], cwd=R.GOLDEN) == \
        (b"", b"Error: Cannot open file: does/not/exist.vcf\n", 1)
    by = {c["name"]: c for c in R.load_cases()}
    for name in ("help", "help_in_group", "version", "bad_long", "missing_argument", "missing_file", "empty.vcf__file",
                 "no_chrom.vcf__file", "header_only.vcf__stdin", "only_newlines.vcf__stdin"):
        c = by[name]
        assert tools.run(c["argv"], R.case_stdin(c), cwd=R.GOLDEN) == (c["stdout"], c["stderr"], c["rc"]), name


def test_executable_answers_without_a_device():
    for argv in NO_DEVICE[:8] + NO_DEVICE[14:16]:
        r = subprocess.run(argv, executable=tool_binary(TOOL), capture_output=True, cwd=R.GOLDEN, timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == R.run(argv, cwd=R.GOLDEN), argv


def test_empty_stdin_needs_no_device():
    assert tools.run([TOOL], b"") == (b"", b"", 0) == R.run([TOOL], b"")
    assert tools.run([TOOL, "-q"], b"") == (b"", b"", 0)
    assert tools.run([TOOL], b"\n##x\n\n") == (b"\n##x\n\n", b"", 0) == R.run([TOOL], b"\n##x\n\n")


def test_shard_plan_is_one_context(tmp_path):
    path = tmp_path / "in.vcf"
    path.write_bytes(R.gen_vcf(1, 50, 3))
    for argv in ([TOOL, "-i", str(path)], [TOOL, "-q", str(path)], [TOOL]):
        assert tools.shard_plan(argv, 2)[0] == 1  # unsharded: rows are numbered across the whole block


# per kernel (VGPRs, occupancy in waves per SIMD) as hipcc 's resource-usage remarks gave them when
# the kernels were written; the test holds the build to them from both sides
MEASURED = {"k_ms_scan": (33, 8), "k_ms_cut": (5, 8), "k_ms_len": (40, 8), "k_ms_write": (53, 8), "k_ms_ranges": (6, 8)}


def test_kernels_compile_without_scratch(tmp_path):
    """every k_ms_* kernel as the compiler builds it for gfx950: no scratch, no spilled VGPRs, no
    spilled SGPRs, and the register count and occupancy measured when they were written"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "ms.o"),
                        os.path.join(src, "vcfxg_ms.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = r.stderr.decode()
    names = set(re.findall(r"Function Name: _ZN5vcfxg\d+(k_ms_\w+?)E", text))
    assert names == set(MEASURED), names
    for kernel, (vgprs, occupancy) in MEASURED.items():
        k = text.index("Function Name: _ZN5vcfxg%d%sE" % (len(kernel), kernel))
        vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\w+)",
                               text[k:k + 3000])[:5])
        assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0" and vals["SGPRs Spill"] == "0", \
            (kernel, vals)
        assert int(vals["VGPRs"]) == vgprs and int(vals["Occupancy [waves/SIMD]"]) == occupancy, (kernel, vals)
