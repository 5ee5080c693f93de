"""CPU checks of the VCFX_field_extractor build: the engine library exports its entry points, the
header's constants are the restatement's, the tools library exports the tool's entry (declared in
include/vcfx_tools.h), the executable is there, the dispatcher answers help, version, argument errors,
a missing field list, an unreadable file, an empty file and the rejected index fields without a device,
the multi-GPU plan runs the tool on one context, and the cell and write kernels compile for gfx950
without scratch or spilled registers."""
import ctypes
import os
import re
import subprocess

from tests import _field_extractor_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL
D = "field_extractor/"


def test_gpu_lib_exports_the_entry_points():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_fields_load", "vcfxg_fields_scan", "vcfxg_fields_lines", "vcfxg_fields_cells", "vcfxg_fields_text"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    for name in ("fields_load", "fields_scan", "fields_text"):
        assert hasattr(engine.Engine, name)
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name, value in (("VCFXG_FX_EMPTY", R.EMPTY), ("VCFXG_FX_HEADER", R.HEADER), ("VCFXG_FX_ROW", R.ROW), ("VCFXG_FX_STD", R.STD),
                        ("VCFXG_FX_INFO", R.INFO), ("VCFXG_FX_SAMPLE", R.SAMPLE), ("VCFXG_FX_NONE", R.NONE),
                        ("VCFXG_FX_CELL_BYTES", R.CELL_BYTES), ("VCFXG_FX_TABLE_LDS", R.TABLE_LDS),
                        ("VCFXG_FX_TILE_ROWS", R.TILE_ROWS), ("VCFXG_FX_STAGE", R.STAGE)):
        assert re.search(r"#define %s %d\n" % (name, value), hdr), name
    for name, value in (("VCFXG_FX_DOT", R.DOT), ("VCFXG_FX_ONE", R.ONE), ("VCFXG_FX_NOKEY", R.NOKEY)):
        assert re.search(r"#define %s 0x%Xu\n" % (name, value), hdr), name
    assert "vcfxg_fx_col" in hdr and ctypes.sizeof(engine.FxCol) == 32


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_field_extractor")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_field_extractor;" in hdr
    assert TOOL in TOOLS


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


NO_DEVICE = ([TOOL, "--help"], [TOOL, "-h"], [TOOL, "--version"], [TOOL, "-v"], [TOOL, "-hf", "CHROM"], [TOOL, "--bogus"],
             [TOOL, "-x", "-f", "CHROM", "-i", D + "rules.vcf"], [TOOL], [TOOL, "-i", D + "rules.vcf"], [TOOL, "-f"],
             [TOOL, "--fields"], [TOOL, "-f", "CHROM", "-i"], [TOOL, "--help=1", "-f", "CHROM"],
             [TOOL, "-f", "CHROM", "-i", D + "does_not_exist.vcf"], [TOOL, "-f", "CHROM", D + "does_not_exist.vcf"],
             [TOOL, "-i", D + "does_not_exist.vcf"], [TOOL, "-f", "CHROM,DP", "-i", D + "empty.vcf"],
             [TOOL, "-f", "", D + "empty.vcf"], [TOOL, "-f", "S:GT", "-i", D + "rules.vcf"], [TOOL, "-f", "CHROM,S99999999999:GT"],
             [TOOL, "-f", "CHROM", "-f", "S:", "-i", D + "does_not_exist.vcf"], [TOOL, "-x", "-f", "S:GT"])


def test_dispatch_knows_the_tool_without_a_device():
    """help, version, argument errors, no fields, an unreadable or empty file and the rejected index
    fields need no device: the reference's bytes (the drop-in's own line for the rejected fields)"""
    for argv in NO_DEVICE:
        assert tools.run(argv, cwd=R.GOLDEN) == R.run(argv, cwd=R.GOLDEN), argv
    assert tools.run([TOOL, "-f", "CHROM", "-i", "nope.vcf"], cwd=R.GOLDEN) == (b"", b"Error: Cannot open file: nope.vcf\n", 1)
    assert tools.run([TOOL, "-f", "a,S:GT"], b"1\t2\n") == (b"", b"Error: invalid sample index in field 'S:GT'\n", 1)
    assert tools.run([TOOL], b"") == (b"", R.NO_FIELDS, 1)
    by = {c["name"]: c for c in R.load_cases()}
    for name in ("help", "version", "no_fields", "missing_file", "empty_file_positional", "bad_long", "f_without_value"):
        c = by[name]
        assert tools.run(c["argv"], R.case_stdin(c), cwd=R.GOLDEN) == (c["stdout"], c["stderr"], c["rc"]), name


def test_executable_answers_without_a_device():
    for argv in NO_DEVICE[:14] + NO_DEVICE[18:20]:
        r = subprocess.run(argv, executable=tool_binary(TOOL), capture_output=True, cwd=R.GOLDEN, timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == R.run(argv, cwd=R.GOLDEN), argv


def test_empty_stdin_needs_no_device():
    assert tools.run([TOOL, "-f", "CHROM,DP"], b"") == (b"CHROM\tDP\n", b"", 0) == R.run([TOOL, "-f", "CHROM,DP"], b"")
    assert tools.run([TOOL, "-f", ",", "-i", "-"], b"") == (b"\t\n", b"", 0)


def test_shard_plan_is_one_context(tmp_path):
    path = tmp_path / "in.vcf"
    path.write_bytes(R.generated("g300"))
    for argv in ([TOOL, "-f", "CHROM,POS", "-i", str(path)], [TOOL, "-f", "NA1:GT", str(path)], [TOOL, "-f", "CHROM"]):
        assert tools.shard_plan(argv, 2)[0] == 1  # the names hold from the "#CHROM" line on: not sharded


def test_kernels_compile_without_scratch(tmp_path):
    """the cell kernel (table in LDS and in global memory) and the writer as the compiler builds them for
    gfx950: no scratch, no spilled VGPRs, no spilled SGPRs"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "fx.o"),
                        os.path.join(src, "vcfxg_fx.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = r.stderr.decode()
    for kernel, max_vgprs in (("_ZN5vcfxg10k_fx_cellsILb1EEE", 96), ("_ZN5vcfxg10k_fx_cellsILb0EEE", 96),
                              ("_ZN5vcfxg10k_fx_writeE", 112)):
        k = text.index("Function Name: " + kernel)
        vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\w+)",
                               text[k:k + 3000])[:5])
        assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0" and vals["SGPRs Spill"] == "0", \
            (kernel, vals)
        assert int(vals["VGPRs"]) <= max_vgprs and int(vals["Occupancy [waves/SIMD]"]) >= 4, (kernel, vals)
