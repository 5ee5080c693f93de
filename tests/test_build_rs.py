"""CPU checks of the VCFX_region_subsampler build: the engine library exports its entry points, the
tools library exports the tool's entry (declared in include/vcfx_tools.h), the executable is there,
the dispatcher answers help, version, argument errors, an unreadable BED or input and an empty input
without a device, the multi-GPU plan runs the tool on one context, and the table and class kernels
compile for gfx950 without scratch or spilled registers."""
import ctypes
import os
import re
import subprocess

from tests import _region_subsampler_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL
D = "region_subsampler/"


def test_gpu_lib_exports_the_entry_points():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_regions_load", "vcfxg_regions_merged", "vcfxg_region_filter", "vcfxg_region_status",
                 "vcfxg_region_counts"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    for name in ("regions_load", "regions_merged", "region_filter"):
        assert hasattr(engine.Engine, name)
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name, value in (("VCFXG_RS_EMPTY", R.EMPTY), ("VCFXG_RS_HEADER", R.HEADER), ("VCFXG_RS_IN", R.IN),
                        ("VCFXG_RS_OUT", R.OUT), ("VCFXG_RS_EARLY", R.EARLY), ("VCFXG_RS_SHORT", R.SHORT),
                        ("VCFXG_RS_BADPOS", R.BADPOS), ("VCFXG_RS_WINDOW", R.WINDOW)):
        assert re.search(r"#define %s %d\n" % (name, value), hdr), name
    assert "vcfxg_rs_params" in hdr and "hash_bits" in hdr


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_region_subsampler")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_region_subsampler;" in hdr
    assert TOOL in TOOLS


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


NO_DEVICE = ([TOOL, "--help"], [TOOL, "-h"], [TOOL, "--version"], [TOOL, "-v"], [TOOL, "-qh"], [TOOL, "--bogus"],
             [TOOL, "-i", D + "line_mix.vcf"], [TOOL, "-q"], [TOOL, "-b"], [TOOL, "--region-bed"], [TOOL, "-b", ""],
             [TOOL, "-b", D + "does_not_exist.bed", "-i", D + "line_mix.vcf"],
             [TOOL, "-b", D + "mix.bed", "-i", D + "does_not_exist.vcf"],
             [TOOL, "-b", D + "bed_forms.bed", "-i", D + "does_not_exist.vcf"],
             [TOOL, "-x", "-b", D + "mix.bed"], [TOOL, "--quiet=1", "-b", D + "mix.bed"],
             [TOOL, "-b", D + "mix.bed", "-i", D + "empty.vcf"], [TOOL, "-q", "-b", D + "bed_forms.bed", "-i", D + "empty.vcf"],
             [TOOL, "-b", "region_subsampler", "-i", D + "empty.vcf"])


def test_dispatch_knows_the_tool_without_a_device():
    """help, version, argument errors, an unreadable BED or input and an empty file need no device:
    the reference's bytes"""
    for argv in NO_DEVICE:
        assert tools.run(argv, cwd=R.GOLDEN) == R.run(argv, cwd=R.GOLDEN), argv
    assert tools.run([TOOL, "-b", "nope.bed"], cwd=R.GOLDEN) == \
        (b"", b"Error: cannot open BED nope.bed\nError: failed to load regions from nope.bed\n", 1)
    out, err, rc = tools.run([TOOL, "-b", D + "bed_forms.bed", "-i", "nope.vcf"], cwd=R.GOLDEN)
    assert (out, rc) == (b"", 1) and err.count(b"Warning: skipping invalid bed line") >= 8
    assert err.endswith(b"Error: failed to process input file: nope.vcf\n")


def test_executable_answers_without_a_device():
    for argv in NO_DEVICE[:13]:
        r = subprocess.run(argv, executable=tool_binary(TOOL), capture_output=True, cwd=R.GOLDEN, timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == R.run(argv, cwd=R.GOLDEN), argv


def test_empty_stdin_needs_no_device():
    bed = os.path.join(R.GOLDEN, "region_subsampler", "mix.bed")
    assert tools.run([TOOL, "-b", bed], b"") == (b"", b"", 0) == R.run([TOOL, "-b", bed], b"")
    assert tools.run([TOOL, "-q", "-b", bed], b"") == (b"", b"", 0)
    forms = os.path.join(R.GOLDEN, "region_subsampler", "bed_forms.bed")
    assert tools.run([TOOL, "-b", forms], b"") == R.run([TOOL, "-b", forms], b"")


def test_shard_plan_is_one_context(tmp_path):
    path, bed = tmp_path / "in.vcf", tmp_path / "in.bed"
    buf, b = R.generated("g600")
    path.write_bytes(buf)
    bed.write_bytes(b)
    for argv in ([TOOL, "-b", str(bed), "-i", str(path)], [TOOL, "-q", "-b", str(bed), "-i", str(path)], [TOOL, "-b", str(bed)]):
        assert tools.shard_plan(argv, 2)[0] == 1  # the header flag is state along the lines: not sharded


def test_kernels_compile_without_scratch(tmp_path):
    """the table kernels (keys, the scan's three, bounds, rows, dictionary) and the class kernels (lane
    pass, wave pass, finish) as the compiler builds them for gfx950: no scratch, no spilled VGPRs, no
    spilled SGPRs"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "rs.o"),
                        os.path.join(src, "vcfxg_rs.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = r.stderr.decode()
    for kernel, max_vgprs in (("k_rs_keys", 32), ("k_rs_sorted", 32), ("k_rs_tile_max", 32), ("k_rs_carry", 40),
                              ("k_rs_reach", 40), ("k_rs_bounds", 32), ("k_rs_rows", 32), ("k_rs_dict", 32),
                              ("k_rs_class", 72), ("k_rs_class_wave", 72), ("k_rs_finish", 32)):
        k = text.index("Function Name: _ZN5vcfxg%d%sE" % (len(kernel), kernel))
        vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\w+)",
                               text[k:k + 3000])[:5])
        assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0" and vals["SGPRs Spill"] == "0", \
            (kernel, vals)
        assert int(vals["VGPRs"]) <= max_vgprs and int(vals["Occupancy [waves/SIMD]"]) >= 7, (kernel, vals)
