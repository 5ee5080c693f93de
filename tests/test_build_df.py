"""CPU checks of the VCFX_diff_tool build: the engine library exports its entry points, the tools
library exports the tool's entry (declared in include/vcfx_tools.h), the executable is there, the
dispatcher and the executable give the recorded bytes for help, version, argument errors and files
that cannot be opened without a device, the multi-GPU plan runs the tool on one context, and the new
kernels compile for gfx950 without scratch or spilled registers."""
import ctypes
import os
import re
import subprocess

from tests import _diff_tool_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL
BY = {c["name"]: c for c in R.load_cases()}
NO_DEVICE = ("help", "help_short", "help_with_files", "help_as_a_value", "help_in_group", "help_prefix", "version",
             "version_short", "version_with_files", "no_arguments", "missing_file1_option", "missing_file2_option",
             "empty_file1_value", "only_operands", "bad_long", "bad_short", "ambiguous_long", "missing_argument",
             "missing_argument_long", "flag_with_value", "missing_first", "missing_second", "missing_both",
             "missing_first_sorted", "directory_first", "directory_second", "empty_both__default", "empty_both__s")


def test_gpu_lib_exports_diff():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_diff", "vcfxg_diff_status", "vcfxg_diff_counts", "vcfxg_diff_text"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    for name in ("diff", "diff_text", "diffed_text"):
        assert hasattr(engine.Engine, name)
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name, value in (("VCFXG_DF_EMPTY", R.EMPTY), ("VCFXG_DF_COMMON", R.COMMON), ("VCFXG_DF_UNIQUE", R.UNIQUE),
                        ("VCFXG_DF_SKIPPED", R.SKIPPED), ("VCFXG_DF_HEADER", R.HEADER), ("VCFXG_DF_REPEAT", R.REPEAT),
                        ("VCFXG_DF_WINDOW", R.WINDOW), ("VCFXG_DF_PATH_HASH", R.PATH_HASH),
                        ("VCFXG_DF_PATH_BOUNDS", R.PATH_BOUNDS), ("VCFXG_DF_PATH_WALK", R.PATH_WALK)):
        assert re.search(r"#define %s %d\n" % (name, value), hdr), name
    assert re.search(r"typedef struct \{\s*uint64_t second_start;[^}]*int assume_sorted;[^}]*int natural;[^}]*uint32_t hash_bits;[^}]*\} "
                     r"vcfxg_df_params;", hdr)
    assert "VCFXG_DF_BLOCK" in hdr and "VCFXG_DF_WALK_STEPS" in hdr
    assert "EACH SIDE\n * IS IN INPUT ORDER OF THE KEY'S FIRST LINE" in hdr
    assert ctypes.sizeof(engine.DfParams) == 24


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_diff_tool")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_diff_tool;" in hdr
    assert TOOL in TOOLS


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


def test_dispatch_gives_the_recorded_bytes_without_a_device():
    for name in NO_DEVICE:
        c = BY[name]
        assert not c["env"]
        assert tools.run(c["argv"], b"", cwd=R.GOLDEN) == (c["stdout"], c["stderr"], c["rc"]), name
    assert BY["missing_second"]["stderr"] == b"Error: Unable to open file diff_tool/does_not_exist.vcf\n"
    assert BY["missing_both"]["stderr"] == b"Error: Unable to open file diff_tool/does_not_exist_1.vcf\n"  # (only the first)
    assert BY["directory_second"]["stderr"] == b"Error: Unable to open file diff_tool\n" and BY["directory_second"]["rc"] == 1
    assert BY["no_arguments"]["rc"] == 1 and BY["bad_short"]["rc"] == 0


def test_executable_gives_the_recorded_bytes_without_a_device():
    for name in NO_DEVICE:
        c = BY[name]
        r = subprocess.run(c["argv"], executable=tool_binary(TOOL), input=b"", capture_output=True, cwd=R.GOLDEN, timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == (c["stdout"], c["stderr"], c["rc"]), name


def test_shard_plan_is_one_context(tmp_path):
    a, b = tmp_path / "a.vcf", tmp_path / "b.vcf"
    a.write_bytes(R.gen_file(1, 200))
    b.write_bytes(R.gen_file(2, 200))
    for argv in ([TOOL, "-a", str(a), "-b", str(b)], [TOOL, "-s", "-n", "-a", str(a), "-b", str(b)], [TOOL]):
        assert tools.shard_plan(argv, 2)[0] == 1  # a join of two inputs does not shard


def test_kernels_compile_without_scratch(tmp_path):
    """every kernel of vcfxg_df.hip as the compiler builds it for gfx950: no scratch, no spilled VGPRs,
    no spilled SGPRs, at least 7 waves per SIMD (k_df_walk runs one lane of one wave: its occupancy
    means nothing and is not asserted)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "df.o"),
                        os.path.join(src, "vcfxg_df.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = r.stderr.decode()
    kernels = ("8k_df_cutE", "8k_df_keyE", "13k_df_key_waveE", "9k_df_textE", "14k_df_text_waveE", "10k_df_pairsE",
               "11k_df_verifyE", "12k_df_resolveE", "11k_df_first2E", "11k_df_decideE", "12k_df_orderedE", "11k_df_boundsE",
               "9k_df_walkE", "10k_df_drainE", "9k_df_flagE", "10k_df_placeE", "8k_df_sumE")
    assert len(re.findall(r"Function Name: _ZN5vcfxg\d+k_df_", text)) == len(kernels)
    for kernel in kernels:
        k = text.index("Function Name: _ZN5vcfxg" + kernel)
        vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\w+)",
                               text[k:k + 3000])[:5])
        assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0" and vals["SGPRs Spill"] == "0", \
            (kernel, vals)
        if kernel != "9k_df_walkE":
            assert int(vals["Occupancy [waves/SIMD]"]) >= 7, (kernel, vals)
