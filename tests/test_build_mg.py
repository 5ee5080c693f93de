"""CPU checks of the VCFX_merger build: the engine library exports its entry points, the tools library
exports the tool's entry (declared in include/vcfx_tools.h), the executable is there, the dispatcher
and the executable give the recorded bytes for help, version, argument errors, files that cannot be
opened and empty files without a device, the multi-GPU plan runs the tool on one context, and the new
kernels compile for gfx950 without scratch or spilled registers."""
import ctypes
import os
import re
import subprocess

from tests import _merger_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL
BY = {c["name"]: c for c in R.load_cases()}
NO_DEVICE = ("help", "help_short", "help_with_files", "help_as_a_value", "help_in_group", "help_prefix", "version",
             "version_short", "version_with_files", "no_arguments", "no_merge_option", "only_operands", "bad_long", "bad_short",
             "unknown_prefix", "missing_argument", "missing_argument_long", "flag_with_value", "missing_all__default",
             "missing_all__s", "empty_files__default", "empty_files__s", "directory_only__default", "directory_only__s",
             "empty_name_only", "only_commas")


def test_gpu_lib_exports_merge():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_merge", "vcfxg_merge_status", "vcfxg_merge_counts", "vcfxg_merge_files", "vcfxg_merge_order",
                 "vcfxg_merge_text"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    for name in ("merge", "merge_files", "merge_text", "merged_text"):
        assert hasattr(engine.Engine, name)
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name, value in (("VCFXG_MG_EMPTY", R.EMPTY), ("VCFXG_MG_KEPT", R.KEPT), ("VCFXG_MG_BAD", R.BAD),
                        ("VCFXG_MG_HEADER", R.HEADER), ("VCFXG_MG_DROPPED", R.DROPPED), ("VCFXG_MG_WINDOW", R.WINDOW),
                        ("VCFXG_MG_PATH_SORT", R.PATH_SORT), ("VCFXG_MG_PATH_WALK", R.PATH_WALK)):
        assert re.search(r"#define %s %d\n" % (name, value), hdr), name
    assert re.search(r"typedef struct \{\s*const uint64_t \*file_start;[^}]*uint32_t n_files;[^}]*int assume_sorted;[^}]*"
                     r"int natural;[^}]*\} vcfxg_mg_params;", hdr)
    assert "VCFXG_MG_WALK_STEPS" in hdr and "VCFXG_SRT_BLOCK" in hdr
    assert "EQUAL KEYS COME OUT IN (FILE LIST ORDER, LINE ORDER)" in hdr
    assert ctypes.sizeof(engine.MgParams) == 24


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_merger")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_merger;" in hdr
    assert TOOL in TOOLS


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


def test_dispatch_gives_the_recorded_bytes_without_a_device():
    for name in NO_DEVICE:
        c = BY[name]
        assert not c["env"]
        assert tools.run(c["argv"], b"", cwd=R.GOLDEN) == (c["stdout"], c["stderr"], c["rc"]), name
    assert BY["missing_all__s"]["stderr"] == b"Failed to open file: merger/does_not_exist_1.vcf\n" \
        b"Failed to open file: merger/does_not_exist_2.vcf\n"
    assert BY["only_commas"]["stderr"] == b"Failed to open file: \n" * 3 and BY["only_commas"]["stdout"] == b""
    assert BY["no_arguments"]["rc"] == 0 and BY["bad_short"]["rc"] == 0 and BY["no_arguments"]["stdout"] == R.HELP
    assert BY["directory_only__default"]["stderr"] == b""


def test_executable_gives_the_recorded_bytes_without_a_device():
    for name in NO_DEVICE:
        c = BY[name]
        r = subprocess.run(c["argv"], executable=tool_binary(TOOL), input=b"", capture_output=True, cwd=R.GOLDEN, timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == (c["stdout"], c["stderr"], c["rc"]), name


def test_shard_plan_is_one_context(tmp_path):
    files = R.deal(R.gen_records(1, 200), 2, natural=False)
    a, b = tmp_path / "a.vcf", tmp_path / "b.vcf"
    a.write_bytes(files[0])
    b.write_bytes(files[1])
    m = "%s,%s" % (a, b)
    for argv in ([TOOL, "-m", m], [TOOL, "-s", "-n", "-m", m], [TOOL]):
        assert tools.shard_plan(argv, 2)[0] == 1  # one order over all records does not shard


def test_kernels_compile_without_scratch(tmp_path):
    """every kernel of vcfxg_mg.hip as the compiler builds it for gfx950: no scratch, no spilled VGPRs,
    no spilled SGPRs, at least 7 waves per SIMD (k_mg_walk and k_mg_hdr run one wave: their occupancy
    means nothing; k_mg_walk's is not asserted)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "mg.o"),
                        os.path.join(src, "vcfxg_mg.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = r.stderr.decode()
    kernels = ("8k_mg_cutE", "8k_mg_keyE", "13k_mg_key_waveE", "8k_mg_hdrE", "10k_mg_classE", "12k_mg_orderedE",
               "12k_mg_scatterE", "9k_mg_partE", "14k_mg_walk_initE", "9k_mg_walkE")
    assert len(re.findall(r"Function Name: _ZN5vcfxg\d+k_mg_", text)) == len(kernels)
    for kernel in kernels:
        k = text.index("Function Name: _ZN5vcfxg" + kernel)
        vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\w+)",
                               text[k:k + 3000])[:5])
        assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0" and vals["SGPRs Spill"] == "0", \
            (kernel, vals)
        if kernel != "9k_mg_walkE":
            assert int(vals["Occupancy [waves/SIMD]"]) >= 7, (kernel, vals)
