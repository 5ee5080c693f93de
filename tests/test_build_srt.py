"""CPU checks of the VCFX_sorter build: the engine library exports its entry points, the tools
library exports the tool's entry (declared in include/vcfx_tools.h), the executable is there, the
dispatcher gives the recorded bytes for help, version, argument errors, a missing file, an empty
file and an empty stdin without a device, the multi-GPU plan runs the tool on one context, and the
new kernels compile for gfx950 without scratch or spilled registers."""
import ctypes
import os
import re
import subprocess

from tests import _sorter_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL
BY = {c["name"]: c for c in R.load_cases()}
NO_DEVICE = ("help", "help_short", "help_with_input", "help_in_group", "help_prefix", "version", "version_short", "bad_long",
             "bad_short", "bad_short_stdin", "missing_argument", "missing_argument_long", "natural_with_value",
             "missing_file", "missing_file_natural", "dash_is_a_file_name", "empty.vcf__file", "empty.vcf__natural_file",
             "empty.vcf__stdin", "empty.vcf__natural_stdin")


def test_gpu_lib_exports_sort():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_sort", "vcfxg_sort_status", "vcfxg_sort_counts", "vcfxg_sort_order", "vcfxg_sort_text"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    for name in ("sort", "sort_text", "sorted_text"):
        assert hasattr(engine.Engine, name)
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name, value in (("VCFXG_SRT_EMPTY", R.EMPTY), ("VCFXG_SRT_KEPT", R.KEPT), ("VCFXG_SRT_PRE", R.PRE),
                        ("VCFXG_SRT_BAD", R.BAD), ("VCFXG_SRT_HEADER", R.HEADER), ("VCFXG_SRT_WINDOW", R.WINDOW)):
        assert re.search(r"#define %s %d\n" % (name, value), hdr), name
    assert "vcfxg_srt_params" in hdr and "int natural;" in hdr and "VCFXG_SRT_BLOCK" in hdr
    assert "EQUAL KEYS\n * KEEP THEIR INPUT ORDER" in hdr


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_sorter")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_sorter;" in hdr
    assert TOOL in TOOLS


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


def test_dispatch_gives_the_recorded_bytes_without_a_device():
    for name in NO_DEVICE:
        c = BY[name]
        assert tools.run(c["argv"], R.case_stdin(c) if name.startswith("empty") else b"", cwd=R.GOLDEN) == \
            (c["stdout"], c["stderr"], c["rc"]), name
    assert BY["missing_file"]["stderr"] == b"Error: cannot open file 'sorter/does_not_exist.vcf'\n" and BY["missing_file"]["rc"] == 1
    assert BY["empty.vcf__file"]["stdout"] == BY["empty.vcf__stdin"]["stdout"] == b""


def test_executable_gives_the_recorded_bytes_without_a_device():
    for name in NO_DEVICE[:3] + NO_DEVICE[5:8] + NO_DEVICE[13:14] + NO_DEVICE[16:17] + NO_DEVICE[18:19]:
        c = BY[name]
        r = subprocess.run(c["argv"], executable=tool_binary(TOOL), input=b"", capture_output=True, cwd=R.GOLDEN, timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == (c["stdout"], c["stderr"], c["rc"]), name


def test_shard_plan_is_one_context(tmp_path):
    path = tmp_path / "in.vcf"
    path.write_bytes(R.generated("mix"))
    for argv in ([TOOL, str(path)], [TOOL, "-n", str(path)], [TOOL, str(path), str(path)], [TOOL]):
        assert tools.shard_plan(argv, 2)[0] == 1  # an order over all records does not shard


def test_kernels_compile_without_scratch(tmp_path):
    """the key kernels (lane pass and wave pass), the class pass and the gather (vcfxg_gather.hip: the
    ordered-text stage the merger and the diff tool share) as the compiler builds them for gfx950: no
    scratch, no spilled VGPRs, no spilled SGPRs"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    for unit, kernels in (("vcfxg_srt.hip", (("9k_srt_keyE", 48), ("14k_srt_key_waveE", 48), ("11k_srt_classE", 32),
                                             ("13k_srt_scatterE", 32), ("10k_srt_wordE", 32))),
                          ("vcfxg_gather.hip", (("10k_line_lenE", 32), ("13k_text_gatherILi0EEE", 48),
                                                ("13k_text_gatherILi1EEE", 48), ("13k_text_gatherILi2EEE", 48),
                                                ("13k_text_gatherILi3EEE", 48)))):
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                            "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                            "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "unit.o"),
                            os.path.join(src, unit)], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        text = r.stderr.decode()
        for kernel, max_vgprs in kernels:
            k = text.index("Function Name: _ZN5vcfxg" + kernel)
            vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\w+)",
                                   text[k:k + 3000])[:5])
            assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0" and vals["SGPRs Spill"] == "0", \
                (kernel, vals)
            assert int(vals["VGPRs"]) <= max_vgprs and int(vals["Occupancy [waves/SIMD]"]) >= 7, (kernel, vals)
