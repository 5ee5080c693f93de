"""CPU checks of the VCFX_duplicate_remover build: the engine library exports its entry points, the
tools library exports the tool's entry (declared in include/vcfx_tools.h), the executable is there,
the dispatcher answers help, version and argument errors without a device, the multi-GPU plan runs
the tool on one context, and the key and verify kernels compile for gfx950 without scratch."""
import ctypes
import os
import re
import subprocess

from tests import _duplicate_remover_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL


def test_gpu_lib_exports_dedup():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_dedup", "vcfxg_dedup_status", "vcfxg_dedup_counts"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    assert hasattr(engine.Engine, "dedup")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name, value in (("VCFXG_DD_EMPTY", R.EMPTY), ("VCFXG_DD_KEPT", R.KEPT), ("VCFXG_DD_DUP", R.DUP),
                        ("VCFXG_DD_SHORT", R.SHORT), ("VCFXG_DD_HEADER", R.HEADER), ("VCFXG_DD_WINDOW", R.WINDOW)):
        assert re.search(r"#define %s %d\n" % (name, value), hdr), name
    assert "vcfxg_dd_params" in hdr and "hash_bits" in hdr


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_duplicate_remover")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_duplicate_remover;" in hdr


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


NO_DEVICE = ([TOOL, "--help"], [TOOL, "-h"], [TOOL, "--version"], [TOOL, "-v"], [TOOL, "-qh"], [TOOL, "--bogus"],
             [TOOL, "-i", "does/not/exist.vcf"], [TOOL, "-q", "does/not/exist.vcf"], [TOOL, "-x", "-i", "f"],
             [TOOL, "-i"], [TOOL, "--input"], [TOOL, "--quiet=1"], [TOOL, "-i", "duplicate_remover/empty.vcf"],
             [TOOL, "duplicate_remover/empty.vcf", "-q"])


def test_dispatch_knows_the_tool_without_a_device():
    """help, version, argument errors, an unreadable and an empty file need no device: the
    reference's bytes"""
    for argv in NO_DEVICE:
        assert tools.run(argv, cwd=R.GOLDEN) == R.run(argv, cwd=R.GOLDEN), argv
    assert tools.run([TOOL, "-i", "does/not/exist.vcf"], cwd=R.GOLDEN) == \
        (b"", b"Error: Cannot open file: does/not/exist.vcf\n", 1)


def test_executable_answers_without_a_device():
    for argv in NO_DEVICE[:8]:
        r = subprocess.run(argv, executable=tool_binary(TOOL), capture_output=True, cwd=R.GOLDEN, timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == R.run(argv, cwd=R.GOLDEN), argv


def test_empty_stdin_needs_no_device():
    assert tools.run([TOOL], b"") == (b"", b"", 0) == R.run([TOOL], b"")
    assert tools.run([TOOL, "-q"], b"") == (b"", b"", 0)


def test_shard_plan_is_one_context(tmp_path):
    path = tmp_path / "in.vcf"
    path.write_bytes(R.generated("g600"))
    for argv in ([TOOL, "-i", str(path)], [TOOL, "-q", str(path)], [TOOL]):
        assert tools.shard_plan(argv, 2)[0] == 1  # a global key set does not shard


def test_kernels_compile_without_scratch(tmp_path):
    """the key kernels (lane pass and wave pass) and the verify kernels as the compiler builds them
    for gfx950: no scratch, no spilled VGPRs, no spilled SGPRs"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "dd.o"),
                        os.path.join(src, "vcfxg_dd.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = r.stderr.decode()
    for kernel, max_vgprs in (("k_dd_key", 72), ("k_dd_key_wave", 72), ("k_dd_verify", 64), ("k_dd_resolve", 64)):
        k = text.index("Function Name: _ZN5vcfxg%d%sE" % (len(kernel), kernel))
        vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\w+)",
                               text[k:k + 3000])[:5])
        assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0" and vals["SGPRs Spill"] == "0", \
            (kernel, vals)
        assert int(vals["VGPRs"]) <= max_vgprs and int(vals["Occupancy [waves/SIMD]"]) >= 7, (kernel, vals)
