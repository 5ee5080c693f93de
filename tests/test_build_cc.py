"""CPU checks of the VCFX_cross_sample_concordance build: the engine library exports its entry
points, the tools library exports the tool's entry (declared in include/vcfx_tools.h), the
executable is there, the dispatcher answers help, version and argument errors without a device,
and the multi-GPU plan runs the tool on one context."""
import ctypes
import os
import subprocess

from tests import _concordance_ref as R
from vcfx_amd import BUILD, GPU_LIB, TOOLS_LIB, engine, tool_binary, tools

TOOL = R.TOOL


def test_gpu_lib_exports_concordance():
    lib = ctypes.CDLL(GPU_LIB)
    for name in ("vcfxg_concordance_region", "vcfxg_concordance_totals", "vcfxg_chrom_lines"):
        assert hasattr(lib, name), name
        assert name in engine.SIGNATURES, name
    assert hasattr(engine.Engine, "concordance")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name in ("vcfxg_cc_params", "VCFXG_CC_CONCORDANT", "VCFXG_CC_DISCORDANT", "VCFXG_CC_NO_GENOTYPES"):
        assert name in hdr, name


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_cross_sample_concordance")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_entry_fn vcfx_tool_cross_sample_concordance;" in hdr


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


NO_DEVICE = ([TOOL, "--help"], [TOOL, "-h"], [TOOL, "--version"], [TOOL, "-v"], [TOOL, "-qh"], [TOOL, "--bogus"],
             [TOOL, "-i", "does/not/exist.vcf", "-t", "2"], [TOOL, "-q", "does/not/exist.vcf"], [TOOL, "-x", "-i", "f"],
             [TOOL, "-t"], [TOOL, "--samples"], [TOOL, "--quiet=1"], [TOOL, "-i", "concordance/empty.vcf"],
             [TOOL, "-t", "2", "-i", "concordance/no_chrom.vcf"])


def test_dispatch_knows_the_tool_without_a_device():
    """help, version, argument errors, an unreadable or empty file and a file without '#CHROM'
    need no device: the reference's bytes"""
    for argv in NO_DEVICE:
        assert tools.run(argv, cwd=R.GOLDEN) == R.run(argv, cwd=R.GOLDEN), argv


def test_executable_answers_without_a_device():
    for argv in NO_DEVICE[:8]:
        r = subprocess.run(argv, executable=tool_binary(TOOL), capture_output=True, cwd=R.GOLDEN, timeout=60)
        assert (r.stdout, r.stderr, r.returncode) == R.run(argv, cwd=R.GOLDEN), argv


def test_stdin_without_chrom_needs_no_device():
    for stdin in (b"", b"##fileformat=VCFv4.2\n1\t5\t.\tA\tT\n"):
        assert tools.run([TOOL], stdin) == (R.HEADER, R.E_NOCHROM, 0)
        assert R.run([TOOL], stdin) == (R.HEADER, R.E_NOCHROM, 0)


def test_shard_plan_is_one_context(tmp_path):
    path = tmp_path / "in.vcf"
    path.write_bytes(R.clean_vcf(3, 200, 5))
    for argv in ([TOOL, "-i", str(path)], [TOOL, "-t", "4", str(path)], [TOOL]):
        assert tools.shard_plan(argv, 2)[0] == 1


def test_concordance_walk_compiles_without_scratch(tmp_path):
    """k_af_walk<CcOp> (instantiated in vcfxg_cc.hip) as the compiler builds it for gfx950: no
    scratch, at most 96 VGPRs, five waves per SIMD, as the other walks of its sweep depth"""
    import re
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.access(hipcc, os.X_OK)
    repo = os.path.dirname(BUILD)
    src = os.path.join(repo, "vcfx_amd", "csrc", "gpu")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + src,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "cc.o"),
                        os.path.join(src, "vcfxg_cc.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = r.stderr.decode()
    k = text.index("k_af_walkINS_4CcOp")
    vals = dict(re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill): (\w+)",
                           text[k:k + 3000])[:4])
    assert vals["ScratchSize [bytes/lane]"] == "0" and vals["VGPRs Spill"] == "0", vals
    assert int(vals["VGPRs"]) <= 96 and int(vals["Occupancy [waves/SIMD]"]) == 5, vals
