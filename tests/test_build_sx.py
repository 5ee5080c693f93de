"""CPU checks of the VCFX_sample_extractor build: the engine library exports its entry point,
the tools library exports the tool's entry (declared in include/vcfx_tools.h), the executable is
there, the dispatcher and the multi-GPU plan know the tool; no GPU is needed for these."""
import ctypes
import os

from vcfx_amd import BUILD, GPU_LIB, TOOLS_LIB, engine, tool_binary, tools

TOOL = "VCFX_sample_extractor"


def test_gpu_lib_exports_sample_extract():
    assert hasattr(ctypes.CDLL(GPU_LIB), "vcfxg_sample_extract")
    assert "vcfxg_sample_extract" in engine.SIGNATURES
    assert hasattr(engine.Engine, "sample_extract")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_gpu.h")).read()
    for name in ("vcfxg_sx_params", "VCFXG_SX_ROW", "VCFXG_SX_SHORT", "VCFXG_SX_NO_SAMPLES", "VCFXG_SX_PRE",
                 "VCFXG_SX_CHROM", "VCFXG_SX_BLOCK"):
        assert name in hdr, name


def test_tools_lib_exports_the_tool():
    assert hasattr(ctypes.CDLL(TOOLS_LIB), "vcfx_tool_sample_extractor")
    hdr = open(os.path.join(os.path.dirname(BUILD), "include", "vcfx_tools.h")).read()
    assert "vcfx_tool_sample_extractor;" in hdr


def test_binary_present():
    assert os.access(tool_binary(TOOL), os.X_OK)


def test_dispatch_knows_the_tool_without_a_device():
    """help, version and argument errors need no device: the reference's bytes"""
    from tests import _sample_extractor_ref as R
    for argv in ([TOOL], [TOOL, "--help"], [TOOL, "--version"], [TOOL, "-i", "nothing.vcf"],
                 [TOOL, "-s", "A", "-i", "does/not/exist.vcf"], [TOOL, "-s", "A", "--bogus"]):
        assert tools.run(argv) == R.run(argv), argv


def test_shard_plan_takes_a_record_view(tmp_path):
    from tests import _sample_extractor_ref as R
    path = tmp_path / "in.vcf"
    path.write_bytes(R.ragged_vcf(3, 200, 5))
    for argv in ([TOOL, "-s", "S1", "-i", str(path)], [TOOL, "--samples=S1,S2", str(path)]):
        w, kind, cuts = tools.shard_plan(argv, 2)
        assert (w, kind) == (2, 1) and cuts[0] < cuts[1] < cuts[2]
    assert tools.shard_plan([TOOL, "-s", "S1"], 2)[0] == 1  # stdin: one context
