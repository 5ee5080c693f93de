"""The record walk with its chunk layout passed by value (WalkLayout, vcfxg_walk_layout.h) as the
compiler builds it for gfx950 (no GPU needed): the layout's arithmetic is scalar and its struct
stays in the kernel arguments, so the depth-10 AF walk keeps 4 waves per SIMD with no scratch, and
every other instantiation its occupancy too.  Read from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) on vcfxg_af_walk.hip, device code only."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(REPO, "vcfx_amd", "csrc", "gpu")

WAVES = {  # template arguments as mangled -> waves per SIMD
    "4AfOpELb0ELi6ELb0E": 5,
    "4AfOpELb0ELi6ELb1E": 5,
    "4AfOpELb0ELi8ELb1E": 5,
    "4AfOpELb0ELi10ELb1E": 4,  # the bench shard's walk
    "4AfOpELb0ELi12ELb1E": 4,
    "4AfOpELb1ELi6ELb0E": 4,
    "5HweOpELb0ELi6ELb0E": 5,
    "10DoseWalkOpELb0ELi6ELb0E": 5,
    "10DoseHeadOpELb0ELi6ELb0E": 5,
}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.fail("no hipcc at %s" % HIPCC)
    out = tmp_path_factory.mktemp("walklayout") / "af_walk.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-I" + os.path.join(REPO, "include"), "-I" + SRC,
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(out),
                        os.path.join(SRC, "vcfxg_af_walk.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    table, cur = {}, None
    for line in r.stderr.decode().splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = table.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|"
                      r"SGPRs Spill|Dynamic Stack): (\w+)", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return {k: v for k, v in table.items() if "k_af_walkINS_" in k}


def test_every_walk_takes_the_layout_by_value(remarks):
    assert len(remarks) == len(WAVES)
    for name in remarks:  # (const char *, long, long, vcfxg::WalkLayout, int, ...)
        assert re.search(r"EEvPKcllNS_10WalkLayoutEil", name), name


@pytest.mark.parametrize("inst", sorted(WAVES))
def test_no_scratch_and_the_same_waves(remarks, inst):
    (r,) = [v for k, v in remarks.items() if "k_af_walkINS_" + inst + "EEvPKc" in k]
    assert r["ScratchSize [bytes/lane]"] == "0" and r["VGPRs Spill"] == "0" and r["Dynamic Stack"] == "False", r
    assert int(r["Occupancy [waves/SIMD]"]) == WAVES[inst], r
