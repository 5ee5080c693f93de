"""The record walk's instantiations as the compiler builds them for gfx950 (no GPU needed): every
k_af_walk kernel -- the AF GT-only walk's sweep depths and the walks that keep their sweep --
compiles without scratch, at the VGPR count and the waves per SIMD that DESIGN §3 tabulates.
Read from the compiler's own remarks (-Rpass-analysis=kernel-resource-usage) on
vcfxg_af_walk.hip, device code only."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(REPO, "vcfx_amd", "csrc", "gpu")

# template arguments as mangled -> (VGPRs at most, waves per SIMD)
AF_DEPTHS = {
    "4AfOpELb0ELi6ELb0E": (96, 5),    # the batches of 6: every record size but the measured ones
    "4AfOpELb0ELi6ELb1E": (96, 5),    # rolling, non-temporal sweeps
    "4AfOpELb0ELi8ELb1E": (96, 5),
    "4AfOpELb0ELi10ELb1E": (128, 4),
    "4AfOpELb0ELi12ELb1E": (128, 4),
}
OTHER_WALKS = {  # unchanged by the depths: exactly these
    "4AfOpELb1ELi6ELb0E": (117, 4),        # GT-first
    "5HweOpELb0ELi6ELb0E": (91, 5),
    "10DoseWalkOpELb0ELi6ELb0E": (96, 5),
    "10DoseHeadOpELb0ELi6ELb0E": (96, 5),
}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.fail("no hipcc at %s" % HIPCC)
    out = tmp_path_factory.mktemp("afwalk") / "af_walk.o"
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
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|"
                      r"Dynamic Stack): (\w+)", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return {re.search(r"k_af_walkINS_(\w+?)EEvPKc", k).group(1): v for k, v in table.items() if "k_af_walkINS_" in k}


def test_every_walk_instantiation_is_listed(remarks):
    assert set(remarks) == set(AF_DEPTHS) | set(OTHER_WALKS)


@pytest.mark.parametrize("inst", sorted(AF_DEPTHS) + sorted(OTHER_WALKS))
def test_no_scratch_and_planned_occupancy(remarks, inst):
    r = remarks[inst]
    vgprs, waves = {**AF_DEPTHS, **OTHER_WALKS}[inst]
    assert r["ScratchSize [bytes/lane]"] == "0" and r["VGPRs Spill"] == "0" and r["Dynamic Stack"] == "False", r
    assert int(r["Occupancy [waves/SIMD]"]) == waves, r
    if inst in OTHER_WALKS:
        assert int(r["VGPRs"]) == vgprs, r
    else:
        assert int(r["VGPRs"]) <= vgprs, r
