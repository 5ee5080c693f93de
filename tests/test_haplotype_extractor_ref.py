"""The Python restatement of VCFX_haplotype_extractor (tests/_haplotype_extractor_ref.py) against every
recorded case of the compiled reference (tests/golden/haplotype_extractor_cases.json.gz): stdout,
stderr and exit code, byte for byte, and the device view's text against the same rows."""
import os

import pytest

from tests import _haplotype_extractor_ref as R

CASES = R.load_cases()


def test_cases_cover_the_forms():
    names = {c["name"] for c in CASES}
    assert len(CASES) >= 150
    for n in ("flips.vcf__check_debug_file", "cr_only_line.vcf__stdin", "cr_only_line.vcf__file", "block_0", "block_m1_no_members",
              "block_100000", "block_100001", "empty.vcf__stream_stdin", "no_header.vcf__stream_file", "help", "version"):
        assert n in names, n
    assert any(c["rc"] == 1 for c in CASES) and any(c["stderr"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_the_reference(case):
    assert R.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN) == (case["stdout"], case["stderr"], case["rc"])


def test_device_view_is_the_tools_rows():
    """the block table and the text of the device view are the rows the tool prints"""
    d = os.path.join(R.GOLDEN, "haplotype_extractor")
    seen = 0
    for name in sorted(os.listdir(d)):
        buf = open(os.path.join(d, name), "rb").read()
        for stdin in (False, True):
            for check in (False, True):
                for T in (100000, 0, -1):
                    v = R.device_view(buf, stdin, T, check)
                    out, _, rc = R.extract(buf, stdin, T=T, check=check, quiet=True)
                    if v is None:
                        assert rc == 1 or out.count(b"\n") <= 1, name
                        continue
                    seen += 1
                    assert rc == 0 and out.split(b"\n", 1)[1] == v["text"], name
                    assert sum(b[5] for b in v["blocks"]) == len(v["text"])
                    assert [b[4] for b in v["blocks"]] == [sum(x[5] for x in v["blocks"][:i]) for i in range(len(v["blocks"]))]
                    assert v["status"].count(R.MEMBER) == len(v["fixed"]) == (v["blocks"][-1][1] + 1 if v["blocks"] else 0)
    assert seen > 100


def test_generators_make_what_they_say():
    buf = R.gen_blocks(1, 5, [1, R.TILE_MEMBERS + 1, 3], widths=(1, 3, 300), between=0.5, fixed_blocks=(1,))
    v = R.device_view(buf, False)
    assert [b[1] - b[0] + 1 for b in v["blocks"]] == [1, R.TILE_MEMBERS + 1, 3]
    assert all(v["fixed"][m] for m in range(1, R.TILE_MEMBERS + 2)) and len(set(v["status"])) >= 4
    for at in ((0,), (63,), (64,), (64, 70)):
        v = R.device_view(R.gen_flips(71, at, gap_lines=3), False, check=True)
        assert [f for f in v["flip"] if f >= 0] == [71, 71, at[0], 71] and len(v["blocks"]) == 2
    assert len(R.LONG_GT) == 300
