"""The numpy restatement of VCFX_inbreeding_calculator (tests/_inbreeding_ref.py) against the
compiled reference's recorded bytes (tests/golden/inbreeding_cases.json.gz, written by
tests/golden/make_inbreeding_golden.py): stdout, stderr and exit code of every case, byte for
byte.  The restatement is the checker of generated inputs in tests/test_gpu_ib.py."""
import pytest

from tests import _inbreeding_ref as R
from tests._inbreeding_cases import GOLDEN, case_input, load_cases

CASES = load_cases()


def test_case_list_covers_the_modes():
    names = {c["name"] for c in CASES}
    assert len(names) == len(CASES) >= 100
    for tag in ("default", "global", "skip", "skipcount", "globalskip"):
        for mode in ("file", "pos", "stdin"):
            assert "hand.vcf__%s__%s" % (tag, mode) in names


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_reference(case, tmp_path):
    stdin, cwd = case_input(case, tmp_path)
    out, err, rc = R.run(case["argv"], stdin, cwd=cwd)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_gt_code_odd_fields():
    want = {b"0/0": 0, b"0|1": 1, b"1/0": 1, b"1|1": 2, b"./.": -1, b".": -1, b"0/.": -1, b"./1": -1, b"2/1": -1,
            b"0/1/1": 1, b" 0/1": 1, b"1|0:5": 1, b"0/1x": 1, b"10/0": -1, b"01/1": 2, b"": -1, b"1": -1, b"\r1/1": 2,
            b"0:1/1": -1, b"0/0 ": 0}
    for f, c in want.items():
        assert R.gt_code(f) == c, f


def test_file_mode_keeps_stale_codes_and_stdin_mode_does_not():
    with open(GOLDEN + "/inbreeding/hand.vcf", "rb") as f:
        buf = f.read()
    a, b = R.accumulate_file(buf), R.accumulate_stdin(buf)
    assert b.variants == a.variants + 1  # the record with an empty ALT counts in stdin mode only
    assert (a.used > b.used).any()  # the samples past the short records' columns
