"""The plain-Python restatement of VCFX_sample_extractor (tests/_sample_extractor_ref.py) against
the compiled reference's recorded bytes (tests/golden/sample_extractor_cases.json.gz, written by
tests/golden/make_sample_extractor_golden.py): stdout, stderr and exit code of every case, byte
for byte.  The restatement is the checker of generated inputs in tests/test_gpu_sx.py."""
import pytest

from tests import _sample_extractor_ref as R
from tests._sample_extractor_cases import GOLDEN, case_stdin, load_cases

CASES = load_cases()


def test_case_list_covers_the_modes():
    names = {c["name"] for c in CASES}
    assert len(names) == len(CASES) >= 100
    for tag in ("one", "none_found", "all", "dup_request", "dup_header", "twice", "space_list", "mixed_list"):
        for mode in ("file", "pos", "stdin"):
            assert "hand.vcf__%s__%s" % (tag, mode) in names
            assert "hand_crlf.vcf__%s__%s" % (tag, mode) in names
    for fx in ("two_chrom", "data_before_chrom", "no_chrom", "chrom8", "chrom9", "hash_inside", "no_final_newline",
               "empty"):
        for mode in ("file", "stdin"):
            assert "%s.vcf__first_last__%s" % (fx, mode) in names
    assert {"missing_file", "no_args", "no_samples_file", "help", "version", "unknown_long"} <= names


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_reference(case):
    out, err, rc = R.run(case["argv"], case_stdin(case), cwd=GOLDEN)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_the_modes_differ_where_the_reference_does():
    """the traps: stdin mode keeps '\\r' (so the last header name does not match on CRLF input),
    skips 8-field lines and selects again at a second '#CHROM' line; file mode does none of it"""
    with open(GOLDEN + "/sample_extractor/hand_crlf.vcf", "rb") as f:
        crlf = f.read()
    fo, fe = R.extract_file(crlf, [b"F"])
    so, se = R.extract_stdin(crlf, [b"F"])
    assert b"not found" not in fe and b"Warning: sample 'F' not found in header.\n" in se
    assert b"\r" not in fo and b"\r\n" in so
    assert fe.count(R.W_NOSAMP) == 0 and se.count(R.W_NOSAMP) == 1
    with open(GOLDEN + "/sample_extractor/two_chrom.vcf", "rb") as f:
        two = f.read()
    assert R.extract_file(two, [b"A"])[0].count(b"#CHROM") == 2  # the second passes through
    assert R.extract_stdin(two, [b"Q"])[0].splitlines()[-1].count(b"\t") == 9  # re-selected: one column


def test_lines_statuses():
    buf = b"\n#x\n#CHROM\ta\n1\t2\n" + b"\t".join([b"f"] * 8) + b"\n" + b"\t".join([b"f"] * 11) + b"\r\n"
    st = [s for s, _ in R.lines(buf, [10, 12], True)]
    assert st == [R.EMPTY, R.HEADER, R.CHROM, R.SHORT, R.NO_SAMPLES, R.ROW]
    rows = R.lines(buf, [10, 12], False)
    assert [s for s, _ in rows] == [R.EMPTY, R.HEADER, R.HEADER, R.SHORT, R.ROW, R.ROW]
    assert rows[4][1] == b"\t".join([b"f"] * 8) + b"\t.\t.\n"
    assert rows[5][1] == b"\t".join([b"f"] * 10) + b"\t.\n"
    assert [s for s, _ in R.lines(buf, [], False, seen=False)][3:] == [R.PRE] * 3
