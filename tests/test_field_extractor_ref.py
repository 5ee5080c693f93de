"""The plain-Python restatement of VCFX_field_extractor (tests/_field_extractor_ref.py) reproduces every
golden case recorded from the compiled reference, in stdout, stderr and exit code: this holds the
checker of the GPU tests to the reference.  Also: what the goldens must cover, and that the matrix and
the text of the restatement agree."""
import os

import pytest

from tests import _field_extractor_ref as R

CASES = R.load_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    out, err, rc = R.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_goldens_cover_the_rules():
    assert len(CASES) >= 100 and all(c["rc"] in (0, 1) for c in CASES)
    names = {c["name"] for c in CASES}
    for fx in ("rules.vcf", "rules_crlf.vcf", "rules_no_final_newline.vcf", "header_only.vcf", "empty.vcf", "data_first.vcf",
               "second_chrom.vcf", "no_header.vcf", "generated.vcf"):
        assert any(n.startswith(fx + "+") and n.endswith("__file") for n in names), fx
        assert any(n.startswith(fx + "+") and n.endswith("__stdin") for n in names), fx
    for n in ("repeated_f", "empty_items", "i_dash", "positional_file", "no_fields", "missing_file", "bad_long", "help", "version"):
        assert n in names
    # no case holds a field on which the reference aborts
    for c in CASES:
        fields = ",".join(v for k, v, _ in R.getopt_long(c["argv"])[0] if k == "f").split(",")
        assert R.bad_field(fields) is None, c["name"]
    # the two modes disagree on the rules fixture for every list
    by = {c["name"]: c for c in CASES}
    for tag in ("keys", "samples", "mixed"):
        assert by["rules.vcf+%s__file" % tag]["stdout"] != by["rules.vcf+%s__stdin" % tag]["stdout"]
    text = by["rules.vcf+samples__stdin"]["stdout"]
    assert b"\nzz\t" in text and b"\t\t" in text  # INFO before the sample field; an empty value printed as nothing
    assert b"\nzz\t" not in by["rules.vcf+samples__file"]["stdout"]
    with open(os.path.join(R.GOLDEN, "field_extractor", "rules.vcf"), "rb") as f:
        nf = {ln.count(b"\t") + 1 for ln in f.read().split(b"\n") if ln and ln[:1] != b"#"}
    assert {1, 2, 8, 9, 10} <= nf


def test_rejected_fields():
    for f in ("S:GT", "S99999999999:GT", "S2147483648:", "S:"):
        for argv in ([R.TOOL, "-f", "CHROM," + f], [R.TOOL, "-f", f, "-i", "field_extractor/does_not_exist.vcf"]):
            assert R.run(argv, b"", cwd=R.GOLDEN) == (b"", b"Error: invalid sample index in field '" + f.encode() + b"'\n", 1)
    assert R.run([R.TOOL, "-f", "S,S99999999999"], b"1\t2\n")[2] == 0  # (no colon: INFO keys)
    assert R.run([R.TOOL, "-h", "-f", "S:GT"])[2] == 0 and R.run([R.TOOL, "-x", "-f", "S:GT"])[2] == 0  # the help comes first


@pytest.mark.parametrize("name", sorted(R.GENERATED))
def test_matrix_and_text_agree(name):
    buf = R.generated(name)
    fields = R.GEN_FIELDS.split(",")
    for stdin in (False, True):
        st, rows = R.statuses(buf, fields, stdin), R.cells(buf, fields, stdin)
        assert st.count(R.ROW) == len(rows) and all(len(r) == len(fields) for r in rows)
        text = R.rows(buf, fields, stdin)
        assert text.count(b"\n") == len(rows)
        assert sum(sum(1 if c[1] >= R.ONE else c[1] for c in r) + len(r) for r in rows) == len(text)
        assert R.run([R.TOOL, "-f", R.GEN_FIELDS], buf)[0] == R.header_row(fields) + R.rows(buf, fields, True)
        assert any(c == R.CELL_ONE for r in rows for c in r) and any(c == R.CELL_DOT for r in rows for c in r)
        assert stdin == any(c[1] == 0 for r in rows for c in r)  # an empty cell exists in stdin mode only
