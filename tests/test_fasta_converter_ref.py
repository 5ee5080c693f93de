"""The plain-Python restatement of VCFX_fasta_converter (tests/_fasta_converter_ref.py) against
every case recorded from the compiled reference: stdout, stderr and exit code, byte for byte."""
import os

from tests import _fasta_converter_ref as R

CASES = R.load_cases()


def test_cases_cover_the_forms():
    names = {c["name"] for c in CASES}
    assert len(CASES) > 150
    for fx in os.listdir(os.path.join(R.GOLDEN, "fasta_converter")):
        for form in ("file", "pos", "stdin", "quiet_file", "quiet_stdin"):
            assert "%s__%s" % (fx, form) in names, (fx, form)
    out = {c["name"]: c["stdout"] for c in CASES}
    assert b"\0" in out["line_forms.vcf__file"] and b"\0" not in out["line_forms.vcf__stdin"]
    assert out["gt_forms_crlf.vcf__file"].count(b"\r\n") == out["gt_forms_crlf.vcf__stdin"].count(b"\r\n") == 1
    assert [len(x) for x in out["cols_61.vcf__file"].split(b"\n")[:3]] == [3, 60, 1]


def test_restatement_equals_every_case():
    bad = []
    for c in CASES:
        got = R.run(c["argv"], R.case_stdin(c), cwd=R.GOLDEN)
        if got != (c["stdout"], c["stderr"], c["rc"]):
            bad.append(c["name"])
    assert not bad, bad


def test_stdin_data_before_chrom_prints_nothing():
    c = {c["name"]: c for c in CASES}["data_before_chrom.vcf__stdin"]
    assert (c["stdout"], c["stderr"], c["rc"]) == (b"", R.NO_CHROM, 0)
    f = {c["name"]: c for c in CASES}["data_before_chrom.vcf__file"]
    assert f["stdout"].startswith(b">S1\n") and f["rc"] == 0


def test_two_headers_rows():
    by = {c["name"]: c for c in CASES}
    assert by["two_headers.vcf__stdin"]["stdout"] == b">S1\nMTAA\n>S2\nRR\n>S3\nGG\n"
    rows = by["two_headers.vcf__file"]["stdout"].split(b"\n")
    assert len(rows[1]) == len(rows[3]) == len(rows[5]) == 5 and rows[3][:2] == b"\0\0"


def test_device_view_matches_the_conversion():
    """the per-line view the GPU tests hold the raw ABI to gives the same FASTA as the restatement"""
    for fx in sorted(os.listdir(os.path.join(R.GOLDEN, "fasta_converter"))):
        buf = open(os.path.join(R.GOLDEN, "fasta_converter", fx), "rb").read()
        for stdin in (False, True):
            start, names, seen, per = R.device_view(buf, stdin)
            if start is None:
                assert (R.convert_stdin(buf)[0] if stdin else R.convert_file(buf)) == b"", fx
                continue
            lines = R.raw_lines(buf[start:])
            assert len(lines) == len(per)
            if stdin and not seen:
                assert R.convert_stdin(buf) == (b"", R.NO_CHROM), fx


def test_sequences_give_the_conversion():
    for fx in sorted(os.listdir(os.path.join(R.GOLDEN, "fasta_converter"))):
        buf = open(os.path.join(R.GOLDEN, "fasta_converter", fx), "rb").read()
        for stdin in (False, True):
            want = R.convert_stdin(buf)[0] if stdin else R.convert_file(buf)
            q = R.sequences(buf, stdin)
            got = b"" if q is None else b"".join(b">" + nm + b"\n" + R.wrap(sq) for nm, sq in zip(q[0], q[1]))
            assert got == want, (fx, stdin)
