"""The plain-Python restatement of VCFX_region_subsampler (tests/_region_subsampler_ref.py) against
the compiled reference's recorded bytes (tests/golden/region_subsampler_cases.json.gz, written by
tests/golden/make_region_subsampler_golden.py): stdout, stderr and exit code of every case, byte for
byte.  The restatement is the checker of generated inputs in tests/test_gpu_rs.py; every such input
is shown here to have a non-trivial answer."""
import pytest

from tests import _region_subsampler_ref as R

CASES = R.load_cases()
BY = {c["name"]: c for c in CASES}


def test_case_list_covers_the_forms():
    assert len(BY) == len(CASES) >= 100
    for pair in ("bed_forms.vcf+bed_forms.bed", "bed_forms.vcf+bed_forms_crlf.bed", "bed_forms.vcf+empty.bed",
                 "bed_forms.vcf+comment_only.bed", "bed_forms.vcf+bed_forms_no_final_newline.bed", "pos_forms.vcf+pos.bed",
                 "boundary.vcf+boundary.bed", "line_mix.vcf+mix.bed", "line_mix_crlf.vcf+mix.bed",
                 "no_final_newline_in.vcf+mix.bed", "header_only.vcf+mix.bed", "only_newlines.vcf+mix.bed", "empty.vcf+mix.bed"):
        for form in ("file", "stdin", "quiet_file", "quiet_stdin"):
            assert "%s__%s" % (pair, form) in BY
    for name in ("region_bed_equals", "attached_value", "prefix_of_long", "no_bed", "b_without_value", "missing_bed",
                 "directory_as_bed", "missing_input", "positional_is_ignored", "help", "help_short", "help_in_group",
                 "version", "bad_long", "bad_short"):
        assert name in BY


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_reference(case):
    out, err, rc = R.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_the_modes_differ_where_the_reference_differs():
    """the goldens pin the differences: other bytes on the POS fixture, -q silent in file mode only"""
    pair = "pos_forms.vcf+pos.bed"
    assert BY[pair + "__file"]["stdout"] != BY[pair + "__stdin"]["stdout"]
    # (file mode never rejects a POS; the one empty POS field is a missing column)
    assert BY[pair + "__file"]["stderr"] == R.WARN_SHORT_FILE and BY[pair + "__stdin"]["stderr"].count(R.WARN_POS) >= 8
    mix = "line_mix.vcf+mix.bed"
    for w in (R.WARN_EARLY, R.WARN_SHORT_FILE):
        assert w in BY[mix + "__file"]["stderr"]
    for w in (R.WARN_EARLY, R.WARN_SHORT_STDIN, R.WARN_POS):
        assert w in BY[mix + "__stdin"]["stderr"]
    assert BY[mix + "__quiet_file"]["stderr"] == b""
    assert BY[mix + "__quiet_stdin"]["stderr"] == BY[mix + "__stdin"]["stderr"]
    assert BY[mix + "__quiet_file"]["stdout"] == BY[mix + "__file"]["stdout"]
    assert BY["directory_as_bed"]["rc"] == 0 and BY["directory_as_bed"]["stdout"].count(b"\n") >= 5
    assert BY["no_bed"]["rc"] == 1 and BY["no_bed"]["stdout"] == R.HELP and BY["no_bed"]["stderr"] == R.NO_BED


def test_pos_forms():
    want = {b"55": (55, 55), b" 7": (7, 7), b"+55": (55, 55), b"-5": (5, -5), b"1e1": (11, 1), b"abc": (0, None),
            b"": (0, None), b"+": (0, None), b"4294967301": (5, None), b"2147483648": (-(1 << 31), None),
            b"2147483647": ((1 << 31) - 1, (1 << 31) - 1), b"-2147483648": (-(1 << 31), -(1 << 31)), b"5 5": (55, 5)}
    for f, (vf, vs) in want.items():
        assert R.pos_file(f) == vf, f
        assert R.pos_stdin(f) == vs, f


def test_bed_forms():
    names, ivs, warn = R.load_bed(b"chr1 0 100\n chr2\t-5\t10\nchr6\t007\t+9\r\ntrack x\nchr4 99999999999 5\nchr5 5.5 9\n"
                                  b"chr5 0x10 20\n#c 1 2\n\nchr5 70 70\n")
    assert names == [b"chr1", b"chr2", b"chr6"]
    assert ivs == [(0, 1, 100), (1, 1, 10), (2, 8, 9)]
    assert warn.count(b"Warning: skipping invalid bed line ") == 4 and b"line 4: track x\n" in warn
    assert R.merged([(0, 21, 30), (0, 1, 20), (0, 32, 40), (1, 5, 9), (0, 3, 4)]) == [(0, 1, 30), (0, 32, 40), (1, 5, 9)]


@pytest.mark.parametrize("name", sorted(R.GENERATED))
def test_generated_inputs_are_not_trivial(name):
    """each generated input of the GPU tests, in both modes: between 10 % and 90 % of its data lines are
    kept, a line sits at each of the four boundary positions of a BED row, and a CHROM is absent from
    the BED"""
    buf, bed = R.generated(name)
    for stdin in (False, True):
        data, kept, at, absent = R.nontrivial(buf, bed, stdin)
        assert data >= 0.7 * R.GENERATED[name][1]["n"]
        assert 0.1 * data <= kept <= 0.9 * data, (data, kept)
        assert min(at) >= 1, at
        assert absent >= 1
