"""The plain-Python restatement of VCFX_duplicate_remover (tests/_duplicate_remover_ref.py) against
the compiled reference's recorded bytes (tests/golden/duplicate_remover_cases.json.gz, written by
tests/golden/make_duplicate_remover_golden.py): stdout, stderr and exit code of every case, byte
for byte.  The restatement is the checker of generated inputs in tests/test_gpu_dd.py; every such
input is shown here to have a non-trivial answer."""
import pytest

from tests import _duplicate_remover_ref as R

CASES = R.load_cases()
BY = {c["name"]: c for c in CASES}


def test_case_list_covers_the_forms():
    assert len(BY) == len(CASES) >= 100
    for fx in ("pos_forms.vcf", "pos_scan.vcf", "alt_forms.vcf", "line_mix.vcf", "line_mix_crlf.vcf",
               "no_final_newline_dup.vcf", "header_only.vcf", "empty.vcf"):
        for form in ("file", "pos", "stdin", "quiet_file", "quiet_stdin"):
            assert "%s__%s" % (fx, form) in BY
    for name in ("missing_file", "help", "help_short", "bad_long", "bad_short", "version"):
        assert name in BY


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_reference(case):
    out, err, rc = R.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_the_modes_differ_where_the_reference_differs():
    """the goldens pin the differences: the two modes give other bytes on the POS and ALT fixtures"""
    for fx in ("pos_forms.vcf", "pos_scan.vcf", "alt_forms.vcf"):
        assert BY[fx + "__file"]["stdout"] != BY[fx + "__stdin"]["stdout"], fx
        assert BY[fx + "__file"]["stdout"] == BY[fx + "__pos"]["stdout"], fx
    assert BY["line_mix.vcf__file"]["stderr"].count(R.WARN) == 5  # three tabs, two, none, three bare tabs, a blank
    assert BY["line_mix.vcf__quiet_file"]["stderr"] == b""


def test_pos_forms():
    want = {b"55": (55, 55), b" 55": (55, 55), b"+55": (55, 55), b"-55": (-55, -55), b"55abc": (55, 55), b"abc": (0, 0),
            b"": (0, 0), b"+-55": (0, 0), b"4294967351": (55, 0), b"2147483648": (-(1 << 31), 0),
            b"-2147483649": ((1 << 31) - 1, 0), b"99999999999999999999": (-1, 0), b"-99999999999999999999": (0, 0),
            b"9223372036854775808": (-1, 0), b"-9223372036854775808": (0, 0), b"18446744073709551671": (-1, 0)}
    for f, (vf, vs) in want.items():
        assert R.pos_file(f + b"\tid", 0) == vf, f
        assert R.pos_stdin(f) == vs, f
    assert R.pos_file(b"\t55\tA", 0) == 55 and R.pos_file(b"\t\t\t\n77\t1", 0) == 77 and R.pos_stdin(b"") == 0


def test_alt_keys():
    def key(alt, stdin):
        ln = b"1\t5\t.\tA\t" + alt
        return R.line_key(ln, 0, len(ln), stdin)

    assert key(b"G,,C", True) == key(b"G,C,", True) != key(b"C,G", True)
    assert key(b"G,,C", False) == key(b"G,C,", False) == key(b"C,G", False)
    for stdin in (False, True):
        assert key(b"A,A", stdin) != key(b"A", stdin)
        assert key(b"A,C,T", stdin) == key(b"T,A,C", stdin)
        assert key(b"A,A,C", stdin) != key(b"A,C,C", stdin)
        assert key(b"C\tq", stdin) == key(b"C", stdin)
    assert R.line_key(b"1\t5\t.\tA", 0, 7, False) is None


@pytest.mark.parametrize("name", sorted(R.GENERATED))
def test_generated_inputs_are_not_trivial(name):
    """each generated input of the GPU tests, in both modes: between 10 % and 90 % of its data
    lines are dropped, one of them stands in another ALT order than its first occurrence, and one
    differs from it only in ID or in the columns after ALT"""
    buf = R.generated(name)
    for stdin in (False, True):
        data, dropped, alt_order, same_but_id = R.nontrivial(buf, stdin)
        assert data == R.GENERATED[name]["n"]
        assert 0.1 * data <= dropped <= 0.9 * data, (data, dropped)
        assert alt_order >= 1 and same_but_id >= 1
