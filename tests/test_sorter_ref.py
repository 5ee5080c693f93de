"""The plain-Python restatement of VCFX_sorter (tests/_sorter_ref.py) against the compiled
reference's recorded bytes (tests/golden/sorter_cases.json.gz, written by
tests/golden/make_sorter_golden.py): stdout, stderr and exit code of every case.  A case is compared
byte for byte unless it sorts a ties_* fixture (17 or more kept lines with equal keys, where the
reference's unstable sort decides the order inside a run): those are held to same_up_to_ties.  The
restatement is the checker of generated inputs in tests/test_gpu_srt.py."""
import os

import pytest

from tests import _sorter_ref as R

CASES = R.load_cases()
BY = {c["name"]: c for c in CASES}
FORMS = ("file", "stdin", "natural_file", "natural_stdin")


def fixture(name):
    with open(os.path.join(R.GOLDEN, "sorter", name), "rb") as f:
        return f.read()


def test_case_list_covers_the_forms():
    assert len(BY) == len(CASES) >= 100
    for fx in ("rules.vcf", "rules_crlf.vcf", "no_final_newline_kept.vcf", "pos_forms.vcf", "empty_chrom.vcf", "natural.vcf",
               "chrom_lengths.vcf", "ties_a.vcf", "ties_b.vcf", "header_only.vcf", "empty.vcf"):
        for form in FORMS:
            assert "%s__%s" % (fx, form) in BY
    for name in ("missing_file", "second_file_missing", "two_files", "help", "help_short", "bad_long", "bad_short",
                 "version", "generated.vcf__m0_stdin", "generated.vcf__m1_file", "generated.vcf__t_stdin"):
        assert name in BY


def test_only_the_ties_fixtures_use_the_weaker_rule():
    """the partition the generator asserted, recomputed: a case marked `ties` sorts a ties_* fixture
    with at least 17 kept lines and runs of equal keys; every other sorted input has no equal keys
    among its kept lines or keeps at most 16"""
    weak = [c for c in CASES if c["ties"]]
    assert len(weak) >= 8
    for c in CASES:
        stdin, natural = R.case_mode(c)
        names = [c["stdin"]] if stdin else R.getopt_long(c["argv"])[1]
        for name in names:
            base = os.path.basename(name or "")
            if not os.path.isfile(os.path.join(R.GOLDEN, "sorter", base)):
                continue
            kept, tied = R.tie_profile(fixture(base), stdin, natural)
            if c["ties"]:
                assert base.startswith("ties_") and kept >= 17 and tied >= 10, c["name"]
            elif c["rc"] == 0 and c["stdout"] != R.HELP:
                assert not base.startswith("ties_") and (tied == 0 or kept <= 16), c["name"]
    for fx in ("ties_a.vcf", "ties_b.vcf"):
        for form in FORMS:
            assert BY["%s__%s" % (fx, form)]["ties"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_reference(case):
    out, err, rc = R.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert err == case["stderr"]
    if case["ties"]:
        assert R.same_up_to_ties(out, case["stdout"], *R.case_mode(case))
    else:
        assert out == case["stdout"]


def test_the_reference_is_not_stable_on_a_ties_fixture():
    """why the weaker rule exists: on some ties_* case the reference's bytes differ from the stable
    order (were that never so, the rule would be idle)"""
    differ = [c["name"] for c in CASES if c["ties"] and R.run(c["argv"], R.case_stdin(c), cwd=R.GOLDEN)[0] != c["stdout"]]
    assert differ


def test_same_up_to_ties_is_a_real_check():
    a = b"#h\n1\t5\tx\n1\t5\ty\n2\t1\tz\n"
    assert R.same_up_to_ties(a, b"#h\n1\t5\ty\n1\t5\tx\n2\t1\tz\n", False, False)
    assert not R.same_up_to_ties(a, b"#h\n1\t5\tx\n2\t1\tz\n1\t5\ty\n", False, False)   # another key sequence
    assert not R.same_up_to_ties(a, b"#h\n1\t5\tx\n1\t5\tx\n2\t1\tz\n", False, False)   # another multiset
    assert not R.same_up_to_ties(a, b"#g\n1\t5\tx\n1\t5\ty\n2\t1\tz\n", False, False)   # another header block
    assert not R.same_up_to_ties(a, a[:-1 - 5], False, False)                             # a line missing


def test_the_modes_and_orders_differ_where_the_reference_differs():
    for fx in ("rules.vcf", "pos_forms.vcf", "empty_chrom.vcf"):
        assert BY[fx + "__file"]["stdout"] != BY[fx + "__stdin"]["stdout"], fx
    for fx in ("natural.vcf", "generated.vcf", "empty_chrom.vcf"):
        assert BY[fx + "__file"]["stdout"] != BY[fx + "__natural_file"]["stdout"], fx
    assert BY["rules.vcf__file"]["stderr"].count(R.WARN_PRE) == 2
    assert BY["rules.vcf__stdin"]["stderr"].count(R.WARN_PRE) == 0
    assert BY["no_chrom_line.vcf__file"]["stdout"] == b"##only meta\n"
    # -m and -t change nothing where no keys are equal
    for fx in ("generated.vcf", "natural.vcf"):
        assert BY[fx + "__m0_stdin"]["stdout"] == BY[fx + "__stdin"]["stdout"] == BY[fx + "__m1_stdin"]["stdout"]
        assert BY[fx + "__m1_file"]["stdout"] == BY[fx + "__file"]["stdout"]
        assert BY[fx + "__t_stdin"]["stdout"] == BY[fx + "__stdin"]["stdout"]


def test_empty_chrom_sorts_first_in_file_mode_and_last_on_stdin():
    for form, first in (("file", True), ("stdin", False)):
        data = R.split_output(BY["empty_chrom.vcf__" + form]["stdout"], form == "stdin", False)[1]
        empties = [i for i, (_, line) in enumerate(data) if line[:1] == b"\t"]
        assert len(empties) == 3
        assert empties == ([0, 1, 2] if first else list(range(len(data) - 3, len(data))))
        assert [data[i][0][-1] for i in empties] == [3, 5, 7]


def test_pos_forms():
    # (file mode: the digit run in a wrapping int, kept unless 0; stdin mode: std::stoi)
    want = {b"55": (55, 55), b" 56": (None, 56), b"+58": (None, 58), b"-59": (None, -59), b"60abc": (60, 60),
            b"abc": (None, None), b"": (None, None), b"+-63": (None, None), b"0": (None, 0), b"-0": (None, 0), b"007": (7, 7),
            b"0x10": (None, 0), b"4294967351": (55, None), b"4294967301": (5, None), b"2147483647": ((1 << 31) - 1,) * 2,
            b"2147483648": (-(1 << 31), None), b"4294967295": (-1, None), b"4294967296": (None, None), b"-2147483648": (None, -(1 << 31)), b"-2147483649": (None, None),
            b"\x0b\x0c\r 57": (None, 57), b"6 2": (6, 6), b"1.5": (1, 1)}
    for f, (vf, vs) in want.items():
        assert R.pos_file(b"c\t" + f + b"\tid", 1) == vf, f
        assert R.stoi(f) == vs, f
    assert R.data_key(b"1\t7", False, False) == (0, b"1", 7) and R.data_key(b"1\t7", True, False) is None
    assert R.data_key(b"no tab", False, False) is None


def test_chrom_to_id():
    """the id scheme, and the ids the recorded natural orders imply: along every recorded -n output
    (id, POS) never decreases, and it increases wherever the restatement says the keys differ"""
    ident = R.chrom_to_id
    assert ident(b"") == ident(b"chr") == ident(b"CHR") == ident(b"cHR") == 999999
    assert ident(b"1") == 100000 and ident(b"22") == 2200000 and ident(b"chr1") == 5130000
    assert ident(b"CHR1") == 5110000 and ident(b"Chr1") == 5120000 and ident(b"cHr1") == ident(b"chR1") == ident(b"chr1")
    assert ident(b"chr01") == ident(b"chr1") and ident(b"001") == ident(b"1")
    # M, MT, X and Y carry the hash of their own letters as a suffix hash: M and MT are two ids
    assert ident(b"M") == 2300000 + 78 and ident(b"MT") == 2300000 + ((77 * 31 + 84) & 0x7FFF) + 1
    assert ident(b"X") == 2400000 + 89 and ident(b"Y") == 2500000 + 90 and ident(b"x") == 2400000 + 121
    assert ident(b"M") < ident(b"MT") < ident(b"X") < ident(b"Y") < ident(b"23") and ident(b"23") >= 6000000
    assert ident(b"1") < ident(b"1_abcdefgh1") == ident(b"1_abcdefgh2") < ident(b"2")
    assert ident(b"scaffold_0123456789") == ident(b"scaffold_0123456788x") != ident(b"scaffold_012345")
    assert ident(b"22") < ident(b"chr1") and ident(b"chr22") < ident(b"chr23")
    n = 0
    for c in CASES:
        stdin, natural = R.case_mode(c)
        if not natural or c["rc"] or c["stdout"] == R.HELP or len(R.getopt_long(c["argv"])[1]) > 1:
            continue  # (two files: two outputs one after the other)
        keys = [k for k, _ in R.split_output(c["stdout"], stdin, True)[1]]
        assert None not in keys
        assert all(a <= b for a, b in zip(keys, keys[1:])), c["name"]
        n += len(keys)
    assert n > 1000


@pytest.mark.parametrize("name", sorted(R.GENERATED))
def test_generated_inputs(name):
    """each generated input of the GPU tests: its kept-line count, no equal keys unless it is a
    ties input, and an order that is not the input's"""
    buf = R.generated(name)
    g = R.GENERATED[name]
    for stdin in (False, True):
        for natural in (False, True):
            kept, tied = R.tie_profile(buf, stdin, natural)
            assert kept == g["n"]
            assert (tied > kept // 2) if g.get("ties") else tied == 0
            o = R.order(buf, stdin, natural)
            assert o != sorted(o) or kept < 3
