"""The plain-Python restatement of VCFX_diff_tool (tests/_diff_tool_ref.py) against every recorded case
of the compiled reference (tests/golden/diff_tool_cases.json.gz), on the CPU: byte for byte where the
case is `ordered` (every -s case, every case whose sides hold at most one key), else by
same_sections (the reference's default-mode order is its C++ library's); the recorded set itself
(how many cases are ordered, what the fixtures cover); and the helper on outputs it must refuse."""
import os

import pytest

from tests import _diff_tool_ref as R

CASES = R.load_cases()
BY = {c["name"]: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_recorded_output(case, monkeypatch):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    out, err, rc = R.run(case["argv"], cwd=R.GOLDEN)
    assert (err, rc) == (case["stderr"], case["rc"])
    if case["ordered"]:
        assert out == case["stdout"]
    else:
        assert R.same_sections(out, case["stdout"])


def test_the_helper_is_never_the_only_check():
    ordered = [c for c in CASES if c["ordered"]]
    assert 3 * len(ordered) >= len(CASES) and len(CASES) - len(ordered) >= 15
    for c in CASES:
        sorted_mode = any(k == "s" for k, _, _ in R.getopt_long(c["argv"])[0])
        sec = R.sections(c["stdout"])
        assert c["ordered"] == (sorted_mode or sec is None or max(len(sec[1]), len(sec[3])) <= 1), c["name"]


def test_same_sections_refuses_what_differs():
    want = BY["rules__default"]["stdout"]
    sec = R.sections(want)
    assert len(sec[1]) >= 3 and len(sec[3]) >= 2
    assert R.same_sections(want, want)
    lines = want.split(b"\n")
    swapped = b"\n".join([lines[0], lines[2], lines[1]] + lines[3:])
    assert swapped != want and R.same_sections(swapped, want)  # another order inside a side
    assert not R.same_sections(want.replace(b"rules_a", b"rules_x"), want)  # another header line
    assert not R.same_sections(b"\n".join(lines[:1] + lines[2:]), want)  # a line missing
    assert not R.same_sections(b"\n".join(lines[:2] + lines[1:]), want)  # a line twice
    moved = b"\n".join(lines[:1] + lines[2:-1] + [lines[1], b""])
    assert not R.same_sections(moved, want)  # a line on the other side
    assert not R.same_sections(want[:-1], want) and not R.same_sections(b"", want)


def test_recorded_facts():
    """what the issue states about the reference, read from the recorded bytes"""
    # the 1:5::A:T collision cancels; 007 and 7 differ as text and are equal as integers
    # (as whole strings; the sorted mode compares the fields and prints the one text on both sides)
    assert BY["collide__default"]["stdout"] == R.output("diff_tool/collide_a.vcf", "diff_tool/collide_b.vcf", [], [])
    for mode in ("s", "sn"):
        assert BY["collide__" + mode]["stdout"] == R.output("diff_tool/collide_a.vcf", "diff_tool/collide_b.vcf", [b"1:5::A:T"], [b"1:5::A:T"])
    assert BY["pos007__default"]["stdout"] == R.output("diff_tool/pos007_a.vcf", "diff_tool/pos007_b.vcf", [b"1:007:A:T"], [b"1:7:A:T"])
    assert BY["pos007__s"]["stdout"] == R.output("diff_tool/pos007_a.vcf", "diff_tool/pos007_b.vcf", [], [])
    # lines that compare equal print different keys
    assert R.sections(BY["equal_not_same__s"]["stdout"])[1] == [b"1:7:A:T", b"1:07:A:T", b"1:09:A:T"]
    assert R.sections(BY["equal_not_same__s"]["stdout"])[3] == [b"1:0008:A:T"]
    assert R.sections(BY["equal_not_same_natural__sn"]["stdout"])[1] == [b"chr1:5:A:T", b"01:5:A:T"]
    # the messages and the return codes
    assert BY["empty_both__default"]["stdout"] == b"Variants unique to diff_tool/empty.vcf:\n\nVariants unique to diff_tool/empty.vcf:\n"
    assert (BY["no_arguments"]["stdout"], BY["no_arguments"]["rc"]) == (R.HELP, 1)
    assert (BY["bad_long"]["stdout"], BY["bad_long"]["rc"]) == (R.HELP, 0) and BY["bad_long"]["stderr"]
    for name, path in (("missing_first", "does_not_exist.vcf"), ("missing_both", "does_not_exist_1.vcf"), ("directory_first", "")):
        c = BY[name]
        assert (c["stdout"], c["rc"]) == (b"", 1)
        assert c["stderr"] == b"Error: Unable to open file diff_tool" + (b"/" + path.encode() if path else b"") + b"\n"
    assert R.same_sections(BY["quiet_default"]["stdout"], BY["rules__default"]["stdout"])  # (-q changes nothing)
    # every status and both device paths of the sorted mode occur in the fixtures
    seen, paths = set(), set()
    for c in CASES:
        opts, _ = R.getopt_long(c["argv"])
        got = {k: v for k, v, _ in opts}
        if c["rc"] or c["env"] or not got.get("a") or not got.get("b") or "h" in got or "?" in got:
            continue
        files = [R.read_input(got[k], R.GOLDEN) for k in "ab"]
        if None in files:
            continue  # ("-a -h": the help)
        st, _, _, path, _, _ = R.diff(files[0], files[1], "s" in got, "n" in got)
        seen |= set(st)
        paths.add(path)
    assert seen == {R.EMPTY, R.COMMON, R.UNIQUE, R.SKIPPED, R.HEADER, R.REPEAT}
    assert paths == {R.PATH_HASH, R.PATH_BOUNDS, R.PATH_WALK}
    assert os.path.getsize(os.path.join(R.GOLDEN, "diff_tool_cases.json.gz")) < (1 << 20)


def test_key_and_order_rules():
    assert R.key(b"1", b"007", b"A", b"T,,C,AT,A") == b"1:007:A:,A,AT,C,T"
    assert R.key(b"", b"", b"", b"") == b":::" and R.key(b"c", b"1", b"r", b"\xff,\x80,a") == b"c:1:r:a,\x80,\xff"
    names = [b"chr1", b"Chr1", b"CHR1", b"1", b"01"]
    assert len({R.sort_key((n, b"5", b"A", b"T"), True)[0] for n in names}) == 1
    assert R.sort_key((b"cHr1", b"5", b"A", b"T"), True)[0] == (1, 0, b"cHr1")  # (not a prefix that is dropped)
    order = sorted([b"X", b"10", b"chr2", b"1a", b"1", b"chr", b"", b"MT"], key=lambda n: R.sort_key((n, b"", b"", b""), True))
    assert order == [b"1", b"1a", b"chr2", b"10", b"chr", b"", b"MT", b"X"]  # ("chr" is "" without its prefix: a tie)
    assert R.parse(b"1\t\t.\tA\tT")[1] == (b"1", b"", b"A", b"T") and R.parse(b"1\t5\t.\tA")[0] == R.SKIPPED
    assert R.parse(b"1\t5\t.\tA\tT\r")[1] == (b"1", b"5", b"A", b"T") and R.parse(b"\r")[0] == R.SKIPPED
    assert R.join(b"a", b"b") == (b"a\nb", 2) and R.join(b"a\n", b"b") == (b"a\nb", 2) and R.join(b"", b"b") == (b"b", 0)
