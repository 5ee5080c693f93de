"""The plain-Python restatement of VCFX_merger (tests/_merger_ref.py) against the compiled reference's
recorded bytes (tests/golden/merger_cases.json.gz, written by tests/golden/make_merger_golden.py):
every ordered case byte for byte; the ties_* cases (equal keys, which the reference leaves to
std::sort and to its heap) by the same header, the same key sequence and the same lines in every run
of equal keys.  CPU only."""
import os

import pytest

from tests import _merger_ref as R

CASES = R.load_cases()
BY = {c["name"]: c for c in CASES}


def run_case(c):
    old = {k: os.environ.get(k) for k in c["env"]}
    os.environ.update(c["env"])
    try:
        return R.run(c["argv"], cwd=R.GOLDEN)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def is_natural(c):
    return any(k == "n" for k, _, _ in R.getopt_long(c["argv"])[0])


def test_the_recording_is_what_the_generator_promises():
    assert len(CASES) >= 100 and len(BY) == len(CASES)
    tied = [c for c in CASES if not c["ordered"]]
    assert tied and all(c["name"].startswith("ties_") for c in tied)
    assert all(c["rc"] == 0 for c in CASES)  # the exit code is always 0
    reading = [c for c in CASES if c["stdout"] != R.HELP and c["stdout"] != R.VERSION]
    assert 5 * len(tied) <= len(reading)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_restatement_matches_the_reference(name):
    c = BY[name]
    out, err, rc = run_case(c)
    assert (err, rc) == (c["stderr"], c["rc"])
    if c["ordered"]:
        assert out == c["stdout"]
    else:
        assert R.same_under_ties(out, c["stdout"], is_natural(c))


def test_recorded_rules():
    """the findings the restatement and the device are built on, as the reference printed them"""
    hdr = R.HDR.split(b"\n")[1] + b"\n"
    # default mode: a '#' line only after the data is the header; -s: it is no candidate
    assert BY["hdr_after_data__default"]["stdout"].startswith(b"#only after the data\n3\t10\t")
    assert BY["hdr_after_data__s"]["stdout"].startswith(b"3\t30\t")  # (and an unsorted file comes out as it is)
    # the header of the third file, all of it in the default mode, its leading lines under -s
    assert BY["hdr_third__default"]["stdout"].startswith(b"##third\n" + hdr + b"#late\n4\t40\t")
    assert BY["hdr_third__s"]["stdout"].startswith(b"##third\n" + hdr + b"4\t40\t")
    # a malformed line ends the candidates under -s, silently; the default mode warns
    assert BY["bad_before_header__s"]["stdout"].startswith(b"##another header\n")
    assert BY["bad_before_header__s"]["stderr"] == b""
    assert BY["bad_before_header__default"]["stdout"].startswith(b"##after a malformed line\n")
    assert BY["bad_before_header__default"]["stderr"] == b"Warning: skipping malformed line in merger/bad_before_header.vcf\n"
    # stderr in list order; a directory yields nothing; an empty name fails to open
    assert BY["missing_middle__default"]["stderr"] == b"Failed to open file: merger/does_not_exist.vcf\n"
    assert BY["directory_only__default"]["stderr"] == b"" and BY["directory_only__default"]["stdout"] == b""
    assert BY["empty_names"]["stderr"] == b"Failed to open file: \n"
    assert BY["no_arguments"]["stdout"] == R.HELP and BY["bad_short"]["stdout"] == R.HELP
    # the natural order's recorded sequence
    names = []
    for l in BY["zoo_nat__n"]["stdout"].split(b"\n"):
        if l and l[:1] != b"#" and l.split(b"\t")[0] not in names:
            names.append(l.split(b"\t")[0])
    want = [b"1", b"2", b"2a", b"2b", b"10", b"X", b"Chr2", b"chr2", b"chr10", b"chrX"]
    assert [n for n in names if n in want] == want
    # the long extremes are kept, the first value past each is malformed
    out = BY["pos_forms__default"]["stdout"]
    assert b"p\t-9223372036854775808\t" in out and b"p\t9223372036854775807\t" in out
    assert b"p\t9223372036854775808\t" not in out and b"p\t-9223372036854775809\t" not in out
    assert out.split(b"\n")[1].startswith(b"p\t-9223372036854775808\t")


def test_stol():
    for f, v in ((b" 7", 7), (b"\v\f\r 8", 8), (b"+3", 3), (b"-5", -5), (b"5abc", 5), (b"0x10", 0), (b"0" * 40 + b"9", 9),
                 (b"", None), (b"-", None), (b"- 3", None), (b"abc", None), (b"9223372036854775808", None),
                 (b"9223372036854775807", 2 ** 63 - 1), (b"-9223372036854775808", -2 ** 63), (b"-9223372036854775809", None)):
        assert R.stol(f) == v, f


def test_tie_rule_and_detector():
    a = R.HDR + b"1\t5\t.\ta0\n1\t5\t.\ta1\n1\t9\t.\ta2\n"
    b = b"1\t5\t.\tb0\n1\t7\t.\tb1\n"
    for s in (False, True):
        m = R.merge([a, b], s)
        assert m.ties and m.path == R.PATH_SORT
        assert [l.split(b"\t")[3] for l in m.text.split(b"\n")[2:-1]] == [b"a0", b"a1", b"b0", b"b1", b"a2"]
    m = R.merge([b"1\t9\t.\n1\t5\t.\n", b"1\t7\t.\n"], True)  # an unsorted file: the heap process, no tie met
    assert m.path == R.PATH_WALK and not m.ties and [k[1] for k in m.keys] == [7, 9, 5]
    assert R.merge([b"1\t9\t.\n1\t5\t.\n", b"1\t7\t.\n"], False).keys == [(b"1", 5), (b"1", 7), (b"1", 9)]
    assert R.sort_key(b"1", 5, True) == R.sort_key(b"01", 5, True) and R.sort_key(b"chr1", 5, True) != R.sort_key(b"Chr1", 5, True)
