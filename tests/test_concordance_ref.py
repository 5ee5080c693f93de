"""The plain-Python restatement of VCFX_cross_sample_concordance (tests/_concordance_ref.py)
against the compiled reference's recorded bytes (tests/golden/concordance_cases.json.gz, written
by tests/golden/make_concordance_golden.py): stdout, stderr and exit code of every case, byte for
byte.  The restatement is the checker of generated inputs in tests/test_gpu_cc.py."""
import pytest

from tests import _concordance_ref as R

CASES = R.load_cases()


def test_case_list_covers_the_modes():
    names = {c["name"] for c in CASES}
    assert len(names) == len(CASES) >= 100
    for t in ("1", "2", "3", "64"):
        assert "hand.vcf__t%s__file" % t in names and "hand.vcf__t%s__pos" % t in names
    assert "hand.vcf__stdin" in names
    for c in CASES:  # the default worker count depends on the host: never recorded
        a = c["argv"][1:]
        if c["stdin"] is None and c["stdout"]:
            assert any(x.startswith("-t") or x.startswith("--thr") for x in a) or "-h" in a or "--help" in a \
                or "-v" in a or "--version" in a or "-qh" in a, c["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_reference(case):
    out, err, rc = R.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_keys():
    want = {b"0/1": (0, 1), b"1|0": (0, 1), b"/0": (0, 0), b"0/x": (0, 0), b"0/": None, b"1": None, b"0/1/1": (0, 1),
            b".": None, b"": None, b"./1": None, b"0/.": None, b"2/0": None, b"0/1:5": (0, 1), b":0/1": None,
            b"01/1": (1, 1), b" 0/1": None, b"|": None, b"/": None}
    for f, k in want.items():
        assert R.gt_key(f, 1) == k, f
    assert R.gt_key(b"127/3", 200) == (3, 127) and R.gt_key(b"128/3", 200) is None
    assert R.gt_key(b"10/2", 10) == (2, 10) and R.gt_key(b"10/2", 9) is None
    assert [R.num_alt(a) for a in (b"", b".", b".,T", b"T", b"T,G", b"T,,")] == [0, 0, 0, 1, 2, 3]


@pytest.mark.parametrize("n", [1, 2, 7, 8, 63, 64, 65, 1000])
def test_order_mapping_is_the_inverse_of_the_worker_blocks(n):
    for t in (1, 2, 3, 7, 9, 64, n, n + 1):
        order = R.output_order(n, t)
        assert sorted(order) == list(range(n))
        assert [R.rank_of(i, n, t) for i in order] == list(range(n))


def test_two_chrom_lines_double_the_samples_not_the_keys():
    by = {c["name"]: c for c in CASES}
    one = by["hand.vcf__t1__file"]["stdout"].split(b"\n")
    two = by["two_chrom.vcf__t1__file"]["stdout"].split(b"\n")
    assert len(one) == len(two)
    doubled = 0
    for a, b in zip(one[1:-1], two[1:-1]):
        fa, fb = a.split(b"\t"), b.split(b"\t")
        assert int(fb[5]) == 2 * int(fa[5]) and fb[6] == fa[6]
        doubled += int(fa[5]) > 0
    assert doubled
