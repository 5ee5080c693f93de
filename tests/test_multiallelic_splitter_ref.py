"""The plain-Python restatement of VCFX_multiallelic_splitter (tests/_multiallelic_splitter_ref.py)
against the compiled reference's recorded bytes (tests/golden/multiallelic_splitter_cases.json.gz,
written by tests/golden/make_multiallelic_splitter_golden.py): stdout, stderr and exit code of every
case, byte for byte.  The restatement is the checker of generated inputs in tests/test_gpu_ms.py."""
import pytest

from tests import _multiallelic_splitter_ref as R

CASES = R.load_cases()
BY = {c["name"]: c for c in CASES}
TAB = b"\t"


def test_case_list_covers_the_forms():
    assert len(BY) == len(CASES) >= 150
    for fx in ("probe.vcf", "probe_crlf.vcf", "gt_forms.vcf", "list_forms.vcf", "sample_forms.vcf", "header_forms.vcf",
               "info_forms.vcf", "alt_forms.vcf", "field_counts.vcf", "field_counts_crlf.vcf", "line_mix.vcf",
               "no_final_newline_copied.vcf", "no_final_newline_split.vcf", "no_chrom.vcf", "data_before_chrom.vcf",
               "only_newlines.vcf", "empty.vcf"):
        for form in ("file", "pos", "stdin", "quiet_file", "quiet_stdin"):
            assert "%s__%s" % (fx, form) in BY
    for name in ("missing_file", "help", "help_short", "help_in_group", "bad_long", "bad_short", "version",
                 "missing_argument"):
        assert name in BY


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_reference(case):
    out, err, rc = R.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_the_probe_record():
    """the record of the issue: both rows as the reference wrote them"""
    rows = [ln.split(TAB) for ln in BY["probe.vcf__file"]["stdout"].split(b"\n") if ln.startswith(b"1\t100\t")]
    assert [r[4] for r in rows] == [b"C", b"G"]
    assert rows[0][7:] == [b"AF=0.1;AC=5,6;DB;AD=1,2,3,4,5,6;ZZ=1,2", b"GT:AD:PL:XA", b"1/.:3,4:0,1,2:7", b"0/.:1,2:.:.",
                           b".:.:.:."]
    assert rows[1][7:] == [b"AF=0.2;AC=5,7;DB;AD=1,2,3,4,5,6;ZZ=1,2", b"GT:AD:PL:XA", b"./1:3,5:0,2,3:8", b"0/1:1,.:.:.",
                           b"1/.:.:.:."]
    for form, tail in (("file", [b".", b"GT", b".", b"1/1", b"./1"]), ("stdin", [b".", b"GT", b".", b"1/1", b"./1", b"."])):
        rows = [ln.split(TAB) for ln in BY["probe.vcf__" + form]["stdout"].split(b"\n") if ln.startswith(b"1\t102\t")]
        assert [r[4] for r in rows] == [b"C", b"G", b"T"]
        assert rows[2][7:] == tail
        assert rows[0][7:] == tail[:2] + [b"."] * (len(tail) - 2)


def test_the_modes_differ_where_the_reference_differs():
    for fx in ("probe.vcf", "field_counts.vcf", "line_mix.vcf", "no_chrom.vcf", "data_before_chrom.vcf",
               "only_newlines.vcf"):
        assert BY[fx + "__file"]["stdout"] != BY[fx + "__stdin"]["stdout"], fx
        assert BY[fx + "__file"]["stdout"] == BY[fx + "__pos"]["stdout"] == BY[fx + "__quiet_file"]["stdout"], fx
    assert BY["only_newlines.vcf__file"]["stdout"] == b"" and BY["only_newlines.vcf__stdin"]["stdout"] == b"\n\n\n"
    assert BY["help"]["stdout"] == R.COMMON_HELP and BY["help_in_group"]["stdout"] == R.HELP
    assert all(c["stderr"] == b"" and c["rc"] == 0 for c in CASES if "__" in c["name"])  # the tool never warns


def test_the_later_declaration_of_an_id_wins():
    meta = R.header_part(R.raw_lines(open(R.GOLDEN + "/multiallelic_splitter/header_forms.vcf", "rb").read()))[1]
    assert meta[b"K1"] == (R.FORMAT, b"R") and meta[b"K2"] == (R.INFO, b"A") and meta[b"K4"] == (R.INFO, b"A")
    assert meta[b"K8"][1] == b"A" and meta[b"K9"][1] == b"2" and b"K3" not in meta and b"K5" not in meta
    assert meta[b"KG"] == (R.INFO, b"A") and b"KH" not in meta and b"F3" not in meta and b"" in meta


def test_value_forms():
    assert R.recode_value(b"G", b"0,1,2,3,4,5", 2, 2) == b"0,2,3" and R.recode_value(b"G", b"0,1,2,3,4", 2, 2) == b"."
    assert R.recode_value(b"R", b".", 1, 2) == b"." and R.recode_value(b"R", b"", 1, 2) == b",."
    assert R.recode_value(b"A", b"", 1, 2) == b"" and R.recode_value(b"A", b"", 2, 2) == b"."
    assert R.recode_sample(b"2/10/1", [b"GT"], 2, 2, {}) == b"1/." and R.recode_sample(b"00/1", [b"GT"], 1, 2, {}) == b"./1"
    assert R.fields_of(b"a\t", False) == [b"a"] and R.fields_of(b"a\t", True) == [b"a", b""]


def test_generated_inputs_split_and_copy():
    """the generators of the GPU tests make lines that split, lines that do not, rows that shrink
    and rows that grow"""
    buf = R.gen_vcf(5, 60, 7, odd=0.2, mix=True)
    for stdin in (False, True):
        _, _, per = R.device_view(buf, stdin)
        st = [p[0] for p in per]
        assert st.count(R.SPLIT) >= 20 and st.count(R.COPY) >= 10 and R.EMPTY in st and R.HEADER in st
