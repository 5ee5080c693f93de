#!/usr/bin/env python3
"""Golden vectors of VCFX_fasta_converter: runs the REFERENCE executable (--ref-bin PATH, built
outside the repository with the flags of oracle/Makefile.ref) over the small fixtures this script
writes under tests/golden/fasta_converter/, in -i, positional-file, stdin and -q forms.

Writes tests/golden/fasta_converter_cases.json.gz: per case the argv, the stdin fixture, and the
reference's stdout, stderr (base64) and exit code.  The tool runs with cwd=tests/golden, relative
fixture paths and argv[0] = the tool's name, so the names it prints are stable.

--ref-data DIR (optional): the reference's own tests/data/fasta_converter; its small .vcf inputs
are copied in as fixtures named ref_<name>.  Without it the copies already here are used.

No fixture holds a GT allele index of more than 9 digits: the reference's int overflows there,
which is outside the tool's domain.
"""
import argparse
import base64
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests import _fasta_converter_ref as R  # noqa: E402  (the fixture generators only)

TOOL = R.TOOL
DIR = "fasta_converter"
HDR = [b"##fileformat=VCFv4.2", b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"g\">"]
REF_DATA = ("basic.vcf", "iupac.vcf", "multiallelic.vcf", "missing.vcf", "malformed.vcf", "missing_columns.vcf",
            "no_gt.vcf", "mixed_ploidy.vcf", "indels.vcf", "adjacent.vcf", "multi_chrom.vcf", "empty.vcf")


def vcf(names, body, hdr=HDR, eol=b"\n", final=True):
    lines = list(hdr) + [R.chrom_line(names)] + list(body)
    return eol.join(lines) + (eol if final else b"")


def rec(ref, alt, fmt, samples, pos=100):
    return b"\t".join([b"1", b"%d" % pos, b".", ref, alt, b".", b".", b".", fmt] + list(samples))


def gt_forms():
    """the GT table with GT first and not first, against 2, 3 and 11 single-base ALT alleles"""
    forms = [b"0/1", b"1|2", b"./.", b".", b"1", b"0", b"1/2/3", b"0/1/2", b"/", b"1/", b"/1", b"0/", b"|0", b"00/1", b"1a/2",
             b"10/2", b"2/10", b"", b"0|0", b"2|1", b"01/2", b"1/02", b"./2", b"2/.", b"|", b"1|", b"|2", b"1/2|3", b"-1/2",
             b" 1/2", b"1/2 ", b"3/3", b"0/3", b"999999999/1", b"11/1", b"1/11", b"0/x", b"0/:4", b"x/0", b"0/1x", b"0x1",
             b"0/.1", b".0/1", b"1/1", b"0/0", b"11/11", b"12/1"]
    names = [b"S%d" % i for i in range(len(forms))]
    pool = [b"C", b"G", b"T", b"A", b"C", b"G", b"T", b"A", b"C", b"G", b"T"]
    body = []
    for n in (2, 3, 11):
        alts = b",".join(pool[:n])
        body.append(rec(b"A", alts, b"GT", forms, 100 + n))
        body.append(rec(b"A", alts, b"DP:GT", [b"7:" + f for f in forms], 200 + n))
        body.append(rec(b"A", alts, b"GT:DP", [f + b":7" for f in forms], 300 + n))
    return vcf(names, body)


def alt_forms():
    """ALT pieces multi-base, lower-case, '*', '.', <DEL>, empty between commas, a trailing comma;
    alleles past the list; 17 alleles with GTs that use alleles 15, 16 and 17"""
    gts = [b"0/1", b"1/1", b"0/2", b"2/2", b"1/2", b"2/1", b"3/3", b"0/3", b"3/1", b"4/4", b"0/0"]
    names = [b"S%d" % i for i in range(len(gts))]
    body = [rec(b"A", alt, b"GT", gts, 100 + i) for i, alt in enumerate(
        (b"C", b"C,G", b"C,G,T", b"AC,G", b"c,g", b"*,C", b".,C", b".", b"<DEL>,T", b"C,,G", b"C,", b",", b",C", b",,", b"",
         b"C,G,", b"N,C", b"R,Y", b"[,C", b"1,C", b"C,GT,T", b"\xe9,C"))]
    many = b",".join([b"C", b"G", b"T", b"A"] * 4 + [b"G"])  # 17 ALT alleles
    wide = [b"15/15", b"16/16", b"17/17", b"0/16", b"16/0", b"17/1", b"18/18", b"0/18", b"15/16", b"16/17", b"9/10"]
    body.append(rec(b"A", many, b"GT", wide, 500))
    body.append(rec(b"A", many + b",AC,t", b"GT:DP", [w + b":3" for w in wide], 501))
    return vcf(names, body)


def ref_forms():
    """REF lower-case, multi-base, '.', '{', 0xE9, '~', empty, a digit"""
    gts = [b"0/0", b"0/1", b"1/0", b"1/1", b"0|0", b"./0"]
    names = [b"S%d" % i for i in range(len(gts))]
    body = [rec(r, b"C", b"GT", gts, 100 + i) for i, r in enumerate(
        (b"A", b"a", b"c", b"g", b"t", b"AT", b".", b"{", b"\xe9", b"~", b"", b"7", b"N", b"n", b"z", b"`", b"\x7f", b"\xff"))]
    return vcf(names, body)


def format_forms():
    """FORMAT without GT, with GT late, empty keys, a key that only starts with GT"""
    s = [b"0/1:1:2", b"1/1", b"", b":0/1", b"::1/1", b"5:0/1:7"]
    names = [b"S%d" % i for i in range(len(s))]
    body = [rec(b"A", b"C", f, s, 100 + i) for i, f in enumerate(
        (b"GT", b"GT:DP", b"DP:GT", b"DP:AD:GT", b"DP", b"", b":", b":GT", b"::GT", b"GTX:GT", b"XGT", b"gt", b"GT:GT",
         b"DP:GT:", b"GT ", b"G:T:GT"))]
    return vcf(names, body)


def line_forms():
    """short, long and empty lines, '#' lines among the data, trailing tabs"""
    good = rec(b"A", b"C", b"GT", [b"0/1", b"1/1", b"0/0"])
    nine = b"\t".join(good.split(b"\t")[:9])
    body = [good, b"", b"#comment", rec(b"A", b"C", b"GT", [b"0/1"]), rec(b"A", b"C", b"GT", [b"0/1", b"1/1"]),
            rec(b"A", b"C", b"GT", [b"0/1", b"1/1", b"0/0", b"1/1", b"1/1"]), nine, nine + b"\t", nine + b"\t\t",
            b"1\t5\t.\tA", b"1\t5\t.\tA\t", b"x", b" ", b"\t", b"\t" * 9, b"\t" * 12, good + b"\t", good + b"\t\t",
            rec(b"A", b"C", b"GT", [b"0/1", b"", b"1/1"]), rec(b"A", b"C", b"GT", [b"", b"", b""]),
            rec(b"A", b"C", b"GT", [b"0/1", b"1/1", b""]), b"##late=header", good]
    return vcf([b"S1", b"S2", b"S3"], body)


def two_headers():
    a = rec(b"A", b"C", b"GT", [b"0/1"])
    b = rec(b"A", b"G", b"GT", [b"0/0", b"0/1", b"1/1"])
    return vcf([b"S1"], [a, rec(b"C", b"T", b"GT", [b"1/1"]), R.chrom_line([b"S2", b"S3"]), b, a, b])


def columns(n):
    return vcf([b"A1", b"B2"], [rec(b"ACGT"[i % 4:i % 4 + 1], b"ACGT"[(i + 1) % 4:(i + 1) % 4 + 1], b"GT",
                                    [(b"0/0", b"0/1", b"1/1")[i % 3], (b"1|0", b"./.", b"0|0")[i % 3]], 100 + i)
                                for i in range(n)])


def fixtures(ref_data=None):
    good = rec(b"A", b"C", b"GT", [b"0/1", b"1/1"])
    hdr = vcf([b"S1", b"S2"], [])
    fx = {
        "gt_forms.vcf": gt_forms(),
        "gt_forms_crlf.vcf": gt_forms().replace(b"\n", b"\r\n"),
        "alt_forms.vcf": alt_forms(),
        "ref_forms.vcf": ref_forms(),
        "format_forms.vcf": format_forms(),
        "line_forms.vcf": line_forms(),
        "line_forms_crlf.vcf": line_forms().replace(b"\n", b"\r\n"),
        "two_headers.vcf": two_headers(),
        "two_headers_crlf.vcf": two_headers().replace(b"\n", b"\r\n"),
        "data_before_chrom.vcf": b"\n".join(HDR) + b"\n" + good + b"\n" + hdr + good + b"\n",
        "empty_line_before_chrom.vcf": b"\n".join(HDR) + b"\n\n" + hdr + good + b"\n",
        "chrom_after_data_only.vcf": good + b"\n" + good + b"\n" + R.chrom_line([b"S1", b"S2"]) + b"\n",
        "data_only.vcf": good + b"\n" + good + b"\n",
        "no_final_newline.vcf": hdr + good + b"\n" + good,
        "no_final_newline_crlf.vcf": (hdr + good + b"\n" + good).replace(b"\n", b"\r\n") + b"\r",
        "no_final_newline_header.vcf": hdr[:-1],
        "no_samples.vcf": vcf([], [b"\t".join(good.split(b"\t")[:9]), good]),
        "header_only.vcf": hdr,
        "hash_lines_only.vcf": b"\n".join(HDR) + b"\n",
        "only_newlines.vcf": b"\n\n\n",
        "chrom_trailing_tab.vcf": b"\n".join(HDR) + b"\n" + R.chrom_line([b"S1", b"", b"S3"]) + b"\t\n" +
        rec(b"A", b"C", b"GT", [b"0/1", b"1/1", b"0/0"]) + b"\n",
        "chrom_prefix.vcf": b"#CHROMOSOME\tx\ty\n#CHROM\n" + good + b"\n",
        "cols_59.vcf": columns(59),
        "cols_60.vcf": columns(60),
        "cols_61.vcf": columns(61),
        "cols_120.vcf": columns(120),
        "generated.vcf": R.gen_vcf(41, 70, 5, fmt=b"GT:AD:DP", odd=0.3, mix=True),
        "generated_gt.vcf": R.gen_vcf(42, 130, 7, clean=True),
        "generated_crlf.vcf": R.gen_vcf(43, 40, 3, odd=0.3, mix=True, crlf=True, final_newline=False),
        "generated_two_headers.vcf": R.gen_vcf(44, 50, 3, odd=0.2, mix=True, second_header=(20, [b"X1", b"X2"])),
        "empty.vcf": b"",
    }
    for name in REF_DATA:
        path = os.path.join(ref_data, name) if ref_data else os.path.join(HERE, DIR, "ref_" + name)
        with open(path, "rb") as f:
            fx["ref_" + name] = f.read()
    return fx


def build_cases(fx):
    cases = []

    def add(name, args, stdin=None):
        assert name not in {c["name"] for c in cases}, name
        cases.append({"name": name, "argv": [TOOL] + args, "stdin": stdin})

    def p(name):
        return DIR + "/" + name

    for name in fx:
        add("%s__file" % name, ["-i", p(name)])
        add("%s__pos" % name, [p(name)])
        add("%s__stdin" % name, [], stdin=p(name))
        add("%s__quiet_file" % name, ["-q", "--input", p(name)])
        add("%s__quiet_stdin" % name, ["--quiet"], stdin=p(name))
    add("i_wins_over_positional", ["-i", p("gt_forms.vcf"), p("line_forms.vcf")])
    add("last_i_wins", ["-i", p("line_forms.vcf"), "-i", p("gt_forms.vcf")])
    add("positional_before_q", [p("gt_forms.vcf"), "-q"])
    add("two_positionals", [p("gt_forms.vcf"), p("line_forms.vcf")])
    add("input_equals", ["--input=" + p("gt_forms.vcf")])
    add("attached_value", ["-qi" + p("gt_forms.vcf")])
    add("prefix_of_long", ["--inp", p("gt_forms.vcf"), "--qu"])
    add("dash_is_a_file_name", ["-i", "-"], stdin=p("gt_forms.vcf"))
    add("double_dash", ["--", p("gt_forms.vcf")])
    add("empty_input_name", ["-i", ""], stdin=p("gt_forms.vcf"))
    add("missing_file", ["-i", p("does_not_exist.vcf")])
    add("missing_file_positional_quiet", ["-q", p("does_not_exist.vcf")])
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", ["-i", p("gt_forms.vcf"), "--help"])
    add("help_in_group", ["-qh"], stdin=p("gt_forms.vcf"))
    add("help_prefix", ["--he"], stdin=p("gt_forms.vcf"))
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("bad_long", ["--bogus", "-i", p("gt_forms.vcf")])
    add("bad_short", ["-i", p("gt_forms.vcf"), "-x"])
    add("bad_short_stdin", ["-x"], stdin=p("gt_forms.vcf"))
    add("two_bad_options", ["-x", "-y", "--bogus"])
    add("missing_argument", ["-q", "-i"])
    add("missing_argument_long", ["--input"])
    add("quiet_with_value", ["--quiet=1"], stdin=p("gt_forms.vcf"))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_fasta_converter executable")
    ap.add_argument("--ref-data", help="the reference's tests/data/fasta_converter (its inputs become fixtures)")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    os.makedirs(os.path.join(HERE, DIR), exist_ok=True)
    fx = fixtures(a.ref_data)
    for name, data in fx.items():
        assert len(data) < 100000, name
        with open(os.path.join(HERE, DIR, name), "wb") as f:
            f.write(data)
    out = []
    for c in build_cases(fx):
        stdin = b""
        if c["stdin"]:
            with open(os.path.join(HERE, c["stdin"]), "rb") as f:
                stdin = f.read()
        r = subprocess.run(c["argv"], executable=ref, input=stdin, capture_output=True, cwd=HERE, timeout=120)
        c["rc"] = r.returncode
        c["stdout"] = base64.b64encode(r.stdout).decode()
        c["stderr"] = base64.b64encode(r.stderr).decode()
        out.append(c)
    blob = json.dumps({"tool": TOOL, "cases": out}, indent=0, sort_keys=True).encode()
    path = os.path.join(HERE, "fasta_converter_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
