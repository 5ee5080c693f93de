#!/usr/bin/env python3
"""Golden vectors of VCFX_region_subsampler: runs the REFERENCE executable (--ref-bin PATH, built
outside the repository with the flags of oracle/Makefile.ref) over the small fixtures this script
writes under tests/golden/region_subsampler/ (.vcf and .bed, data only), each VCF with its BED in -i,
stdin and -q forms, plus the command-line forms.

Writes tests/golden/region_subsampler_cases.json.gz: per case the argv, the stdin fixture, and the
reference's stdout, stderr (base64) and exit code.  The tool runs with cwd=tests/golden, relative
fixture paths and argv[0] = the tool's name, so the names it prints are stable.

No fixture holds a NUL byte or a BED start or end of 2147483647: both are outside the tool's domain.
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
sys.path.insert(0, HERE)

from tests import _region_subsampler_ref as R  # noqa: E402  (the fixture generators only)
from make_duplicate_remover_golden import POS_FORMS  # noqa: E402  (every POS form of the two grammars)

TOOL = R.TOOL
DIR = "region_subsampler"
HDR = R.HDR
REST = b".\tA\tC\t.\tPASS\t.\tGT\t0/1"

# every form of the loader: accepted, rejected with a warning, dropped silently
BED_FORMS = [b"chr1 0 100",                    # [1, 100]
             b" chr2\t-5\t10",                 # leading white space, a negative start: [1, 10]
             b"chr6\t007\t+9\r",               # leading zeros, a plus sign, a '\r' after the end: [8, 9]
             b"#chr1\t500\t600",               # a comment
             b"",                              # an empty line
             b"track x",                       # a missing token: warns
             b"chr4 99999999999 5",            # outside int: warns
             b"chr5 5.5 9",                    # the end begins at '.': warns
             b"chr5 0x10 20",                  # the end begins at 'x': warns
             b"chr5 abc 9",                    # no digit: warns
             b"chr5 10 -",                     # a sign without a digit: warns
             b"chr5 10",                       # two tokens: warns
             b"chr5",                          # one token: warns
             b"   ",                           # white space only: warns
             b"\tchr5\t10\t20\textra\tcolumns",  # more columns: ignored
             b"chr5\v30\f40",                  # vertical tab and form feed separate
             b"chr5 50 60abc",                 # the end stops at 'a'
             b"chr5 70 70",                    # empty: dropped silently
             b"chr5 80 79",                    # negative length: dropped silently
             b"chr5 90 -3",                    # a negative end: dropped silently
             b"chr7 5 2147483646",
             b"chr7 -2147483648 3",
             b"chr7 2147483648 3",             # outside int: warns
             b"chr7 1 -2147483649",            # outside int: warns
             b"chr1 150 200", b"chr1 100 120", b"chr1 199 250"]
BED_VCF_POS = [1, 2, 3, 8, 9, 10, 11, 20, 21, 31, 40, 41, 51, 60, 61, 70, 71, 80, 90, 100, 101, 120, 121, 150, 151, 200,
               250, 251, 2147483646, 2147483647]


def bed_forms_vcf():
    s = [HDR.rstrip(b"\n")]
    for c in (b"chr1", b"chr2", b"chr4", b"chr5", b"chr6", b"chr7", b"track", b"#chr1"):
        for p in BED_VCF_POS:
            s.append(R.record(c, b"%d" % p, REST))
    return b"\n".join(s) + b"\n"


def pos_forms():
    s = [HDR.rstrip(b"\n")]
    for i, f in enumerate(POS_FORMS + [b"1e1", b" 7", b"5-5", b"4294967301", b"12345678901234567890"]):
        s.append(R.record(b"c", f, REST + b"\tform%d" % i))
    return b"\n".join(s) + b"\n"


POS_BED = b"c\t0\t60\nc\t999\t1000\nc\t2147483600\t2147483646\n"

# (BED start, BED end) rows: plain, overlapping, nested, touching (end + 1 == the next start in
# 1-based terms: the BED end equals the next BED start), nearly touching (one base between)
BOUNDARY_ROWS = [(b"p", 10, 20), (b"o", 10, 30), (b"o", 20, 40), (b"n", 10, 50), (b"n", 20, 30), (b"t", 10, 20), (b"t", 20, 30),
                 (b"g", 10, 20), (b"g", 21, 30), (b"z", 0, 5), (b"u", 40, 50), (b"u", 10, 20), (b"u", 10, 25), (b"u", 10, 20)]


def boundary_bed():
    return b"".join(b"%s\t%d\t%d\n" % r for r in BOUNDARY_ROWS)


def boundary_vcf():
    s = [HDR.rstrip(b"\n")]
    for c, a, b in BOUNDARY_ROWS:
        for p in (a, a + 1, b, b + 1):
            s.append(R.record(c, b"%d" % p, REST))
    s += [R.record(b"absent", b"15", REST), R.record(b"P", b"15", REST), R.record(b"p ", b"15", REST), R.record(b"p", b"0", REST)]
    return b"\n".join(s) + b"\n"


MIX_BED = b"1\t0\t10\n1\t19\t30\nchr1\t0\t100\n"


def line_mix():
    s = [b"##fileformat=VCFv4.2", b"", R.record(b"1", b"10", REST), b"x", HDR.split(b"\n")[1], b"",
         R.record(b"1", b"10", REST), R.record(b"1", b"11", REST), b"#a comment between data lines", b"", b"",
         b"1", b"1\t", b"1\t10", b"1\t11", b"\t10\t" + REST, b"1\t\t" + REST, b"1\t10\t.\tA\tC\t.\t.", b"1\t10\t.\tA\tC\t.\t.\t",
         b" ", b"\t", b"\t\t\t\t\t\t\t", b"#", b"#CHROM again", R.record(b"1", b"20", REST), R.record(b"2", b"5", REST),
         R.record(b"chr1", b"50", REST), R.record(b"chr1 ", b"50", REST), R.record(b"CHR1", b"50", REST),
         R.record(b"1", b"abc", REST), R.record(b"1", b"-5", REST), R.record(b"1", b" 7", REST), R.record(b"1", b"1e1", REST),
         R.record(b"1", b"+", REST), R.record(b"1", b"99999999999", REST), R.record(b"1", b"25", REST)]
    return b"\n".join(s) + b"\n"


def fixtures():
    lm = line_mix()
    bf = b"\n".join(BED_FORMS) + b"\n"
    gen_bed = R.gen_bed(40, per_chrom=6)
    return {
        "bed_forms.bed": bf,
        "bed_forms_crlf.bed": bf.replace(b"\n", b"\r\n"),
        "bed_forms_no_final_newline.bed": bf + b"chr2\t49\t50",
        "comment_only.bed": b"#chr1\t0\t100\n# nothing else\n",
        "empty.bed": b"",
        "bed_forms.vcf": bed_forms_vcf(),
        "pos.bed": POS_BED,
        "pos_forms.vcf": pos_forms(),
        "boundary.bed": boundary_bed(),
        "boundary.vcf": boundary_vcf(),
        "boundary_crlf.vcf": boundary_vcf().replace(b"\n", b"\r\n"),
        "mix.bed": MIX_BED,
        "line_mix.vcf": lm,
        "line_mix_crlf.vcf": lm.replace(b"\n", b"\r\n"),
        "no_final_newline_in.vcf": lm + R.record(b"1", b"5", REST),
        "no_final_newline_out.vcf": lm + R.record(b"1", b"15", REST),
        "no_final_newline_short.vcf": lm + b"1",
        "no_final_newline_header.vcf": lm + b"#end",
        "generated.bed": gen_bed,
        "generated.vcf": R.gen_vcf(41, 80, gen_bed, mix=True),
        "generated_crlf.vcf": R.gen_vcf(42, 60, gen_bed, mix=True, crlf=True, final_newline=False),
        "header_only.vcf": HDR,
        "only_newlines.vcf": b"\n\n\n",
        "one_line.vcf": b"#CHROM\n1\t5\n",
        "empty.vcf": b"",
    }


# every VCF fixture with the BED it is run against
PAIRS = [("bed_forms.vcf", "bed_forms.bed"), ("bed_forms.vcf", "bed_forms_crlf.bed"),
         ("bed_forms.vcf", "bed_forms_no_final_newline.bed"), ("bed_forms.vcf", "comment_only.bed"),
         ("bed_forms.vcf", "empty.bed"), ("pos_forms.vcf", "pos.bed"), ("boundary.vcf", "boundary.bed"),
         ("boundary_crlf.vcf", "boundary.bed"), ("line_mix.vcf", "mix.bed"), ("line_mix_crlf.vcf", "mix.bed"),
         ("no_final_newline_in.vcf", "mix.bed"), ("no_final_newline_out.vcf", "mix.bed"),
         ("no_final_newline_short.vcf", "mix.bed"), ("no_final_newline_header.vcf", "mix.bed"),
         ("generated.vcf", "generated.bed"), ("generated_crlf.vcf", "generated.bed"), ("header_only.vcf", "mix.bed"),
         ("only_newlines.vcf", "mix.bed"), ("one_line.vcf", "mix.bed"), ("empty.vcf", "mix.bed")]


def build_cases():
    cases = []

    def add(name, args, stdin=None):
        assert name not in {c["name"] for c in cases}, name
        cases.append({"name": name, "argv": [TOOL] + args, "stdin": stdin})

    def p(fx):
        return DIR + "/" + fx

    for vcf, bed in PAIRS:
        tag = "%s+%s" % (vcf, bed)
        add("%s__file" % tag, ["-b", p(bed), "-i", p(vcf)])
        add("%s__stdin" % tag, ["--region-bed", p(bed)], stdin=p(vcf))
        add("%s__quiet_file" % tag, ["-q", "-b", p(bed), "--input", p(vcf)])
        add("%s__quiet_stdin" % tag, ["--quiet", "-b", p(bed)], stdin=p(vcf))
    lm, mb = p("line_mix.vcf"), p("mix.bed")
    add("region_bed_equals", ["--region-bed=" + mb, "--input=" + lm])
    add("attached_value", ["-b" + mb, "-qi" + lm])
    add("prefix_of_long", ["--reg", mb, "--inp", lm, "--qu"])
    add("last_b_wins", ["-b", p("empty.bed"), "-b", mb, "-i", lm])
    add("no_bed", ["-i", lm])
    add("no_bed_stdin", [], stdin=lm)
    add("no_bed_quiet", ["-q"], stdin=lm)
    add("b_without_value", ["-i", lm, "-b"])
    add("region_bed_without_value", ["--region-bed"])
    add("empty_bed_name", ["-b", "", "-i", lm])
    add("missing_bed", ["-b", p("does_not_exist.bed"), "-i", lm])
    add("missing_bed_and_input", ["-b", p("does_not_exist.bed"), "-i", p("does_not_exist.vcf")])
    add("directory_as_bed", ["-b", DIR, "-i", lm])
    add("directory_as_bed_stdin", ["-b", DIR], stdin=lm)
    add("missing_input", ["-b", mb, "-i", p("does_not_exist.vcf")])
    add("missing_input_after_bed_warnings", ["-b", p("bed_forms.bed"), "-i", p("does_not_exist.vcf")])
    add("positional_is_ignored", ["-b", mb, p("boundary.vcf")], stdin=lm)
    add("positional_before_options", [p("boundary.vcf"), "-b", mb], stdin=lm)
    add("double_dash", ["-b", mb, "--", lm], stdin=lm)
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", ["-b", mb, "-i", lm, "--help"])
    add("help_in_group", ["-qh"], stdin=lm)
    add("help_prefix", ["--he"], stdin=lm)
    add("help_wins_over_no_bed", ["-q", "--hel"])
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("bad_long", ["--bogus", "-b", mb, "-i", lm])
    add("bad_short", ["-b", mb, "-i", lm, "-x"])
    add("bad_short_stdin", ["-x"], stdin=lm)
    add("quiet_with_value", ["--quiet=1", "-b", mb], stdin=lm)
    add("missing_argument_i", ["-b", mb, "-i"])
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_region_subsampler executable")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    os.makedirs(os.path.join(HERE, DIR), exist_ok=True)
    for name, data in fixtures().items():
        with open(os.path.join(HERE, DIR, name), "wb") as f:
            f.write(data)
    out = []
    for c in build_cases():
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
    path = os.path.join(HERE, "region_subsampler_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
