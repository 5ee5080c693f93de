#!/usr/bin/env python3
"""Golden vectors of VCFX_duplicate_remover: runs the REFERENCE executable (--ref-bin PATH, built
outside the repository with the flags of oracle/Makefile.ref) over the small fixtures this script
writes under tests/golden/duplicate_remover/, in -i, positional-file, stdin and -q forms.

Writes tests/golden/duplicate_remover_cases.json.gz: per case the argv, the stdin fixture, and the
reference's stdout, stderr (base64) and exit code.  The tool runs with cwd=tests/golden, relative
fixture paths and argv[0] = the tool's name, so the names it prints are stable.

No fixture lets the file mode's POS scan (strtol from the field's first byte) reach the end of the
input, and none holds a NUL byte: both are outside the tool's domain.
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

from tests import _duplicate_remover_ref as R  # noqa: E402  (the fixture generators only)

TOOL = R.TOOL
DIR = "duplicate_remover"
HDR = R.HDR

# every POS form of the two modes; after each, lines that carry the values it may read as
POS_FORMS = [b"55", b" 55", b"\x0b\x0c\r 55", b"+55", b"-55", b"55abc", b"55 ", b"5 5", b"abc", b"", b" ", b"+", b"-",
             b"+-55", b"0", b"-0", b"007", b"0x10", b"1e3", b"2147483647", b"2147483648", b"-2147483648",
             b"-2147483649", b"4294967351", b"-4294967241", b"9223372036854775807", b"9223372036854775808",
             b"-9223372036854775808", b"-9223372036854775809", b"99999999999999999999", b"-99999999999999999999",
             b"18446744073709551671"]
POS_VALUES = [b"0", b"55", b"-55", b"-1", b"7", b"5", b"1", b"16", b"1000", b"2147483647", b"-2147483648"]


def pos_forms():
    s = [HDR.rstrip(b"\n")]
    for i, f in enumerate(POS_FORMS):
        c = b"c%d" % i
        s.append(b"\t".join([c, f, b"id", b"A", b"C", b"form"]))
        for v in POS_VALUES:
            s.append(b"\t".join([c, v, b".", b"A", b"C", b"value"]))
    return b"\n".join(s) + b"\n"


def pos_scan():
    """an empty or blank POS: the file mode reads the number from the next field, or the next line"""
    s = [HDR.rstrip(b"\n"),
         b"1\t\t55\tA\tC",              # file: POS 55 from the ID field
         b"1\t55\tx\tA\tC",             # file: a duplicate; stdin: POS 0 above, so kept
         b"1\t0\ty\tA\tC",              # stdin: a duplicate of the first
         b"2\t \t 66\tG\tT\tq",         # blanks, then the ID field
         b"2\t66\t.\tG\tT",
         b"3\t\t-7\tG\tT",              # a sign in the next field
         b"3\t-7\t.\tG\tT",
         b"4\t\t\t\t",                  # four tabs and nothing else: the scan crosses the newline ...
         b"77\t1\t.\tA\tC",             # ... and reads this line's CHROM
         b"4\t77\t.\t\t",               # file: a duplicate of the four-tab line; stdin: POS 77 against 0
         b"4\t0\t.\t\t",
         b"5\t\t\t\t",                  # the same across an empty line and a '#' line start
         b"",
         b"#88 is not read: '#' is no digit",
         b"5\t0\t.\t\t",
         b"5\t88\t.\t\t",
         b"6\t\tid\tA\tC",              # no number follows: 0
         b"6\t0\t.\tA\tC",
         b"7\t+\t9\tA\tC",              # a sign without digits does not scan on: 0
         b"7\t9\t.\tA\tC",
         b"7\t0\t.\tA\tC"]
    return b"\n".join(s) + b"\n"


def alt_forms():
    s = [HDR.rstrip(b"\n")]

    def grp(chrom, alts, ref=b"A"):
        for k, a in enumerate(alts):
            s.append(b"\t".join([chrom, b"100", b"a%d" % k, ref, a, b"50", b"PASS"]))

    grp(b"1", [b"G,,C", b"G,C,", b"C,G", b",C,G", b"C,G,,", b"G,C"])      # empty tokens: kept (stdin), dropped (file)
    grp(b"2", [b"A,A", b"A", b"A,A,A", b"A,A"])                           # multiplicity counts
    grp(b"3", [b"A,C,T", b"T,C,A", b"C,A,T", b"A,C", b"A,C,T,T"])         # order never matters
    grp(b"4", [b"A,A,C", b"A,C,C", b"C,A,A", b"C,C,A"])
    grp(b"5", [b"", b",", b",,", b"", b"."])                              # an empty ALT field
    grp(b"6", [b"AC,G", b"A,CG", b"ACG", b"G,AC"])                        # the same bytes, other tokens
    grp(b"7", [b"<DEL>,<INS:ME>,*", b"*,<DEL>,<INS:ME>", b"<INS:ME>,*,<DEL>"])
    grp(b"8", [b"a", b"A", b"\xc3\xa9", b"\xff,A", b"A,\xff"])          # raw bytes
    # ALT runs to the fifth tab or to the line's end
    s += [b"9\t5\t.\tA\tC", b"9\t5\tx\tA\tC\tq", b"9\t5\ty\tA\tC\t", b"9\t5\t.\tA\tC,", b"9\t5\t.\tA\t,C\t.\t."]
    # CHROM and REF compare as raw bytes; ID and everything after ALT are not compared
    s += [b"chr1\t7\t.\tA\tC", b"1\t7\t.\tA\tC", b"CHR1\t7\t.\tA\tC", b"chr1\t7\trs1\tA\tC\t99\tq10\tDP=1\tGT\t0/1",
          b"chr1 \t7\t.\tA\tC", b"chr1\t7\t.\ta\tC", b"chr1\t7\t.\tAA\tC", b"chr1\t7\t.\t\tC", b"\t7\t.\tA\tC",
          b"\t7\tz\tA\tC", b"chr1\t07\t.\tA\tC", b"chr1\t7.0\t.\tA\tC", b"chr1\t7\t.\tA\tC\t.\t.\t.\tGT\t1/1"]
    return b"\n".join(s) + b"\n"


def line_mix():
    s = [b"##fileformat=VCFv4.2", b"", b"1\t10\t.\tA\tC\tbefore the header line", HDR.split(b"\n")[1], b"",
         b"1\t10\tdup\tA\tC", b"#a comment between data lines", b"1\t11\t.\tA\tC", b"", b"", b"1\t11\t.\tA\tC\t.",
         b"1\t12\t.\tA", b"1\t12\t.\tA\t", b"1\t12\t.\tA\t", b"1\t12\t.", b"1", b"\t\t\t", b"\t\t\t\t", b"\t\t\t\t",
         b" ", b"#", b"#CHROM again", b"1\t10\t.\tA\tC", b"2\t10\t.\tA\tC"]
    return b"\n".join(s) + b"\n"


def fixtures():
    lm = line_mix()
    return {
        "pos_forms.vcf": pos_forms(),
        "pos_scan.vcf": pos_scan(),
        "alt_forms.vcf": alt_forms(),
        "line_mix.vcf": lm,
        "line_mix_crlf.vcf": lm.replace(b"\n", b"\r\n"),
        "alt_forms_crlf.vcf": alt_forms().replace(b"\n", b"\r\n"),
        "no_final_newline_kept.vcf": lm + b"3\t1\t.\tG\tT",
        "no_final_newline_dup.vcf": lm + b"2\t10\tlast\tA\tC\tq",
        "no_final_newline_short.vcf": lm + b"3\t1\t.\tG",
        "no_final_newline_header.vcf": lm + b"#end",
        "generated.vcf": R.gen_vcf(41, 60, mix=True),
        "generated_crlf.vcf": R.gen_vcf(42, 40, mix=True, crlf=True, final_newline=False),
        "header_only.vcf": HDR,
        "only_newlines.vcf": b"\n\n\n",
        "one_line.vcf": b"1\t5\t.\tA\tC\n",
        "empty.vcf": b"",
    }


def build_cases():
    cases = []

    def add(name, args, stdin=None):
        assert name not in {c["name"] for c in cases}, name
        cases.append({"name": name, "argv": [TOOL] + args, "stdin": stdin})

    def p(fx):
        return DIR + "/" + fx

    for fx in fixtures():
        add("%s__file" % fx, ["-i", p(fx)])
        add("%s__pos" % fx, [p(fx)])
        add("%s__stdin" % fx, [], stdin=p(fx))
        add("%s__quiet_file" % fx, ["-q", "--input", p(fx)])
        add("%s__quiet_stdin" % fx, ["--quiet"], stdin=p(fx))
    add("i_wins_over_positional", ["-i", p("alt_forms.vcf"), p("line_mix.vcf")])
    add("last_i_wins", ["-i", p("line_mix.vcf"), "-i", p("alt_forms.vcf")])
    add("positional_after_q", ["-q", p("line_mix.vcf")])
    add("positional_before_q", [p("line_mix.vcf"), "-q"])
    add("two_positionals", [p("line_mix.vcf"), p("alt_forms.vcf")])
    add("input_equals", ["--input=" + p("line_mix.vcf")])
    add("attached_value", ["-qi" + p("line_mix.vcf")])
    add("prefix_of_long", ["--inp", p("line_mix.vcf"), "--qu"])
    add("dash_is_a_file_name", ["-i", "-"], stdin=p("line_mix.vcf"))
    add("double_dash", ["--", p("line_mix.vcf")])
    add("missing_file", ["-i", p("does_not_exist.vcf")])
    add("missing_file_positional_quiet", ["-q", p("does_not_exist.vcf")])
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", ["-i", p("line_mix.vcf"), "--help"])
    add("help_in_group", ["-qh"], stdin=p("line_mix.vcf"))
    add("help_prefix", ["--he"], stdin=p("line_mix.vcf"))
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("bad_long", ["--bogus", "-i", p("line_mix.vcf")])
    add("bad_short", ["-i", p("line_mix.vcf"), "-x"])
    add("bad_short_stdin", ["-x"], stdin=p("line_mix.vcf"))
    add("missing_argument", ["-q", "-i"])
    add("missing_argument_long", ["--input"])
    add("quiet_with_value", ["--quiet=1"], stdin=p("line_mix.vcf"))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_duplicate_remover executable")
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
    path = os.path.join(HERE, "duplicate_remover_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
