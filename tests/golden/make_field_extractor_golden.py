#!/usr/bin/env python3
"""Golden vectors of VCFX_field_extractor: runs the REFERENCE executable (--ref-bin PATH, built outside
the repository with the flags of oracle/Makefile.ref) over the small fixtures this script writes under
tests/golden/field_extractor/ (data only), each with several field lists in file mode (-i, a
positional file) and stdin mode (no file, -i -), plus the command-line forms.

Writes tests/golden/field_extractor_cases.json.gz: per case the argv, the stdin fixture, and the
reference's stdout, stderr (base64) and exit code.  The tool runs with cwd=tests/golden, relative
fixture paths and argv[0] = the tool's name, so the names it prints are stable.

No case holds a field on which the reference aborts ('S' alone or an index outside int before the
colon): every recorded exit code is 0 or 1.  No fixture holds a NUL byte.
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

from tests import _field_extractor_ref as R  # noqa: E402  (the fixture generators only)

TOOL = R.TOOL
DIR = "field_extractor"
HDR = R.HDR


def rec(info=b"DP=5", fmt=b"GT:DP", samples=(b"0/1:3", b"1|1:4", b"0|0:5", b"./.:6", b"1/1:7"), chrom=b"1", pos=b"100",
        id_=b"rs1", filt=b"PASS"):
    return b"\t".join((chrom, pos, id_, b"A", b"C", b"50", filt, info, fmt) + tuple(samples))


def rules_vcf(nl=b"\n", final=True):
    lines = [b"##fileformat=VCFv4.2", HDR.split(b"\n")[1]]
    for info in R.INFOS:
        lines.append(rec(info))
    for fmt in R.FORMATS:
        lines.append(rec(fmt=fmt))
    lines += [
        rec(samples=(b"0/1", b"", b":", b"0/1:", b":9")),           # fewer tokens than FORMAT, empty tokens
        rec(fmt=b"DP:GT", samples=(b"7", b"7:", b"7:0/1:x", b"::", b"")),
        rec(id_=b"", filt=b"", chrom=b""),                          # empty standard columns
        rec(info=b"AF=;DP="),                                       # found but empty
        b"1", b"1\t5", b"\t", b"1\t5\tid\tA\tC\t9\tPASS\tDP=8",      # 1, 2, 2 and 8 fields
        b"1\t5\tid\tA\tC\t9\tPASS\tDP=8\tGT", b"1\t5\tid\tA\tC\t9\tPASS\tDP=8\tGT\t0/1",  # 9 and 10
        b"1\t5\tid\tA\tC\t9\tPASS\tDP=8\tGT\t0/1\t",                 # a trailing tab
        b"", b"#not a header\tDP=1",
        rec(info=b"DP=1;DP=2;DP=3"),                                # duplicate keys
    ]
    return nl.join(lines) + (nl if final else b"")


def fixtures():
    fx = {
        "rules.vcf": rules_vcf(),
        "rules_crlf.vcf": rules_vcf(b"\r\n"),
        "rules_no_final_newline.vcf": rules_vcf(final=False),
        "rules_crlf_no_final_newline.vcf": rules_vcf(b"\r\n", final=False),
        "header_only.vcf": HDR,
        "empty.vcf": b"",
        "only_newlines.vcf": b"\n\n\n",
        "no_header.vcf": rec() + b"\n" + rec(info=b"AF=1") + b"\n",
        "data_first.vcf": rec(info=b"NA1:GT=early") + b"\n" + HDR + rec() + b"\n",
        "second_chrom.vcf": HDR + rec() + b"\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA2\tNA1\n" + rec() + b"\n",
        "short_chrom.vcf": b"#CHROM\tPOS\n" + rec() + b"\n",
        "chrom_trailing_tab.vcf": HDR[:-1] + b"\t\n" + rec(samples=(b"a:1", b"b:2", b"c:3", b"d:4", b"e:5", b"f:6")) + b"\n",
        "generated.vcf": R.gen_vcf(11, 60),
        "generated_crlf.vcf": R.gen_vcf(12, 60, crlf=True, final_newline=False),
    }
    return fx


LISTS = {
    "std": "CHROM,POS,ID,REF,ALT,QUAL,FILTER,INFO",
    "keys": "DP,DP4,ADP,X,AF,DB,H2,,chrom,pos",
    "samples": "NA1:GT,NA2:DP,dup:GT,dup:DP,S1:GT,S2:DP,S5:GT,S6:GT,S0:GT,S005:DP,absent:GT,NA1:,S1:,S3:GT,S3:GQ,NA1:GT:x",
    "mixed": R.GEN_FIELDS,
}


def build_cases():
    cases = []

    def add(name, args, stdin=None):
        assert name not in {c["name"] for c in cases}, name
        cases.append({"name": name, "argv": [TOOL] + args, "stdin": stdin})

    def p(fx):
        return DIR + "/" + fx

    for fx in sorted(fixtures()):
        for tag, fields in LISTS.items():
            if tag in ("std", "keys", "samples") and not fx.startswith(("rules", "generated", "data_first", "second", "chrom_t")):
                continue
            add("%s+%s__file" % (fx, tag), ["-f", fields, "-i", p(fx)])
            add("%s+%s__stdin" % (fx, tag), ["--fields", fields], stdin=p(fx))
    r = p("rules.vcf")
    add("positional_file", ["-f", "CHROM,DP", r])
    add("positional_before_options", [r, "-f", "CHROM,DP"])
    add("positional_with_stdin", ["-f", "CHROM,AF", r], stdin=p("generated.vcf"))
    add("i_wins_over_positional", ["-f", "CHROM,DP", "-i", r, p("generated.vcf")])
    add("empty_i_then_positional", ["-f", "CHROM,DP", "-i", "", r])
    add("i_dash", ["-f", "CHROM,AF,NA1:GT", "-i", "-"], stdin=r)
    add("positional_dash", ["-f", "CHROM,AF,NA1:GT", "-"], stdin=r)
    add("double_dash", ["-f", "CHROM,DP", "--", r])
    add("repeated_f", ["-f", "CHROM,POS", "-f", "DP", "--fields", "NA1:GT,", "-i", r])
    add("repeated_f_stdin", ["-f", "CHROM", "-f", "", "-f", "AF"], stdin=r)
    add("empty_field_list", ["-f", "", "-i", r])
    add("empty_field_list_stdin", ["-f", ""], stdin=r)
    add("empty_items", ["-f", ",CHROM,,DP,", "-i", r])
    add("empty_items_stdin", ["-f", ",CHROM,,DP,"], stdin=r)
    add("fields_equals", ["--fields=CHROM,DP", "--input=" + r])
    add("attached_value", ["-fCHROM,DP", "-i" + r])
    add("prefix_of_long", ["--fi", "CHROM", "--inp", r])
    add("case_matters", ["-f", "chrom,Pos,INFO,info", "-i", r])
    add("no_fields", ["-i", r])
    add("no_fields_stdin", [], stdin=r)
    add("no_fields_missing_file", ["-i", p("does_not_exist.vcf")])
    add("missing_file", ["-f", "CHROM", "-i", p("does_not_exist.vcf")])
    add("missing_positional", ["-f", "CHROM", p("does_not_exist.vcf")])
    add("empty_file_positional", ["-f", "CHROM", p("empty.vcf")])
    add("empty_stdin", ["-f", "CHROM,DP"])
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", ["-f", "CHROM", "-i", r, "--help"])
    add("help_in_group", ["-hf", "CHROM"], stdin=r)
    add("help_prefix", ["--he"], stdin=r)
    add("help_wins_over_no_fields", ["--hel"])
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("bad_long", ["--bogus", "-f", "CHROM", "-i", r])
    add("bad_short", ["-f", "CHROM", "-i", r, "-x"])
    add("bad_short_stdin", ["-x"], stdin=r)
    add("bad_wins_over_no_fields", ["-x", "-i", r])
    add("f_without_value", ["-i", r, "-f"])
    add("fields_without_value", ["--fields"])
    add("i_without_value", ["-f", "CHROM", "-i"])
    add("help_with_value", ["--help=1", "-f", "CHROM"], stdin=r)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_field_extractor executable")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    os.makedirs(os.path.join(HERE, DIR), exist_ok=True)
    for name, data in fixtures().items():
        assert b"\0" not in data
        with open(os.path.join(HERE, DIR, name), "wb") as f:
            f.write(data)
    out = []
    for c in build_cases():
        fields = [v for k, v, _ in R.getopt_long(c["argv"])[0] if k == "f"]
        assert R.bad_field(",".join(fields).split(",")) is None, c["name"]
        stdin = b""
        if c["stdin"]:
            with open(os.path.join(HERE, c["stdin"]), "rb") as f:
                stdin = f.read()
        r = subprocess.run(c["argv"], executable=ref, input=stdin, capture_output=True, cwd=HERE, timeout=120)
        assert r.returncode in (0, 1), (c["name"], r.returncode)
        c["rc"] = r.returncode
        c["stdout"] = base64.b64encode(r.stdout).decode()
        c["stderr"] = base64.b64encode(r.stderr).decode()
        out.append(c)
    blob = json.dumps({"tool": TOOL, "cases": out}, indent=0, sort_keys=True).encode()
    path = os.path.join(HERE, "field_extractor_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
