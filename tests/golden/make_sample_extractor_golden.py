#!/usr/bin/env python3
"""Golden vectors of VCFX_sample_extractor: runs the REFERENCE executable (--ref-bin PATH, built
outside the repository with the flags of oracle/Makefile.ref) over the small fixtures this
script writes under tests/golden/sample_extractor/, in file (-i), positional-file and stdin mode.

Writes tests/golden/sample_extractor_cases.json.gz: per case the argv, the input file or the
stdin fixture, and the reference's stdout, stderr (base64) and exit code.  The tool runs with
cwd=tests/golden, relative fixture paths and argv[0] = the tool's name, so the file names and
the getopt messages it prints are stable.
"""
import argparse
import base64
import gzip
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
TOOL = "VCFX_sample_extractor"
DIR = "sample_extractor"
HDR = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"


def rec(pos, cols, fmt=b"GT", tail=b""):
    return b"\t".join([b"1", b"%d" % pos, b"rs%d" % pos, b"A", b"T", b"50", b"PASS", b"DP=%d" % pos, fmt] + list(cols)) + tail


def hand_built():
    """six samples, one name twice in the header; lines of 6, 7, 8 and 9 fields, ragged lines, a
    line ending in a tab, an empty sample field, GT:AD:DP fields, more columns than the header"""
    s = [b"##fileformat=VCFv4.2", b"##source=hand", HDR + b"\tA\tB\tC\tD\tB\tF"]
    s.append(rec(100, [b"0/0", b"0/1", b"1/1", b"0|1", b"1|0", b"./."]))
    s.append(rec(101, [b"0/1:10,2:12", b"1/1:0,9:9", b"0/0:7,0:7", b".:.:.", b"0|1:3,3:6", b"1|1:1,8:9"], fmt=b"GT:AD:DP"))
    s.append(rec(102, [b"0/0", b"0/1", b"1/1"]))                         # ragged: 12 fields
    s.append(rec(103, [b"0/0"]))                                         # ragged: 10 fields
    s.append(rec(104, []))                                               # 9 fields
    s.append(b"\t".join(rec(105, []).split(b"\t")[:8]))                   # 8 fields
    s.append(b"\t".join(rec(106, []).split(b"\t")[:7]))                   # 7 fields
    s.append(b"\t".join(rec(107, []).split(b"\t")[:6]))                   # 6 fields
    s.append(rec(108, [b"0/0", b"0/1", b"1/1", b"0|1"], tail=b"\t"))      # ends in a tab: an empty 14th field
    s.append(rec(109, [b"0/0", b"", b"1/1", b"", b"1|0", b""]))           # empty sample fields
    s.append(rec(110, [b"0/0", b"0/1", b"1/1", b"0|1", b"1|0", b"./.", b"9/9", b"8/8"]))  # more columns
    s.append(rec(111, [], tail=b"\t"))                                    # 9 fields and a tab
    s.append(b"\t".join(rec(112, []).split(b"\t")[:8]) + b"\t")           # 8 fields and a tab: FORMAT empty
    s.append(b"x")                                                        # one field
    s.append(rec(113, [b"1/1", b"1/0", b"0/1", b"0/0", b"1|1", b"0|0"]))
    return b"\n".join(s) + b"\n"


def fixtures():
    hb = hand_built()
    lines = hb.split(b"\n")[:-1]
    head, chrom, data = lines[:2], lines[2], lines[3:]
    join = lambda ls: b"\n".join(ls) + b"\n"  # noqa: E731
    return {
        "hand.vcf": hb,
        "hand_crlf.vcf": hb.replace(b"\n", b"\r\n"),
        "no_final_newline.vcf": hb[:-1],
        "no_final_newline_crlf.vcf": hb.replace(b"\n", b"\r\n")[:-2],
        "last_kept_crlf.vcf": join(head + [chrom] + data[:2]).replace(b"\n", b"\r\n"),
        "two_chrom.vcf": join(head + [chrom] + data[:3] + [HDR + b"\tF\tA\tQ"] + data[3:]),
        "data_before_chrom.vcf": join(head + data[:2] + [b""] + [chrom] + data[2:]),
        "no_chrom.vcf": join(head + data),
        "chrom8.vcf": join(head + [b"\t".join(HDR.split(b"\t")[:8])] + data),
        "chrom9.vcf": join(head + [HDR] + data),
        "chrom8_then_full.vcf": join(head + [b"\t".join(HDR.split(b"\t")[:8])] + data[:4] + [chrom] + data[4:]),
        "hash_inside.vcf": join(head + [chrom] + data[:4] + [b"#a comment\twith a tab", b"", b"##another", b"#"] + data[4:]
                                + [b"", b"#CHROMosome"]),
        "header_only.vcf": join(head + [chrom]),
        "empty_lines_only.vcf": b"\n\n\r\n\n",
        "empty.vcf": b"",
    }


SEL = {
    "one": ["-s", "C"],
    "none_found": ["-s", "X,Y"],
    "all": ["-s", "A,B,C,D,F"],
    "dup_request": ["-s", "C,A,C,Z,Z"],
    "dup_header": ["-s", "B"],
    "twice": ["-s", "A", "--samples", "F"],
    "space_list": ["--samples", "D A  F"],
    "mixed_list": ["--samples=A, ,,B\tC,"],
    "first_last": ["-sA,F"],
}


def build_cases():
    cases = []

    def add(name, args, file=None, stdin=None):
        cases.append({"name": name, "argv": [TOOL] + args, "file": file, "stdin": stdin})

    for fx in ("hand.vcf", "hand_crlf.vcf"):
        p = DIR + "/" + fx
        for tag, sel in SEL.items():
            add("%s__%s__file" % (fx, tag), sel + ["-i", p], file=p)
            add("%s__%s__pos" % (fx, tag), [p] + sel, file=p)
            add("%s__%s__stdin" % (fx, tag), sel, stdin=p)
    for fx in ("no_final_newline.vcf", "no_final_newline_crlf.vcf", "last_kept_crlf.vcf", "two_chrom.vcf",
               "data_before_chrom.vcf", "no_chrom.vcf", "chrom8.vcf", "chrom9.vcf", "chrom8_then_full.vcf",
               "hash_inside.vcf", "header_only.vcf", "empty_lines_only.vcf", "empty.vcf"):
        p = DIR + "/" + fx
        for tag in ("first_last", "none_found", "dup_request"):
            add("%s__%s__file" % (fx, tag), SEL[tag] + ["--input", p], file=p)
            add("%s__%s__stdin" % (fx, tag), SEL[tag], stdin=p)
        add("%s__one__pos" % fx, ["-s", "F", p], file=p)
        add("%s__one__dash" % fx, ["-s", "F", "-i", "-"], stdin=p)
    hand = DIR + "/hand.vcf"
    add("missing_file", ["-s", "A", "-i", DIR + "/does_not_exist.vcf"])
    add("missing_file_pos", ["-s", "A", DIR + "/does_not_exist.vcf"])
    add("no_args", [])
    add("no_samples_file", ["-i", hand], file=hand)
    add("no_samples_stdin", ["-i", "-"], stdin=hand)
    add("only_separators", ["-s", " ,, ", "-i", hand], file=hand)
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", ["-s", "A", "-i", hand, "--help"], file=hand)
    add("help_abbrev", ["--he", "-s", "A"])
    add("version", ["--version"])
    add("version_short", ["-s", "A", "-v"])
    add("unknown_long", ["--bogus", "-s", "A", "-i", hand], file=hand)
    add("unknown_short", ["-s", "A", "-x", hand], file=hand)
    add("missing_value", ["-i", hand, "-s"], file=hand)
    add("input_wins_over_positional", ["-s", "A", "-i", hand, DIR + "/does_not_exist.vcf"], file=hand)
    add("double_dash", ["-s", "F", "--", hand], file=hand)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_sample_extractor executable")
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
    path = os.path.join(HERE, "sample_extractor_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
