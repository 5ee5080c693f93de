#!/usr/bin/env python3
"""Golden vectors of VCFX_cross_sample_concordance: runs the REFERENCE executable (--ref-bin PATH,
built outside the repository with the flags of oracle/Makefile.ref) over the small fixtures this
script writes under tests/golden/concordance/, in file, positional-file and stdin mode.

Writes tests/golden/concordance_cases.json.gz: per case the argv, the stdin fixture, and the
reference's stdout, stderr (base64) and exit code.  The tool runs with cwd=tests/golden, relative
fixture paths and argv[0] = the tool's name, so the names it prints are stable.  Every run that
reaches the file mode's workers carries an explicit -t: the default depends on the host.
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

from tests import _concordance_ref as R  # noqa: E402  (the fixture generators only)

TOOL = R.TOOL
HDR = R.HDR9
DIR = "concordance"


def rec(pos, gts, alt=b"T", fmt=b"GT", tail=b"", chrom=b"1"):
    return b"\t".join([chrom, b"%d" % pos, b".", b"A", alt, b".", b"PASS", b".", fmt] + list(gts)) + tail


def hand_built():
    """every trap of parseGenotypeToId and of the row rules"""
    s = [b"##fileformat=VCFv4.2", HDR + b"\tA\tB\tC\tD\tE\tF"]
    s.append(rec(100, [b"0/1", b"1/0", b"0|1", b"1|0", b"0/1", b"0/1"]))             # phase and order ignored
    s.append(rec(101, [b"0/0", b"0/1", b"1/1", b"0/1", b"0/0", b"1/1"]))
    s.append(rec(102, [b"./.", b".", b"0/.", b"./1", b".|.", b""]))                  # no genotypes
    s.append(rec(103, [b"/0", b"0/x", b"0/", b"1", b"0/1/1", b"|"]))                 # empty runs, no separator
    s.append(rec(104, [b"0/1", b"0/2", b"2/1", b"1/2", b"3/0", b"2/2"], alt=b"T,G"))  # above numAlt
    s.append(rec(105, [b"0/0", b"0/1", b"1/1", b"0/0", b"0/0", b"0/0"], alt=b"."))   # ALT '.': numAlt 0
    s.append(rec(106, [b"0/0", b"0/0", b"0/0", b"0/0", b"0/0", b"0/0"], alt=b""))    # empty ALT
    s.append(rec(107, [b"10/0", b"0/10", b"10/10", b"9/10", b"11/0", b"010/0"], alt=b",".join([b"T"] * 10)))
    s.append(rec(108, [b"127/0", b"128/0", b"127/127", b"0/127", b"128/128", b"1/127"], alt=b",".join([b"T"] * 130)))
    s.append(rec(109, [b"3:0/1", b"5:0/1", b"0/1:7", b"1/1:0/0", b".:0/1", b"0|0:1"], fmt=b"DP:GT"))
    s.append(rec(110, [b"0/1:12,3:15", b"1|0:1,1:2", b"0/1:.", b"1/1:0,9:9", b"./.:.", b"0/0:9,0:9"], fmt=b"GT:AD:DP"))
    s.append(rec(111, [b"0/1", b"1/1"]))                                             # fewer columns than the header
    s.append(rec(112, [b"0/1", b"1/1", b"0/0", b"0/0", b"0/1", b"1/1", b"2/2", b"0/1"]))  # more columns
    s.append(rec(113, [b"0/1", b"0/1", b"0/1"], tail=b"\t"))                         # a line ending in a tab
    s.append(rec(114, []))                                                           # nine fields
    s.append(b"1\t115\t.\tA\tT")                                                     # five fields
    s.append(b"1\t116\t.\tA\t")                                                      # four fields and a tab
    s.append(b"1\t117\t.\tA")                                                        # four fields
    s.append(b"1\t118\t.\tA\tT\t.\tPASS")                                            # seven fields
    s.append(b"1\t119\t.\tA\tT\t.\tPASS\t.")                                         # eight fields
    s.append(rec(120, [b"0/1"] * 6, chrom=b""))                                      # empty CHROM
    s.append(rec(121, [b"1/1", b"", b"1|1", b"", b"1/1", b"1/1"]))             # empty columns
    s.append(rec(122, [b" 0/1", b"0/1 ", b"0 /1", b"+0/1", b"-0/1", b"0/-1"]))       # not digits
    s.append(rec(123, [b"0/1", b"0|1", b"1/0", b"0/1", b"./.", b"0/1"]))             # mixed separators, concordant
    return b"\n".join(s) + b"\n"


def fixtures():
    hb = hand_built()
    lines = hb.split(b"\n")
    dup = b"\n".join([lines[0], HDR + b"\tA\tB\tA\tD\tA\tF"] + lines[2:])
    return {
        "hand.vcf": hb,
        "ragged_a.vcf": R.ragged_vcf(31, 70, 5),
        "ragged_b.vcf": R.ragged_vcf(32, 120, 17),
        "clean.vcf": R.clean_vcf(33, 40, 12, missing=0.05, max_alt=3),
        "crlf.vcf": R.ragged_vcf(34, 60, 6, crlf=True),
        "hand_crlf.vcf": hb.replace(b"\n", b"\r\n"),
        "two_chrom.vcf": b"\n".join([lines[0], lines[1], lines[1]] + lines[2:]),
        "two_chrom_apart.vcf": b"\n".join(lines[:6] + [b"#a comment", b"", HDR + b"\tA\tB\tC"] + lines[6:]),
        "data_before_chrom.vcf": b"\n".join([lines[0], lines[3], lines[4], lines[1]] + lines[2:]),
        "no_chrom.vcf": b"\n".join([lines[0]] + lines[2:]),
        "no_samples.vcf": b"\n".join([lines[0], HDR] + lines[2:]),
        "dup_names.vcf": dup,
        "header_only.vcf": b"\n".join(lines[:2]) + b"\n",
        "no_final_newline.vcf": hb[:-1],
        "eight_lines.vcf": b"\n".join(lines[:10]) + b"\n",
        "empty.vcf": b"",
    }


def build_cases():
    cases = []

    def add(name, args, stdin=None):
        assert name not in {c["name"] for c in cases}, name
        cases.append({"name": name, "argv": [TOOL] + args, "stdin": stdin})

    def p(fx):
        return DIR + "/" + fx

    for fx in ("hand.vcf", "ragged_a.vcf", "clean.vcf"):
        for t in ("1", "2", "3", "64"):
            add("%s__t%s__file" % (fx, t), ["-i", p(fx), "-t", t])
            add("%s__t%s__pos" % (fx, t), ["--threads", t, p(fx)])
        add("%s__stdin" % fx, [], stdin=p(fx))
        add("%s__stdin_t3" % fx, ["-t", "3"], stdin=p(fx))
    for fx in ("ragged_b.vcf", "crlf.vcf", "hand_crlf.vcf", "two_chrom.vcf", "two_chrom_apart.vcf",
               "data_before_chrom.vcf", "no_chrom.vcf", "no_samples.vcf", "dup_names.vcf", "header_only.vcf",
               "no_final_newline.vcf", "empty.vcf"):
        add("%s__t1__file" % fx, ["-i", p(fx), "-t", "1"])
        add("%s__t3__file" % fx, ["-t3", "--input", p(fx)])
        add("%s__stdin" % fx, [], stdin=p(fx))
        add("%s__quiet_t2__file" % fx, ["-q", "-t", "2", p(fx)])
        add("%s__quiet_stdin" % fx, ["--quiet"], stdin=p(fx))
    for t in ("1", "2", "3", "9"):  # eight data lines: T = 9 is clamped to 8
        add("eight_lines__t%s" % t, ["-i", p("eight_lines.vcf"), "-t", t])
    # -s forms
    for tag, s in (("first", "A"), ("last", "F"), ("two", "A,C"), ("second", "B,D,F"), ("none", "X,Y"), ("empty", ""),
                   ("some_unknown", "A,Q,F"), ("dup", "A,A"), ("trailing_comma", "B,")):
        add("hand__s_%s__file" % tag, ["-s", s, "-t", "2", "-i", p("hand.vcf")])
        add("hand__s_%s__stdin" % tag, ["--samples=" + s], stdin=p("hand.vcf"))
    add("hand__two_s__file", ["-s", "A", "-s", "B", "-t", "1", "-i", p("hand.vcf")])
    add("hand_crlf__s_last__file", ["-s", "F", "-t", "2", "-i", p("hand_crlf.vcf")])
    add("hand_crlf__s_last__stdin", ["-s", "F"], stdin=p("hand_crlf.vcf"))   # the name keeps its '\r': no match
    add("hand_crlf__s_first__stdin", ["-s", "A"], stdin=p("hand_crlf.vcf"))
    add("dup_names__s_A__file", ["-s", "A", "-t", "2", "-i", p("dup_names.vcf")])
    add("dup_names__s_A__stdin", ["-s", "A"], stdin=p("dup_names.vcf"))
    add("two_chrom__s_B__file", ["-s", "B", "-t", "1", "-i", p("two_chrom.vcf")])
    add("two_chrom_apart__s_C__file", ["-s", "C", "-t", "3", "-i", p("two_chrom_apart.vcf")])
    add("no_samples__s_A__file", ["-s", "A", "-t", "1", "-i", p("no_samples.vcf")])
    add("i_wins_over_positional", ["-t", "1", "-i", p("hand.vcf"), p("clean.vcf")])
    add("last_i_wins", ["-t", "1", "-i", p("clean.vcf"), "-i", p("hand.vcf")])
    add("missing_file", ["-t", "1", "-i", p("does_not_exist.vcf")])
    add("missing_file_quiet", ["-q", "-t", "1", p("does_not_exist.vcf")])
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", ["-i", p("hand.vcf"), "--help"])
    add("help_in_group", ["-qh"])
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("bad_long", ["--bogus", "-i", p("hand.vcf")])
    add("bad_short", ["-i", p("hand.vcf"), "-x"])
    add("bad_after_help_group", ["-qx", "-h2"])
    add("missing_argument", ["-i", p("hand.vcf"), "-t"])
    add("missing_argument_long", ["--samples"])
    add("ambiguous_prefix", ["--in", p("hand.vcf"), "--thr", "2"])
    add("quiet_with_value", ["--quiet=1"])
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_cross_sample_concordance executable")
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
    path = os.path.join(HERE, "concordance_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
