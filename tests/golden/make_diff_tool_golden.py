#!/usr/bin/env python3
"""Golden vectors of VCFX_diff_tool: runs the REFERENCE executable (--ref-bin PATH, built outside the
repository with the flags of oracle/Makefile.ref) over the small fixtures this script writes under
tests/golden/diff_tool/, in the default mode, -s, -s -n and the help / version / error forms.

Writes tests/golden/diff_tool_cases.json.gz: per case the argv, the environment it is recorded for
(the .vcf.gz pair: VCFX_GZIP=0, the reference reads the compressed bytes as text), the reference's
stdout, stderr (base64) and exit code, and `ordered`.  The tool runs with cwd=tests/golden, relative
fixture paths and argv[0] = the tool's name, so the names it prints are stable.

`ordered` is true for every -s case and every case whose sections hold at most one key each: those
are compared byte for byte.  The other default-mode cases print each side in the iteration order of
the reference's unordered_set and are compared by tests/_diff_tool_ref.py same_sections().  At least
a third of all cases are ordered (asserted): the helper is never the only check.
"""
import argparse
import base64
import gzip
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests import _diff_tool_ref as R  # noqa: E402  (the generators and the sort key of the sorted fixtures)

TOOL = R.TOOL
DIR = "diff_tool"
HDR = R.HDR
rec = R.rec

# the natural-order name zoo of make_sorter_golden.py
NAMES = [b"1", b"2", b"10", b"22", b"23", b"0", b"9", b"chr1", b"Chr1", b"CHR1", b"cHr1", b"CHr1", b"chR1", b"chr2", b"chr10",
         b"chr22", b"M", b"MT", b"X", b"Y", b"x", b"chrM", b"chrX", b"CHRX", b"ChrY", b"MT_alt", b"2_random", b"chr2_random",
         b"1x", b"1a", b"01", b"001", b"chr01", b"chr", b"CHR", b"Chr", b"ch", b"c", b"", b"chr0", b"HLA-A*01:01", b"\xc3\xa9",
         b"chr\xff", b"GL000220.1"]


def text(lines, final_newline=True):
    return b"\n".join(lines) + (b"\n" if final_newline else b"")


def ordered(lines, natural=False):
    """the data lines sorted (stably) under compareKeys"""
    return sorted(lines, key=lambda l: R.sort_key(R.parse(l)[1], natural))


def rules(side):
    """every line rule, '#' and empty lines between the data; the two sides share some keys"""
    s = [b"##fileformat=VCFv4.2", b"", HDR.split(b"\n")[1], rec(b"1", b"100"), b"#a comment between data lines",
         b"no_tab_at_all", b"1\t101", b"1\t102\t.", b"1\t103\t.\tA", b"1\t104\t.\tA\t", b"1\t105\t.\tA\tT", b"\t\t\t\t", b"\t\t\t",
         rec(b"1", b"", b"A", b"G"), rec(b"1", b"12a"), rec(b"1", b"-5"), rec(b"1", b" 7"), rec(b"1", b"+3"), rec(b"1", b"1.0"),
         rec(b"1", b"007"), rec(b"", b"9"), rec(b"2", b"5", b"", b""), b"", b"", b"\r", b"#\r", b"1\t106\t.\tA\tC\r",
         b"1\t107\t.\tA\r", b"1\t108\t.\tA\t\r", b"1\t109\t.\tA\tC\t\r", rec(b"1", b"100"),
         rec(b"n\x00ul", b"4", b"A\x00", b"\x00"), rec(b"\xff\xfe", b"4", b"\x80", b"\xc3\xa9,\x80,\xff")]
    if side == 1:
        s = s[:3] + [rec(b"1", b"7"), rec(b"2", b"5", b"", b""), b"1\t105\t.\tA\tT\tonly in two"] + s[12:20] + \
            [rec(b"4", b"1"), rec(b"\xff\xfe", b"4", b"\x80", b"\xff,\x80,\xc3\xa9"), b"1\t106\t.\tA\tC", rec(b"4", b"1")]
    return s


def alts(side):
    """ALT permutations, empty tokens, repeated tokens, a prefix before its extensions, bytes >= 0x80"""
    a = [b"A,C,G", b",A", b"A,,", b"A,A,C", b"AT,A,ATT", b"\xc3\xa9,\x80,z", b",", b"", b"T,<DEL>,*", b"C,c", b"G"]
    b = [b"G,A,C", b"A,", b",A,", b"A,C,A", b"ATT,AT,A", b"z,\x80,\xc3\xa9", b",", b"", b"*,T,<DEL>", b"c,C", b"G,G"]
    extra = [rec(b"7", b"70", b"A", b"A,C")] if side == 0 else [rec(b"7", b"70", b"A", b"A,C,C"), rec(b"7", b"71", b"A", b"C,A")]
    return [rec(b"5", b"%d" % (10 + i), b"A", x) for i, x in enumerate(b if side else a)] + extra


def zoo(side, natural):
    """the name zoo, sorted under the order it is compared in; the sides differ in a few names"""
    names = [n for i, n in enumerate(NAMES) if i % 7 != (2 if side else 5)]
    return ordered([rec(n, b"%d" % p) for n in names for p in (5, 30)], natural)


def repeats(side, both):
    """sorted lines with runs of equal lines on one side (file 1) or on both"""
    s = []
    for p, k1, k2 in ((5, 3, 1), (6, 1, 1), (7, 2, 2), (8, 4, 0), (9, 1, 3), (10, 2, 5)):
        k = (k1 if side == 0 else k2) if both else (k1 if side == 0 else min(k2, 1))
        s += [rec(b"1", b"%d" % p, id_=b"r%d" % i) for i in range(k)]
    return s


def equal_not_same(side):
    """lines that compare equal under compareKeys but print different keys: POS 007 / 7 / 07, and with
    -n the names 1 / chr1 / 01; a run is longer on one side, so some of them are printed"""
    if side == 0:
        return [rec(b"1", b"007"), rec(b"1", b"7"), rec(b"1", b"07"), rec(b"1", b"8"), rec(b"1", b"9"), rec(b"1", b"09")]
    return [rec(b"1", b"7"), rec(b"1", b"008"), rec(b"1", b"0008"), rec(b"1", b"9")]


def equal_not_same_natural(side):
    if side == 0:
        return [rec(b"1", b"5"), rec(b"chr1", b"5"), rec(b"01", b"5"), rec(b"CHR2", b"6")]
    return [rec(b"Chr1", b"5"), rec(b"2", b"6"), rec(b"chr2", b"6")]


def fixtures():
    rnd = random.Random(7)
    gen_a, gen_b = R.gen_lines(1, 60), R.gen_lines(2, 60)
    shuf = list(zoo(0, False))
    rnd.shuffle(shuf)
    fx = {
        "rules_a.vcf": text(rules(0)),
        "rules_b.vcf": text(rules(1)),
        "rules_a_crlf.vcf": text(rules(0)).replace(b"\n", b"\r\n"),
        "rules_b_crlf.vcf": text(rules(1)).replace(b"\n", b"\r\n"),
        "no_final_newline_a.vcf": text(rules(0) + [rec(b"9", b"1")], False),
        "no_final_newline_b.vcf": text(rules(1) + [rec(b"9", b"2")], False),
        "no_final_newline_header.vcf": text(rules(0) + [b"#end"], False),
        "empty.vcf": b"",
        "header_only.vcf": HDR,
        "only_newlines.vcf": b"\n\n\n",
        "one_a.vcf": HDR + rec(b"1", b"5") + b"\n",
        "one_b.vcf": HDR + rec(b"1", b"6") + b"\n",
        "collide_a.vcf": rec(b"1:5", b"", b"A", b"T") + b"\n",
        "collide_b.vcf": rec(b"1", b"5", b"", b"A:T") + b"\n",
        "alts_a.vcf": HDR + text(alts(0)),
        "alts_b.vcf": HDR + text(alts(1)),
        "longpos_a.vcf": HDR + rec(b"3", b"99999999999999999999999", b"G", b"A") + b"\n" + rec(b"3", b"0" * 30 + b"1") + b"\n",
        "longpos_b.vcf": HDR + rec(b"3", b"99999999999999999999999", b"G", b"A") + b"\n" + rec(b"3", b"1") + b"\n",
        "pos007_a.vcf": HDR + rec(b"1", b"007") + b"\n",
        "pos007_b.vcf": HDR + rec(b"1", b"7") + b"\n",
        "zoo_lex_a.vcf": HDR + text(zoo(0, False)),
        "zoo_lex_b.vcf": HDR + text(zoo(1, False)),
        "zoo_nat_a.vcf": HDR + text(zoo(0, True)),
        "zoo_nat_b.vcf": HDR + text(zoo(1, True)),
        "zoo_shuffled.vcf": HDR + text(shuf),
        "repeats_one_a.vcf": HDR + text(repeats(0, False)),
        "repeats_one_b.vcf": HDR + text(repeats(1, False)),
        "repeats_both_a.vcf": HDR + text(repeats(0, True)),
        "repeats_both_b.vcf": HDR + text(repeats(1, True)),
        "equal_a.vcf": HDR + text(equal_not_same(0)),
        "equal_b.vcf": HDR + text(equal_not_same(1)),
        "equal_nat_a.vcf": HDR + text(equal_not_same_natural(0)),
        "equal_nat_b.vcf": HDR + text(equal_not_same_natural(1)),
        "gen_a.vcf": HDR + text(gen_a),
        "gen_b.vcf": HDR + text(gen_b),
        "gen_sorted_a.vcf": HDR + text(ordered(gen_a)),
        "gen_sorted_b.vcf": HDR + text(ordered(gen_b)),
        "gen_sorted_nat_a.vcf": HDR + text(ordered(gen_a, True)),
        "gen_sorted_nat_b.vcf": HDR + text(ordered(gen_b, True)),
    }
    fx["rules_a.vcf.gz"] = gzip.compress(fx["rules_a.vcf"], mtime=0)
    fx["rules_b.vcf.gz"] = gzip.compress(fx["rules_b.vcf"], mtime=0)
    return fx


def build_cases():
    cases = []

    def p(fx):
        return DIR + "/" + fx

    def add(name, args, env=None):
        assert name not in {c["name"] for c in cases}, name
        cases.append({"name": name, "argv": [TOOL] + args, "env": env or {}})

    def pair(name, a, b, modes=("", "s", "sn")):
        for m in modes:
            add("%s__%s" % (name, m or "default"), ["-a", p(a), "-b", p(b)] + (["-" + m] if m else []))

    pair("rules", "rules_a.vcf", "rules_b.vcf")
    pair("rules_swapped", "rules_b.vcf", "rules_a.vcf")
    pair("rules_crlf", "rules_a_crlf.vcf", "rules_b_crlf.vcf")
    pair("rules_crlf_against_lf", "rules_a_crlf.vcf", "rules_a.vcf", ("", "s"))
    pair("no_final_newline_first", "no_final_newline_a.vcf", "rules_b.vcf")
    pair("no_final_newline_second", "rules_a.vcf", "no_final_newline_b.vcf")
    pair("no_final_newline_both", "no_final_newline_a.vcf", "no_final_newline_b.vcf")
    pair("no_final_newline_header", "no_final_newline_header.vcf", "one_a.vcf", ("", "s"))
    pair("empty_both", "empty.vcf", "empty.vcf", ("", "s"))
    pair("empty_first", "empty.vcf", "one_a.vcf", ("", "s"))
    pair("empty_second", "one_a.vcf", "empty.vcf", ("", "s"))
    pair("header_only_both", "header_only.vcf", "header_only.vcf", ("", "s"))
    pair("header_only_first", "header_only.vcf", "rules_b.vcf", ("", "s"))
    pair("only_newlines", "only_newlines.vcf", "one_b.vcf", ("", "sn"))
    pair("same_path_twice", "rules_a.vcf", "rules_a.vcf")
    pair("identical_files", "pos007_a.vcf", "pos007_a.vcf", ("", "s"))
    pair("one_each", "one_a.vcf", "one_b.vcf")
    pair("one_each_swapped", "one_b.vcf", "one_a.vcf", ("", "s"))
    pair("collide", "collide_a.vcf", "collide_b.vcf")
    pair("alts", "alts_a.vcf", "alts_b.vcf")
    pair("pos007", "pos007_a.vcf", "pos007_b.vcf")
    pair("longpos", "longpos_a.vcf", "longpos_b.vcf", ("",))  # (POS is only text in the default mode)
    pair("zoo_lex", "zoo_lex_a.vcf", "zoo_lex_b.vcf", ("", "s"))
    pair("zoo_nat", "zoo_nat_a.vcf", "zoo_nat_b.vcf", ("", "sn"))
    pair("zoo_lex_files_in_natural_order", "zoo_lex_a.vcf", "zoo_lex_b.vcf", ("sn",))
    pair("zoo_nat_files_in_byte_order", "zoo_nat_a.vcf", "zoo_nat_b.vcf", ("s",))
    pair("zoo_unsorted_first", "zoo_shuffled.vcf", "zoo_lex_b.vcf", ("", "s", "sn"))
    pair("zoo_unsorted_second", "zoo_nat_a.vcf", "zoo_shuffled.vcf", ("s", "sn"))
    pair("repeats_one", "repeats_one_a.vcf", "repeats_one_b.vcf")
    pair("repeats_both", "repeats_both_a.vcf", "repeats_both_b.vcf")
    pair("repeats_both_swapped", "repeats_both_b.vcf", "repeats_both_a.vcf", ("s", "sn"))
    pair("equal_not_same", "equal_a.vcf", "equal_b.vcf")
    pair("equal_not_same_natural", "equal_nat_a.vcf", "equal_nat_b.vcf")
    pair("gen_unsorted_both", "gen_a.vcf", "gen_b.vcf")
    pair("gen_unsorted_first", "gen_a.vcf", "gen_sorted_b.vcf", ("s", "sn"))
    pair("gen_unsorted_second", "gen_sorted_a.vcf", "gen_b.vcf", ("s",))
    pair("gen_sorted", "gen_sorted_a.vcf", "gen_sorted_b.vcf", ("", "s"))
    pair("gen_sorted_nat", "gen_sorted_nat_a.vcf", "gen_sorted_nat_b.vcf", ("sn",))
    # the reference reads compressed bytes as text: the drop-in does with VCFX_GZIP=0
    for m in ("", "s"):
        add("gz_pair_as_text__%s" % (m or "default"), ["-a", p("rules_a.vcf.gz"), "-b", p("rules_b.vcf.gz")] + (["-" + m] if m else []),
            env={"VCFX_GZIP": "0"})
    a, b = p("rules_a.vcf"), p("rules_b.vcf")
    add("long_options", ["--file1", a, "--file2", b, "--assume-sorted", "--natural-chr", "--quiet"])
    add("long_options_joined", ["--file1=" + a, "--file2=" + b])
    add("long_prefixes", ["--file1", a, "--file2", b, "--assume", "--nat", "--qu"])
    add("short_joined", ["-a" + a, "-b" + b, "-sq"])
    add("quiet_default", ["-q", "-a", a, "-b", b])
    add("options_after_operands", ["stray", "-a", a, "operand", "-b", b])
    add("double_dash", ["-a", a, "-b", b, "--", "-s"])
    add("last_file_wins", ["-a", p("one_a.vcf"), "-a", a, "-b", p("one_b.vcf"), "-b", b])
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_files", ["-a", a, "-b", b, "--help"])
    add("help_as_a_value", ["-a", "-h", "-b", b])
    add("help_in_group", ["-sh", "-a", a, "-b", b])
    add("help_prefix", ["--he", "-a", a, "-b", b])
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("version_with_files", ["-a", a, "-b", b, "-v"])
    add("no_arguments", [])
    add("missing_file1_option", ["-b", b])
    add("missing_file2_option", ["-a", a])
    add("empty_file1_value", ["-a", "", "-b", b])
    add("only_operands", [a, b])
    add("bad_long", ["--bogus", "-a", a, "-b", b])
    add("bad_short", ["-a", a, "-b", b, "-x"])
    add("ambiguous_long", ["--file", a, "-b", b])
    add("missing_argument", ["-a", a, "-b"])
    add("missing_argument_long", ["--file1"])
    add("flag_with_value", ["--assume-sorted=1", "-a", a, "-b", b])
    add("missing_first", ["-a", p("does_not_exist.vcf"), "-b", b])
    add("missing_second", ["-a", a, "-b", p("does_not_exist.vcf")])
    add("missing_both", ["-a", p("does_not_exist_1.vcf"), "-b", p("does_not_exist_2.vcf")])
    add("missing_first_sorted", ["-s", "-a", p("does_not_exist.vcf"), "-b", b])
    add("directory_first", ["-a", DIR, "-b", b])
    add("directory_second", ["-a", a, "-b", DIR, "-s"])
    return cases


def is_ordered(case, stdout):
    """every -s case, and every case whose sections hold at most one key each"""
    opts, _ = R.getopt_long(case["argv"])
    if any(k == "s" for k, _, _ in opts):
        return True
    sec = R.sections(stdout)
    return sec is None or (len(sec[1]) <= 1 and len(sec[3]) <= 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_diff_tool executable")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    os.makedirs(os.path.join(HERE, DIR), exist_ok=True)
    for name, data in fixtures().items():
        with open(os.path.join(HERE, DIR, name), "wb") as f:
            f.write(data)
    out = []
    for c in build_cases():
        r = subprocess.run(c["argv"], executable=ref, input=b"", capture_output=True, cwd=HERE, timeout=120)
        c["rc"] = r.returncode
        c["ordered"] = is_ordered(c, r.stdout)
        c["stdout"] = base64.b64encode(r.stdout).decode()
        c["stderr"] = base64.b64encode(r.stderr).decode()
        out.append(c)
    n_ordered = sum(c["ordered"] for c in out)
    assert 3 * n_ordered >= len(out), (n_ordered, len(out))
    blob = json.dumps({"tool": TOOL, "cases": out}, indent=0, sort_keys=True).encode()
    path = os.path.join(HERE, "diff_tool_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases (%d ordered), %d bytes" % (len(out), n_ordered, os.path.getsize(path)))


if __name__ == "__main__":
    main()
