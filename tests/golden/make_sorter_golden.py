#!/usr/bin/env python3
"""Golden vectors of VCFX_sorter: runs the REFERENCE executable (--ref-bin PATH, built outside the
repository with the flags of oracle/Makefile.ref) over the small fixtures this script writes under
tests/golden/sorter/, in file, stdin, -n, -m, -t, two-file and help / version / error forms.

Writes tests/golden/sorter_cases.json.gz: per case the argv, the stdin fixture, the reference's
stdout, stderr (base64) and exit code, and `ties`.  The tool runs with cwd=tests/golden, relative
fixture paths and argv[0] = the tool's name, so the names it prints are stable.

The reference's sort is not stable (tests/_sorter_ref.py), so this script asserts a partition by
computing the keys itself: every sorted input either has no two kept lines with equal keys or has
at most 16 kept lines (ties = false: compared byte for byte), except the fixtures named ties_*,
which have at least 17 kept lines with runs of equal keys in both orders and both modes
(ties = true: compared by same_up_to_ties).  Outside the domain and in no fixture: a non-numeric
-m, an unwritable -t, a CHROM digit run or a stdin POS whose value overflows the reference's own
arithmetic in an undefined way.
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

from tests import _sorter_ref as R  # noqa: E402  (the fixture generators and the key, for the partition)

TOOL = R.TOOL
DIR = "sorter"
HDR = R.HDR
REST = b"A\tC\t50\tPASS\tDP=7"


def rec(chrom, pos, id_=b"."):
    return b"\t".join([chrom, pos, id_, REST])


def shuffled(seed, lines):
    lines = list(lines)
    random.Random(seed).shuffle(lines)
    return lines


def rules():
    """every line rule of the two modes, '#' and empty lines between the data"""
    s = [b"##fileformat=VCFv4.2", b"", b"9\t1\tbefore the header line", b"no tab before the header line",
         HDR.split(b"\n")[1], b"",
         rec(b"2", b"200", b"a"), b"#a comment between data lines", rec(b"1", b"300", b"b"), b"", b"",
         rec(b"10", b"5", b"c"), b"no_tab_at_all", rec(b"3", b"0", b"zero"), rec(b"3", b"-4", b"minus"),
         rec(b"3", b"+3", b"plus"), rec(b"3", b" 2", b"space"), rec(b"3", b"abc", b"letters"), rec(b"3", b"5abc", b"digits_then"),
         b"1\t7", b"1\t8\t", rec(b"4", b"4294967301", b"ten_digits_wraps_to_5"), rec(b"4", b"6", b"six"),
         rec(b"4", b"4", b"four"), rec(b"4", b"2147483648", b"wraps_negative"), rec(b"4", b"", b"empty_pos"),
         b"#CHROM again", b"##late meta line", rec(b"1", b"299", b"d"), b"\t", b" ", rec(b"1", b"0300", b"e")]
    return b"\n".join(s) + b"\n"


# every POS form std::stoi and the file mode's digit run tell apart, each on a CHROM of its own
POS_FORMS = [b"55", b" 56", b"\x0b\x0c\r 57", b"+58", b"-59", b"60abc", b"61 ", b"6 2", b"abc", b"", b" ", b"+", b"-",
             b"+-63", b"0", b"-0", b"007", b"0x10", b"1e3", b"2147483647", b"2147483648", b"-2147483648",
             b"-2147483649", b"4294967351", b"99999999999999999999", b"-99999999999999999999", b"1.5"]
POS_VALUES = [b"-2147483648", b"-4", b"0", b"3", b"12", b"2147483647", b"-1", b"100"]


def pos_forms():
    s = [HDR.rstrip(b"\n")]
    s += [rec(b"f%02d" % i, f, b"form%d" % i) for i, f in enumerate(POS_FORMS)]
    s += [rec(b"z", v, b"value%d" % i) for i, v in enumerate(POS_VALUES)]  # signed order inside one CHROM
    return b"\n".join(s[:1] + shuffled(3, s[1:])) + b"\n"


def empty_chrom():
    s = [HDR.rstrip(b"\n")] + shuffled(4, [rec(b"", b"5", b"e5"), rec(b"", b"3", b"e3"), rec(b"1", b"9", b"a"), rec(b"\x01", b"2", b"ctl"),
                                          rec(b"~", b"1", b"tilde"), rec(b"\xff", b"4", b"high"), rec(b"chr", b"8", b"bare_chr"),
                                          rec(b"CHR", b"6", b"bare_CHR"), rec(b"", b"7", b"e7"), rec(b"Y", b"1", b"y")])
    return b"\n".join(s) + b"\n"


NATURAL_NAMES = [b"1", b"2", b"10", b"22", b"23", b"0", b"9", b"chr1", b"Chr1", b"CHR1", b"cHr1", b"CHr1", b"chR1", b"chr2",
                 b"chr10", b"chr22", b"chr23", b"M", b"MT", b"X", b"Y", b"m", b"mt", b"x", b"y", b"chrM", b"chrMT", b"chrX",
                 b"chrY", b"CHRX", b"ChrY", b"chrm", b"MT_alt", b"MTx", b"Mx", b"XY", b"chrMT_random", b"2_random",
                 b"chr2_random", b"chr2_alt", b"1x", b"22abcdefghij", b"chrUn_gl000220", b"GL000220.1", b"KI270728.1",
                 b"chr", b"CHR", b"Chr", b"ch", b"c", b"chr0", b"chr01", b"001", b"HLA-A*01:01", b"\xc3\xa9", b"chr\xff"]
# names that share an id: the suffix hash reads 8 bytes, the hash of an unknown name 16
SAME_ID = [(b"1_abcdefgh1", b"1_abcdefgh2"), (b"chr7_gl0001_random", b"chr7_gl0001_alt"),
           (b"scaffold_0123456789", b"scaffold_0123456788x"), (b"chrMT_decoy001A", b"chrMT_decoy001B")]


def natural():
    s = []
    for i, c in enumerate(NATURAL_NAMES):
        s += [rec(c, b"%d" % (100 + i), b"n%da" % i), rec(c, b"%d" % (50 - (i % 7)), b"n%db" % i)]
    for i, (a, b) in enumerate(SAME_ID):
        assert R.chrom_to_id(a) == R.chrom_to_id(b), (a, b)
        s += [rec(a, b"30", b"s%da" % i), rec(b, b"20", b"s%db" % i), rec(a, b"10", b"s%dc" % i), rec(b, b"40", b"s%dd" % i)]
    return HDR + b"\n".join(shuffled(5, s)) + b"\n"


def chrom_lengths():
    """CHROM lengths 0, 1, 7, 8, 9, 16, 17 and 40; names equal in their first 8 and first 16 bytes;
    a prefix before its extensions; bytes >= 0x80"""
    b8 = b"ABCDEFGH"
    b16 = b8 + b"IJKLMNOP"
    b39 = b16 + b"QRSTUVWXYZ0123456789abc"
    assert len(b39) == 39
    names = [b"", b"A", b"B", b"ABCDEFG", b8, b8 + b"I", b8 + b"J", b8 + b"\x80", b16, b16 + b"Q", b16 + b"R",
             b16[:15] + b"\xf0", b39 + b"d", b39 + b"e", b39[:38] + b"\x80x", b"\x80", b"A\xff", b"\xc3\xa9", b"AB", b"ABCDEFGHI "]
    assert sorted({len(n) for n in names}) == [0, 1, 2, 7, 8, 9, 10, 16, 17, 40]
    s = []
    for i, c in enumerate(names):
        s += [rec(c, b"%d" % (200 + i), b"L%da" % i), rec(c, b"%d" % (100 - i), b"L%db" % i)]  # (names may share an id: no POS twice)
    return HDR + b"\n".join(shuffled(6, s)) + b"\n"


def ties(seed):
    """40 kept lines over few keys: runs of equal keys in both orders and both modes"""
    rnd = random.Random(seed)
    chroms = (b"1", b"2", b"chr1", b"M", b"MT", b"", b"1_abcdefgh1", b"1_abcdefgh2")
    s = [rec(rnd.choice(chroms), b"%d" % rnd.randrange(1, 4), b"t%d" % i) for i in range(40)]
    s.insert(20, b"#between")
    s.insert(10, b"")
    s.insert(5, b"1\t0\tdropped")
    return HDR + b"\n".join(s) + b"\n"


def fixtures():
    r = rules()
    return {
        "rules.vcf": r,
        "rules_crlf.vcf": r.replace(b"\n", b"\r\n"),
        "no_final_newline_kept.vcf": r + rec(b"0", b"1", b"last"),
        "no_final_newline_bad.vcf": r + b"tail",
        "no_final_newline_header.vcf": r + b"#end",
        "no_chrom_line.vcf": b"##only meta\n" + rec(b"1", b"5") + b"\n\n" + rec(b"1", b"3") + b"\nbad\n",
        "chrom_prefix_line.vcf": b"#CHROMOSOMES are listed below\n" + rec(b"2", b"5") + b"\n" + rec(b"1", b"3") + b"\n#CHRO\n",
        "pos_forms.vcf": pos_forms(),
        "empty_chrom.vcf": empty_chrom(),
        "natural.vcf": natural(),
        "chrom_lengths.vcf": chrom_lengths(),
        "generated.vcf": R.gen_vcf(41, 120, mix=True, pad=30),
        "generated_no_final_newline.vcf": R.gen_vcf(42, 60, mix=True, final_newline=False),
        "ties_a.vcf": ties(1),
        "ties_b.vcf": ties(2).replace(b"\n", b"\r\n"),
        "header_only.vcf": HDR,
        "only_newlines.vcf": b"\n\n\n",
        "one_line.vcf": rec(b"1", b"5") + b"\n",
        "one_line_no_header.vcf": b"#CHROM\n" + rec(b"1", b"5"),
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
        add("%s__file" % fx, [p(fx)])
        add("%s__stdin" % fx, [], stdin=p(fx))
        add("%s__natural_file" % fx, ["-n", p(fx)])
        add("%s__natural_stdin" % fx, ["--natural-chr"], stdin=p(fx))
    for fx in ("generated.vcf", "natural.vcf", "ties_a.vcf"):
        add("%s__m1_file" % fx, ["-m", "1", p(fx)])
        add("%s__m0_stdin" % fx, ["-m", "0"], stdin=p(fx))
        add("%s__m0_natural_stdin" % fx, ["-n", "--max-memory=0"], stdin=p(fx))
        add("%s__m1_stdin" % fx, ["-m1"], stdin=p(fx))
        add("%s__t_stdin" % fx, ["-t", "/tmp", "-m", "0"], stdin=p(fx))
        add("%s__t_file" % fx, ["--temp-dir", "/tmp", p(fx), "-n"])
    add("two_files", [p("rules.vcf"), p("chrom_lengths.vcf")])
    add("two_files_natural", ["-n", p("natural.vcf"), p("rules_crlf.vcf")])
    add("two_files_empty_first", [p("empty.vcf"), p("rules.vcf")])
    add("same_file_twice", [p("generated.vcf"), p("generated.vcf")])
    add("second_file_missing", [p("rules.vcf"), p("does_not_exist.vcf"), p("natural.vcf")])
    add("missing_file", [p("does_not_exist.vcf")])
    add("missing_file_natural", ["-n", p("does_not_exist.vcf")])
    add("option_after_file", [p("natural.vcf"), "-n"])
    add("prefix_of_long", ["--nat", p("natural.vcf")])
    add("double_dash", ["--", p("rules.vcf")])
    add("dash_is_a_file_name", ["-"], stdin=p("rules.vcf"))
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", [p("rules.vcf"), "--help"])
    add("help_in_group", ["-nh"], stdin=p("rules.vcf"))
    add("help_prefix", ["--he"], stdin=p("rules.vcf"))
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("bad_long", ["--bogus", p("rules.vcf")])
    add("bad_short", [p("rules.vcf"), "-x"])
    add("bad_short_stdin", ["-x"], stdin=p("rules.vcf"))
    add("missing_argument", ["-n", "-m"])
    add("missing_argument_long", ["--temp-dir"])
    add("natural_with_value", ["--natural-chr=1"], stdin=p("rules.vcf"))
    add("double_dash_stdin", ["--"], stdin=p("one_line.vcf"))
    return cases


def check_partition(case, fx):
    """ties = the case sorts a ties_* fixture; every other sorted input is free of equal keys among
    its kept lines or keeps at most 16"""
    stdin, natural = R.case_mode(case)
    opts, operands = R.getopt_long(case["argv"])
    if any(k in ("?", "h") for k, _, _ in opts) or "--help" in case["argv"] or "--version" in case["argv"] or \
            "-v" in case["argv"] or "-h" in case["argv"]:
        return False
    names = [case["stdin"]] if stdin else operands
    flags = set()
    for name in names:
        base = os.path.basename(name or "")
        if base not in fx:
            continue  # (a missing file)
        kept, tied = R.tie_profile(fx[base], stdin, natural)
        if base.startswith("ties_"):
            assert kept >= 17 and tied >= 10, (case["name"], kept, tied)
            flags.add(True)
        else:
            assert tied == 0 or kept <= 16, (case["name"], base, kept, tied)
            flags.add(False)
    assert len(flags) <= 1, case["name"]
    return bool(flags and flags.pop())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_sorter executable")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    os.makedirs(os.path.join(HERE, DIR), exist_ok=True)
    fx = fixtures()
    for name, data in fx.items():
        with open(os.path.join(HERE, DIR, name), "wb") as f:
            f.write(data)
    out = []
    for c in build_cases():
        stdin = b""
        if c["stdin"]:
            with open(os.path.join(HERE, c["stdin"]), "rb") as f:
                stdin = f.read()
        c["ties"] = check_partition(c, fx)
        r = subprocess.run(c["argv"], executable=ref, input=stdin, capture_output=True, cwd=HERE, timeout=120)
        c["rc"] = r.returncode
        c["stdout"] = base64.b64encode(r.stdout).decode()
        c["stderr"] = base64.b64encode(r.stderr).decode()
        out.append(c)
    blob = json.dumps({"tool": TOOL, "cases": out}, indent=0, sort_keys=True).encode()
    path = os.path.join(HERE, "sorter_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases (%d up to ties), %d bytes" % (len(out), sum(c["ties"] for c in out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
