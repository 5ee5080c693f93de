#!/usr/bin/env python3
"""Golden vectors of VCFX_merger: runs the REFERENCE executable (--ref-bin PATH, built outside the
repository with the flags of oracle/Makefile.ref) over the small fixtures this script writes under
tests/golden/merger/, in the default mode, -s, -n, -s -n and the help / version / error forms.

Writes tests/golden/merger_cases.json.gz: per case the argv, the environment it is recorded for (the
.vcf.gz file: VCFX_GZIP=0, the reference reads the compressed bytes as text), the reference's stdout,
stderr (base64) and exit code, and `ordered`.  The tool runs with cwd=tests/golden, relative fixture
paths and argv[0] = the tool's name, so the names it prints are stable.

The reference leaves equal keys to std::sort and to its heap; the drop-in is stable.  So ONLY cases
named ties_* may meet equal keys: this script computes the keys itself (tests/_merger_ref.py) and
asserts that in every other default-mode case no two kept lines have equal keys and that in every
other -s case no pop sees two equal least heads; those cases are `ordered` and compared byte for
byte.  ties_* cases (sorted inputs, or the default mode) are compared by same_under_ties().  They are
at most a fifth of the file-reading cases (asserted).
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

from tests import _merger_ref as R  # noqa: E402  (the generators and the keys)

TOOL = R.TOOL
DIR = "merger"
HDR = R.HDR
rec = R.rec

# the natural-order name zoo of make_sorter_golden.py, plus 1 / 01 and chr / Chr / CHR
NAMES = [b"1", b"2", b"10", b"22", b"23", b"0", b"9", b"chr1", b"Chr1", b"CHR1", b"cHr1", b"CHr1", b"chR1", b"chr2", b"chr10",
         b"chr22", b"M", b"MT", b"X", b"Y", b"x", b"chrM", b"chrX", b"CHRX", b"ChrY", b"MT_alt", b"2_random", b"chr2_random",
         b"1x", b"1a", b"01", b"001", b"chr01", b"chr", b"CHR", b"Chr", b"ch", b"c", b"", b"chr0", b"HLA-A*01:01", b"\xc3\xa9",
         b"chr\xff", b"GL000220.1", b"2a", b"2b", b"Chr2", b"Chr10", b"CHR2", b"chr2a", b"chrUn_KI270742v1",
         b"a_name_of_more_than_sixteen_bytes", b"a_name_of_more_than_sixteen_bytes_b", b"12345678", b"123456789", b"abcdefgh",
         b"abcdefghi", b"abcdefgh\x00", b"n\x00ul"]


def text(lines, final_newline=True):
    return b"\n".join(lines) + (b"\n" if final_newline and lines else b"")


def ordered(lines, natural=False):
    return sorted(lines, key=lambda l: R.sort_key(*R.parse(l)[1:], natural))


def rules():
    """every line rule; no two kept lines share (CHROM, POS)"""
    return [b"##fileformat=VCFv4.2", b"", HDR.split(b"\n")[1], rec(b"1", b"100"), b"#a comment between data lines",
            b"no_tab_at_all", b"1\t101", b"1\t102\t", b"1\t103\t.", b"\t\t", b"\t\t\t\t", b"\t9\t.", rec(b"", b"10"),
            rec(b"1", b""), b"", b"", b"\r", b"#\r", b"1\t106\t.\tA\tC\r", b"1\t107\r", b"1\t108\r\t.", b"1\t\r109\t.",
            b" 1\t110\t.", b"1 \t111\t.", rec(b"n\x00ul", b"4"), rec(b"\xff\xfe", b"4"), rec(b"\x80", b"4"), rec(b"1", b"99"),
            b"x" * 70, b"y" * 61 + b"\t5\t.", b"y" * 62 + b"\t5\t.", b"y" * 63 + b"\t5\t.", b"y" * 64 + b"\t5\t.", b"y" * 300 + b"\t5\t.",
            b"z\t" + b"0" * 70 + b"12\t.", b"z\t" + b" " * 70 + b"13\t.", b"z\t14" + b"q" * 80 + b"\t."]


def pos_forms():
    """every POS form std::stol takes or refuses, with distinct values"""
    forms = [b" 7", b"\v8", b"\f9", b"\r10", b" \r\v 11", b"+3", b"-5", b"0x10", b"5abc", b"0070", b"0" * 30 + b"12", b"", b"-",
             b"+", b"- 3", b"abc", b"9223372036854775808", b"9223372036854775807", b"-9223372036854775808",
             b"-9223372036854775809", b"1.5", b"+-3", b"--3", b" +4", b"-0" + b"0" * 25 + b"6", b"99999999999999999999", b"2 2",
             b"13\r", b".5", b"e3", b"-1"]
    return [HDR.split(b"\n")[1]] + [rec(b"p", f) for f in forms]


def zoo(natural, part, pos0):
    """the name zoo: name i at POS pos0 + i and 5000 + pos0 + i, part `part` of three, in the order's order"""
    lines = [rec(n, b"%d" % (p + i)) for i, n in enumerate(NAMES) for p in (pos0, 5000 + pos0)]
    return ordered(lines[part::3], natural)


def ties(side, natural):
    """sorted lines with runs of equal keys inside a file and across files (lines that differ in their tail)"""
    s = []
    for p, k in ((5, (3, 1, 2)), (6, (1, 1, 1)), (7, (2, 0, 2)), (8, (0, 4, 0)), (9, (1, 3, 1))):
        s += [rec(b"1", b"%d" % p, b";f%d_%d" % (side, i)) for i in range(k[side])]
    s += [rec(b"01" if side else b"1", b"20", b";n%d" % side), rec(b"chr1", b"007" if side else b"7", b";p%d" % side)]
    return ordered(s, natural)


def fixtures():
    rnd = random.Random(11)
    gen = R.gen_records(3, 90)
    shuf = zoo(False, 0, 200) + zoo(False, 1, 200)
    rnd.shuffle(shuf)
    one = HDR.split(b"\n")
    fx = {
        "rules.vcf": text(rules()),
        "rules_crlf.vcf": b"\r\n".join(rules()) + b"\r\n",
        "pos_forms.vcf": text(pos_forms()),
        "hdr_after_data.vcf": text([rec(b"3", b"30"), rec(b"3", b"10"), b"#only after the data"]),
        "nohdr_a.vcf": text([rec(b"4", b"40"), rec(b"4", b"44")]),
        "nohdr_b.vcf": text([rec(b"4", b"41"), b"", rec(b"5", b"1")]),
        "hdr_third.vcf": text([b"##third", one[1], rec(b"4", b"42"), b"#late", rec(b"4", b"43")]),
        "bad_before_header.vcf": text([b"malformed line", b"##after a malformed line", rec(b"6", b"60")]),
        "empty_around_header.vcf": text([b"", b"", b"##first", b"", one[1], b"", b"", rec(b"6", b"61"), b"", b"#late", rec(b"6", b"62")]),
        "hdr_other.vcf": text([b"##another header", b"#CHROM\tother", rec(b"6", b"63")]),
        "empty.vcf": b"",
        "header_only.vcf": HDR,
        "only_newlines.vcf": b"\n\n\n",
        "nofinal_kept.vcf": text([one[1], rec(b"7", b"70"), rec(b"7", b"72")], False),
        "nofinal_header.vcf": text([rec(b"7", b"71"), b"#a last line without its newline"], False),
        "nofinal_bad.vcf": text([rec(b"7", b"73"), b"7\t74"], False),
        "unsorted_a.vcf": text([one[1], rec(b"8", b"50"), rec(b"8", b"10"), rec(b"9", b"5"), rec(b"8", b"30"), rec(b"7", b"1")]),
        "unsorted_b.vcf": text([rec(b"8", b"40"), rec(b"8", b"20"), b"bad", rec(b"9", b"4"), rec(b"8", b"60")]),
        "unsorted_c.vcf": text([rec(b"8", b"45"), rec(b"9", b"1"), rec(b"8", b"15")]),
        "zoo_shuffled.vcf": text([one[1]] + shuf),
        "gen_unsorted.vcf": text([one[1]] + gen[60:]),
        "rules.vcf.gz": gzip.compress(text(rules()), mtime=0),
    }
    for part in range(3):
        fx["zoo_lex_%d.vcf" % part] = text(one[:2] + zoo(False, part, 100))
        fx["zoo_nat_%d.vcf" % part] = text(one[:2] + zoo(True, part, 100))
        fx["gen_lex_%d.vcf" % part] = text(one[:2] + ordered(gen[part:60:3], False))
        fx["gen_nat_%d.vcf" % part] = text(one[:2] + ordered(gen[part:60:3], True))
        fx["ties_lex_%d.vcf" % part] = text(one[:2] + ties(part, False))
        fx["ties_nat_%d.vcf" % part] = text(one[:2] + ties(part, True))
    big = [rec(b"1", b"5", b";a%d" % i) for i in range(20)], [rec(b"1", b"5", b";b%d" % i) for i in range(20)]
    fx["ties_run_a.vcf"] = text(one[:2] + big[0])
    fx["ties_run_b.vcf"] = text(big[1])
    return fx


MODES = ("", "s", "n", "sn")


def build_cases():
    cases = []

    def p(fx):
        return DIR + "/" + fx

    def add(name, args, env=None):
        assert name not in {c["name"] for c in cases}, name
        cases.append({"name": name, "argv": [TOOL] + args, "env": env or {}})

    def files(name, names, modes=MODES, env=None):
        for m in modes:
            add("%s__%s" % (name, m or "default"), ["-m", ",".join(n if n == DIR else p(n) for n in names)] + (["-" + m] if m else []), env)

    files("rules", ["rules.vcf"])
    files("rules_crlf", ["rules_crlf.vcf"], ("", "s"))
    files("pos_forms", ["pos_forms.vcf"])
    files("pos_forms_after_rules", ["rules.vcf", "pos_forms.vcf"], ("", "sn"))
    files("hdr_after_data", ["hdr_after_data.vcf"], ("", "s"))
    files("hdr_after_data_then_header", ["hdr_after_data.vcf", "hdr_third.vcf"], ("", "s"))
    files("hdr_third", ["nohdr_a.vcf", "nohdr_b.vcf", "hdr_third.vcf"])
    files("hdr_first_of_two", ["hdr_third.vcf", "hdr_other.vcf", "nohdr_a.vcf"], ("", "s"))
    files("bad_before_header", ["bad_before_header.vcf", "hdr_other.vcf"], ("", "s"))
    files("bad_before_header_alone", ["bad_before_header.vcf"], ("", "s"))
    files("empty_around_header", ["empty_around_header.vcf", "hdr_other.vcf"], ("", "s"))
    files("empty_files", ["empty.vcf", "empty.vcf"], ("", "s"))
    files("empty_first", ["empty.vcf", "hdr_third.vcf", "empty.vcf"], ("", "s"))
    files("header_only", ["header_only.vcf"], ("", "s"))
    files("header_only_twice", ["header_only.vcf", "header_only.vcf"], ("", "s"))
    files("header_only_then_data", ["header_only.vcf", "nohdr_a.vcf", "only_newlines.vcf", "nohdr_b.vcf"], ("", "s"))
    files("only_newlines", ["only_newlines.vcf"], ("", "s"))
    files("nofinal_first", ["nofinal_kept.vcf", "nohdr_a.vcf", "nohdr_b.vcf"], ("", "s"))
    files("nofinal_middle", ["nohdr_a.vcf", "nofinal_header.vcf", "nohdr_b.vcf"], ("", "s"))
    files("nofinal_last", ["nohdr_a.vcf", "nohdr_b.vcf", "nofinal_bad.vcf"], ("", "s"))
    files("nofinal_all", ["nofinal_kept.vcf", "nofinal_header.vcf", "nofinal_bad.vcf"], ("", "s", "n"))
    files("directory", [DIR, "nohdr_a.vcf"], ("", "s"))
    files("directory_only", [DIR], ("", "s"))
    files("missing_middle", ["nohdr_a.vcf", "does_not_exist.vcf", "hdr_third.vcf"], ("", "s"))
    files("missing_all", ["does_not_exist_1.vcf", "does_not_exist_2.vcf"], ("", "s"))
    files("bad_lines_in_two_files", ["rules.vcf", "does_not_exist.vcf", "nofinal_bad.vcf", "bad_before_header.vcf"], ("", "s"))
    files("unsorted", ["unsorted_a.vcf", "unsorted_b.vcf", "unsorted_c.vcf"])
    files("unsorted_one", ["unsorted_b.vcf"], ("", "s"))
    files("unsorted_with_sorted", ["gen_lex_0.vcf", "gen_unsorted.vcf", "gen_lex_1.vcf"], ("s", "sn"))
    files("zoo_lex", ["zoo_lex_0.vcf", "zoo_lex_1.vcf", "zoo_lex_2.vcf"], ("", "s"))
    files("zoo_nat", ["zoo_nat_0.vcf", "zoo_nat_1.vcf", "zoo_nat_2.vcf"], ("n", "sn"))
    files("zoo_lex_files_in_natural_order", ["zoo_lex_0.vcf", "zoo_lex_1.vcf", "zoo_lex_2.vcf"], ("sn",))
    files("zoo_nat_files_in_byte_order", ["zoo_nat_2.vcf", "zoo_nat_0.vcf"], ("s",))
    files("zoo_shuffled", ["zoo_shuffled.vcf", "zoo_lex_2.vcf"])
    files("gen_lex", ["gen_lex_0.vcf", "gen_lex_1.vcf", "gen_lex_2.vcf"], ("", "s"))
    files("gen_nat", ["gen_nat_2.vcf", "gen_nat_1.vcf", "gen_nat_0.vcf"], ("n", "sn"))
    files("gen_all_unsorted_mode", ["gen_unsorted.vcf", "gen_nat_0.vcf", "gen_lex_1.vcf", "gen_lex_2.vcf"], ("", "n"))
    files("gz_as_text", ["rules.vcf.gz", "nohdr_a.vcf"], ("", "s"), env={"VCFX_GZIP": "0"})
    files("ties_lex", ["ties_lex_0.vcf", "ties_lex_1.vcf", "ties_lex_2.vcf"], ("", "s"))
    files("ties_nat", ["ties_nat_0.vcf", "ties_nat_1.vcf", "ties_nat_2.vcf"], ("n", "sn"))
    files("ties_run_of_forty", ["ties_run_a.vcf", "ties_run_b.vcf"], ("", "s"))
    files("ties_same_path_twice", ["gen_lex_0.vcf", "gen_lex_0.vcf"], ("", "s"))
    a, b = p("nohdr_a.vcf"), p("hdr_third.vcf")
    add("long_options", ["--merge", a + "," + b, "--assume-sorted", "--natural-chr"])
    add("long_option_joined", ["--merge=" + a + "," + b])
    add("long_prefixes", ["--mer", a, "--assume", "--nat"])
    add("short_joined", ["-sm" + a + "," + b])
    add("short_group", ["-ns", "-m", b])
    add("two_merge_options_add_up", ["-m", a, "-m", b])
    add("two_merge_options_mixed", ["--merge", b, "-s", "-m" + a])
    add("empty_names", ["-m", a + ",," + b])
    add("empty_name_only", ["-m", ""])
    add("only_commas", ["-m", ",,", "-s"])
    add("trailing_comma", ["-m", a + ","])
    add("options_after_operands", ["stray", "-m", a, "operand", "-s"])
    add("double_dash", ["-m", a, "--", "-s", "-m", b])
    add("operand_files_are_ignored", ["-m", a, b])
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_files", ["-m", a, "--help"])
    add("help_as_a_value", ["-m", "-h"])
    add("help_in_group", ["-sh", "-m", a])
    add("help_prefix", ["--he", "-m", a])
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("version_with_files", ["-m", a, "-v"])
    add("no_arguments", [])
    add("no_merge_option", ["-s", "-n"])
    add("only_operands", [a, b])
    add("bad_long", ["--bogus", "-m", a])
    add("bad_short", ["-m", a, "-x"])
    add("unknown_prefix", ["--sorted", "-m", a])
    add("missing_argument", ["-s", "-m"])
    add("missing_argument_long", ["--merge"])
    add("flag_with_value", ["--assume-sorted=1", "-m", a])
    return cases


def raw_files(case):
    """(the opened files' bytes as the REFERENCE reads them, -s, -n), None when the case reads no file"""
    argv = case["argv"]
    if any(x in argv[1:] for x in ("--help", "-h", "--version", "-v")):
        return None
    opts, _ = R.getopt_long(argv)
    letters = [k for k, _, _ in opts]
    names = R.split_names([v for k, v, _ in opts if k == "m"])
    if "h" in letters or "?" in letters or not names:
        return None
    data = []
    for n in names:
        full = os.path.join(HERE, n)
        if n and os.path.isdir(full):
            data.append(b"")
        elif os.path.isfile(full):
            data.append(open(full, "rb").read())
    return data, "s" in letters, "n" in letters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_merger executable")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    os.makedirs(os.path.join(HERE, DIR), exist_ok=True)
    for name, data in fixtures().items():
        with open(os.path.join(HERE, DIR, name), "wb") as f:
            f.write(data)
    out, reading, tied = [], 0, 0
    for c in build_cases():
        r = subprocess.run(c["argv"], executable=ref, input=b"", capture_output=True, cwd=HERE, timeout=120)
        c["rc"] = r.returncode
        c["ordered"] = not c["name"].startswith("ties_")
        raw = raw_files(c)
        if raw is not None:
            reading += 1
            m = R.merge(*raw)
            if c["ordered"]:
                assert not m.ties, c["name"]  # only ties_* cases may meet equal keys
            else:
                tied += 1
                assert m.ties and m.path == R.PATH_SORT, c["name"]  # (and those are sorted inputs or the default mode)
        else:
            assert c["ordered"]
        c["stdout"] = base64.b64encode(r.stdout).decode()
        c["stderr"] = base64.b64encode(r.stderr).decode()
        out.append(c)
    assert 5 * tied <= reading, (tied, reading)
    blob = json.dumps({"tool": TOOL, "cases": out}, indent=0, sort_keys=True).encode()
    path = os.path.join(HERE, "merger_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases (%d read files, %d of them ties_*), %d bytes" % (len(out), reading, tied, os.path.getsize(path)))


if __name__ == "__main__":
    main()
