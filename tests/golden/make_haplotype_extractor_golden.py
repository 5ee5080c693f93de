#!/usr/bin/env python3
"""Records VCFX_haplotype_extractor's goldens from the compiled reference tool.

    python tests/golden/make_haplotype_extractor_golden.py --ref-bin PATH/VCFX_haplotype_extractor

The executable is built outside the repository from the reference's own sources with the flags of
oracle/Makefile.ref (C++17, -O3 -DNDEBUG, VCFX_VERSION="1.1.4").  Writes the data-only fixtures under
tests/golden/haplotype_extractor/ and tests/golden/haplotype_extractor_cases.json.gz: per case argv,
the stdin fixture, and the reference's stdout, stderr and exit code.  Cases run with cwd tests/golden.

Outside the domain, and in no case here: a POS above 2147483647 or a difference of two POS values that
does not fit an int (the reference's int overflows); a NUL byte in the input; a line of 2 GiB or
more; a -b value that std::stoi rejects (the reference dies on the uncaught exception); a negative -b
value on an input that holds a member (the reference dies of std::length_error in its first reserve).
"""
import argparse
import base64
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _haplotype_extractor_ref as R  # noqa: E402

TOOL = R.TOOL
DIR = "haplotype_extractor"


def vcf(lines, eol=b"\n", final=True):
    return eol.join(lines) + (eol if final else b"")


def fixtures():
    rec, H2, H3 = R.record, R.chrom_line(2), R.chrom_line(3)
    meta = b"##fileformat=VCFv4.2"
    ph = [b"0|1", b"1|0"]
    statuses = [meta, H2,
                rec(b"1", 100, ph), rec(b"1", 200, ph),
                b"", b"#comment", b"1\t5\t.\tA\tC", b"1\t5\t.\tA\tC\t.\t.\t.\tGT", b"1\tx5\t.\tA\tC\t.\t.\t.\tGT\t0|1\t0|1",
                b"1\t5 \t.\tA\tC\t.\t.\t.\tGT\t0|1\t0|1", b"1\t-5\t.\tA\tC\t.\t.\t.\tGT\t0|1\t0|1",
                rec(b"1", 250, ph, b"AD:DP"), rec(b"1", 260, [b"0/1", b"0|1"]), rec(b"1", 270, [b"0|1", b"0/1"]),
                rec(b"1", 300, ph),
                b"1\t\t.\tA\tC\t.\t.\t.\tGT\t0|1\t1|1",        # an empty POS is 0
                b"1\t00310\t.\tA\tC\t.\t.\t.\tGT\t0|1\t1|1",   # leading zeros
                rec(b"1", 320, [b"0|1"]),                       # ragged: a sample missing
                b"1\t330\t.\tA\tC\t.\t.\t.\tGT\t0|1\t",         # ... and an empty one
                rec(b"1", 340, ph, extra=[b"0/1", b"junk"]),    # over-long: the extra fields are ignored
                H3, b"#CHROM",                                  # later "#CHROM" lines are ignored
                rec(b"1", 350, ph)]
    formats = [H2,
               rec(b"1", 100, ph, b"GT"), rec(b"1", 110, ph, b"GT:AD:DP"), rec(b"1", 120, ph, b"AD:GT:DP"),
               rec(b"1", 130, ph, b"AD:DP:GT"), rec(b"1", 140, ph, b"AD:DP"), rec(b"1", 150, ph, b"GTX:GT"),
               rec(b"1", 160, ph, b"XGT"), rec(b"1", 170, ph, b""), rec(b"1", 180, ph, b"gt"),
               b"1\t190\t.\tA\tC\t.\t.\t.\tAD:GT\t5:0|1\t5",        # the GT sub-field missing
               b"1\t200\t.\tA\tC\t.\t.\t.\tAD:GT\t5:0|1\t5:",       # ... and empty
               b"1\t210\t.\tA\tC\t.\t.\t.\tAD:GT:DP\t5:0|1:3\t5::3",
               rec(b"1", 220, ph, b"GT:GT")]
    gts = [H3,
           rec(b"1", 100, [b"|", b".|.", b"10|2"]), rec(b"1", 110, [b"0|1|1", R.LONG_GT, b"0|1"]),
           rec(b"1", 120, [b"|", b"|1", b"1|"]), rec(b"1", 130, [b"0|1", b"", b"0|1"]),
           rec(b"1", 140, [b"0|1", b".", b"0|1"]), rec(b"1", 150, [b"||", b"a|b", b"0|1/2"]),
           rec(b"2", 150, [b"0|1", b"0|1", b"0|1"])]
    T = 100000
    dist = [H2, rec(b"1", 1000, ph), rec(b"1", 1000 + T, ph), rec(b"1", 1001 + 2 * T, ph), rec(b"1", 1001 + 2 * T, ph),
            rec(b"1", 500, ph), rec(b"1", 400, ph),                    # a falling POS extends; END falls
            rec(b"2", 400, ph), rec(b"1", 400, ph), rec(b"1 ", 400, ph),  # a CHROM change at equal POS
            rec(b"1 ", 450, ph), rec(b"1 ", 460, ph)]
    f01, f10 = b"0|1", b"1|0"
    flips = [H3,
             rec(b"1", 100, [f01, f01, f01]), rec(b"1", 110, [f10, f01, f01]),   # a flip in the first sample
             rec(b"1", 120, [f10, f01, f01]), rec(b"1", 130, [f10, f01, f10]),   # ... and in the last
             rec(b"1", 140, [f10, f10, f01]),                                    # two at once: the first is named
             rec(b"1", 150, [b"1|", b"1|0", b"0|1"]), rec(b"1", 160, [b"|1", b"1|0", b"0|1"]),  # hidden by a short GT
             rec(b"1", 170, [b"0|0|1", f10, f01]), rec(b"1", 180, [b"1|1|0", f10, f01]),  # polyploid: first and last byte
             rec(b"1", 190, [b"1|0|0", f10, f01]),                               # 1..0 after 1..0: no flip
             rec(b"1", 200, [b"0|2", b"0|0", b"1|1"]), rec(b"1", 210, [b"2|1", b"1|1", b"0|0"]),  # not a swap
             b"#between", b"short", rec(b"1", 215, [b"0/1"] * 3),
             rec(b"1", 220, [b"1|2", b"1|1", b"0|0"]),                           # a flip across non-members
             rec(b"2", 220, [b"2|1", b"1|1", b"0|0"]),                           # a would-be flip on another CHROM
             rec(b"2", 900000, [b"1|2", b"1|1", b"0|0"])]                        # ... and beyond the distance
    small = [meta, H2, rec(b"1", 100, ph), rec(b"1", 110, [b"1|0", b"1|0"]), rec(b"1", 120, [b"|", b"0|1"]),
             rec(b"1", 130, [b"1|0", b"0|1"])]
    crlf = [meta, H2, rec(b"1", 100, ph), b"", rec(b"1", 110, ph), b"1\t5", rec(b"2", 110, ph)]
    fx = {
        "statuses.vcf": vcf(statuses),
        "formats.vcf": vcf(formats),
        "gts.vcf": vcf(gts),
        "distance.vcf": vcf(dist),
        "flips.vcf": vcf(flips),
        "small.vcf": vcf(small),
        "crlf.vcf": vcf(crlf, b"\r\n"),
        "cr_only_line.vcf": vcf([meta, H2, rec(b"1", 100, ph), b"\r", rec(b"1", 110, ph), b"\r"]),
        "cr_only_first.vcf": vcf([b"\r", meta, H2, rec(b"1", 100, ph)]),
        "no_final_newline.vcf": vcf(small, final=False),
        "no_final_newline_crlf.vcf": vcf(small, b"\r\n", final=False),
        "header_only.vcf": vcf([meta, H2]),
        "no_header.vcf": vcf([meta, b"#other"]),
        "only_newlines.vcf": b"\n\n\n",
        "no_samples.vcf": vcf([meta, R.COLS, rec(b"1", 100, ph)]),
        "no_samples_tab.vcf": vcf([meta, R.COLS + b"\t", rec(b"1", 100, ph)]),
        "data_first.vcf": vcf([meta, rec(b"1", 100, ph), H2, rec(b"1", 110, ph)]),
        "one_sample.vcf": vcf([R.chrom_line(1), rec(b"1", 100, [b"0|1"]), rec(b"1", 110, [b"1|1"])]),
        "generated.vcf": R.gen_blocks(51, 5, [1, 3, 2, 7, 1], widths=(1, 3, 4, 5), between=0.4),
        "generated_fmt.vcf": R.gen_blocks(52, 3, [4, 1, 5], widths=(3, 5), fmt=b"AD:GT:DP", between=0.3),
        "generated_crlf.vcf": R.gen_blocks(53, 4, [2, 6, 1], widths=(3, 4, 300), between=0.3, crlf=True, final_newline=False),
        "no_members.vcf": vcf([meta, H2, rec(b"1", 100, [b"0/1", b"0|1"]), b"1\t5", rec(b"1", 120, ph, b"DP")]),
        "empty.vcf": b"",
    }
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
        add("%s__stdin" % name, [], stdin=p(name))
        add("%s__stream_file" % name, ["-s", p(name)])
        add("%s__stream_stdin" % name, ["--streaming"], stdin=p(name))
        add("%s__quiet_check_file" % name, ["-qc", "--input", p(name)])
        add("%s__check_stdin" % name, ["--check-phase-consistency"], stdin=p(name))
        add("%s__check_debug_file" % name, ["-c", "-d", "-i", p(name)])
    for name in ("small.vcf", "flips.vcf", "gts.vcf"):
        add("%s__check_debug_stdin" % name, ["-cd"], stdin=p(name))
        add("%s__check_debug_stream_quiet" % name, ["-c", "--debug", "-s", "-q", "-i", p(name)])
        add("%s__debug_alone" % name, ["-d", "-i", p(name)])
    for b in ("0", "1", "10", "99999", "100000", "100001", "2147483647", " 7", "+10", "10x", "010"):
        add("block_%s" % b.strip().replace("-", "m").replace("+", "p"), ["-b", b, "-i", p("distance.vcf")])
    # (a negative value makes the reference reserve size_t(T) / 50 * 4 bytes per sample at its first member and
    # die of std::length_error: with a member in the input it is outside the domain)
    for b in ("-1", "-100000"):
        add("block_m%s_header_only" % b[1:], ["-b", b, "-i", p("header_only.vcf")])
        add("block_m%s_no_members" % b[1:], ["-c", "-b", b], stdin=p("no_members.vcf"))
    add("block_long_form", ["--block-size", "100001"], stdin=p("distance.vcf"))
    add("block_equals", ["--block-size=0", "-s"], stdin=p("distance.vcf"))
    add("block_attached", ["-b100001", p("distance.vcf")])
    add("block_last_wins", ["-b", "0", "-b", "100001", p("distance.vcf")])
    add("block_check_flips", ["-c", "-b", "5", "-d", "-i", p("flips.vcf")])
    add("i_wins_over_positional", ["-i", p("small.vcf"), p("gts.vcf")])
    add("last_i_wins", ["-i", p("gts.vcf"), "-i", p("small.vcf")])
    add("positional_before_q", [p("statuses.vcf"), "-q"])
    add("two_positionals", [p("small.vcf"), p("gts.vcf")])
    add("input_equals", ["--input=" + p("small.vcf")])
    add("attached_value", ["-qi" + p("statuses.vcf")])
    add("prefix_of_long", ["--inp", p("statuses.vcf"), "--qu", "--str", "--ch", "--de", "--bl", "5"])
    add("dash_is_a_file_name", ["-i", "-"], stdin=p("small.vcf"))
    add("double_dash", ["--", p("small.vcf")])
    add("empty_input_name", ["-i", ""], stdin=p("small.vcf"))
    add("missing_file", ["-i", p("does_not_exist.vcf")])
    add("missing_file_positional_stream", ["-s", p("does_not_exist.vcf")])
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", ["-i", p("small.vcf"), "--help"])
    add("help_in_group", ["-qh"], stdin=p("small.vcf"))
    add("help_prefix", ["--he"], stdin=p("small.vcf"))
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("bad_long", ["--bogus", "-i", p("small.vcf")])
    add("bad_short", ["-i", p("small.vcf"), "-x"])
    add("bad_short_stdin", ["-x"], stdin=p("small.vcf"))
    add("two_bad_options", ["-x", "-y", "--bogus"])
    add("missing_argument", ["-q", "-i"])
    add("missing_argument_b", ["-b"])
    add("missing_argument_long", ["--block-size"])
    add("quiet_with_value", ["--quiet=1"], stdin=p("small.vcf"))
    add("double_dash_alone", ["--"], stdin=p("small.vcf"))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_haplotype_extractor executable")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    os.makedirs(os.path.join(HERE, DIR), exist_ok=True)
    fx = fixtures()
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
        assert r.returncode in (0, 1), (c["name"], r.returncode)  # (a crash of the reference is outside the domain)
        c["rc"] = r.returncode
        c["stdout"] = base64.b64encode(r.stdout).decode()
        c["stderr"] = base64.b64encode(r.stderr).decode()
        out.append(c)
    blob = json.dumps({"tool": TOOL, "cases": out}, indent=0, sort_keys=True).encode()
    path = os.path.join(HERE, "haplotype_extractor_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
