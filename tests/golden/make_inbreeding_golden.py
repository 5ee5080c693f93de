#!/usr/bin/env python3
"""Golden vectors of VCFX_inbreeding_calculator: runs the REFERENCE executable (--ref-bin PATH,
built outside the repository with the flags of oracle/Makefile.ref) over the small fixtures
this script writes under tests/golden/inbreeding/, in file, positional-file and stdin mode.

Writes tests/golden/inbreeding_cases.json.gz: per case the argv, the input file or the stdin
fixture, and the reference's stdout, stderr (base64) and exit code.  The tool runs with
cwd=tests/golden and relative fixture paths, so the file names it prints are stable.  The
synthetic cases store the generator's parameters and the reference's stdout, not the input.
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

from tests import _inbreeding_ref as R  # noqa: E402  (the fixture generator only)

TOOL = "VCFX_inbreeding_calculator"
FLAGS = {
    "default": [],
    "global": ["--freq-mode", "global"],
    "skip": ["--skip-boundary"],
    "skipcount": ["--skip-boundary", "--count-boundary-as-used"],
    "globalskip": ["--freq-mode", "global", "--skip-boundary"],
}
HDR = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"


def rec(pos, gts, alt=b"T", fmt=b"GT", tail=b""):
    return b"\t".join([b"1", b"%d" % pos, b".", b"A", alt, b".", b"PASS", b".", fmt] + list(gts)) + tail


def hand_built():
    """short records (the first one too), a line ending in a tab, multi-allelic and empty ALT,
    the odd genotype fields, a record with fewer than two calls between short ones"""
    s = [b"##fileformat=VCFv4.2", HDR + b"\tA\tB\tC\tD\tE\tF"]
    s.append(rec(100, [b"0/1", b"1/1"]))                                    # short first record
    s.append(rec(101, [b"0/0", b"0/1", b"1/1", b"0/1", b"0/0", b"1/1"]))
    s.append(rec(102, [b"0/1", b"0/0", b"0/1"]))                            # the tail keeps record 101's codes
    s.append(rec(103, [b"./.", b".", b"0/.", b"./1", b"2/1", b"0/1/1"]))    # one call: parsed, not used
    s.append(rec(104, [b"0/0", b"0/1"]))                                    # the tail keeps record 103's codes
    s.append(rec(105, [b" 0/1", b"1|0:5", b"0/1x", b"10/0", b"01/1", b"0|0"]))
    s.append(rec(106, [b"0/1", b"1/1", b"0/0", b"0/0"], tail=b"\t"))        # a line ending in a tab
    s.append(rec(107, [b"0/1", b"1/1", b"0/0", b"0/0", b"0/1", b"1/1"], alt=b"T,G"))
    s.append(rec(108, [b"1/1", b"1/1", b"0/0", b"0/0", b"0/1", b"1/1"], alt=b""))
    s.append(rec(109, []))                                                  # nine fields
    s.append(rec(110, [], tail=b"\t"))                                      # nine fields and a tab
    s.append(rec(111, [b"0/0"] * 6))                                        # boundary frequency 0
    s.append(rec(112, [b"1/1"] * 6))                                        # boundary frequency 1
    s.append(rec(113, [b"0/1", b"0/0", b"0/0", b"0/0", b"0/0", b"0/0"]))    # a boundary for one sample only
    s.append(rec(114, [b"0/1:3", b"1/1:4", b"0|0:9", b"1|0:.", b".:.", b"0/0:1"], fmt=b"GT:DP"))
    s.append(rec(115, [b"0/1", b"1/1", b"0/0", b"0/0", b"0/1", b"1/1", b"0/1", b"0/1"]))  # more columns than samples
    s.append(rec(116, [b"1/1", b"", b"0/1"]))                               # an empty column
    return b"\n".join(s) + b"\n"


def basic():
    return R.ragged_vcf(11, 60, 7, odd=0.05, short=0.0, junk=0.0)


def fixtures():
    hb = hand_built()
    lines = hb.split(b"\n")
    return {
        "hand.vcf": hb,
        "basic.vcf": basic(),
        "ragged_a.vcf": R.ragged_vcf(21, 80, 5),
        "ragged_b.vcf": R.ragged_vcf(22, 120, 20),
        "crlf.vcf": R.ragged_vcf(23, 60, 6, crlf=True),
        "hand_crlf.vcf": hb.replace(b"\n", b"\r\n"),
        "hash_inside.vcf": b"\n".join(lines[:5] + [b"#a comment", b"", b"##another", HDR + b"\tX\tY"] + lines[5:]),
        "two_chrom.vcf": b"\n".join([lines[0], HDR + b"\tP\tQ", lines[1]] + lines[2:]),
        "data_before_chrom.vcf": b"\n".join([lines[0], lines[3], lines[4], lines[1]] + lines[2:]),
        "no_chrom.vcf": b"\n".join([lines[0]] + lines[2:]),
        "no_samples.vcf": b"\n".join([lines[0], HDR] + lines[2:]),
        "no_usable.vcf": b"\n".join([lines[0], lines[1], rec(1, [b"./."] * 6), rec(2, [b"0/1"] * 6, alt=b"T,G"),
                                     rec(3, [b"0/1", b"./.", b".", b".", b".", b"."])]) + b"\n",
        "header_only.vcf": b"\n".join(lines[:2]) + b"\n",
        "no_final_newline.vcf": hb[:-1],
        "empty.vcf": b"",
    }


def build_cases():
    cases = []

    def add(name, args, file=None, stdin=None, synth=None):
        cases.append({"name": name, "argv": [TOOL] + args, "file": file, "stdin": stdin, "synth": synth})

    for fx in ("hand.vcf", "basic.vcf", "ragged_a.vcf"):
        p = "inbreeding/" + fx
        for tag, fl in FLAGS.items():
            add("%s__%s__file" % (fx, tag), ["-i", p] + fl, file=p)
            add("%s__%s__pos" % (fx, tag), fl + [p], file=p)
            add("%s__%s__stdin" % (fx, tag), fl, stdin=p)
    for fx in ("ragged_b.vcf", "crlf.vcf", "hand_crlf.vcf", "hash_inside.vcf", "two_chrom.vcf", "data_before_chrom.vcf",
               "no_chrom.vcf", "no_samples.vcf", "no_usable.vcf", "header_only.vcf", "no_final_newline.vcf", "empty.vcf"):
        p = "inbreeding/" + fx
        add("%s__file" % fx, ["-i", p], file=p)
        add("%s__stdin" % fx, [], stdin=p)
        add("%s__quiet_file" % fx, ["-q", "--input", p], file=p)
        add("%s__quiet_stdin" % fx, ["--quiet"], stdin=p)
    add("hand__skip_global_quiet", ["-q", "-i", "inbreeding/hand.vcf", "--skip-boundary", "--freq-mode=global"],
        file="inbreeding/hand.vcf")
    add("missing_file", ["-i", "inbreeding/does_not_exist.vcf"])
    add("missing_file_quiet", ["-q", "inbreeding/does_not_exist.vcf"])
    add("bad_freq_mode_file", ["--freq-mode", "perSample", "-i", "inbreeding/basic.vcf"], file="inbreeding/basic.vcf")
    add("bad_freq_mode_stdin", ["--freq-mode", "GLOBAL", "--skip-boundary"], stdin="inbreeding/basic.vcf")
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", ["-i", "inbreeding/basic.vcf", "--help"])
    add("version", ["--version"])
    # synthetic inputs (vcfx_amd.synth.generate arguments): the reference's rows only
    for k, cfg in enumerate([(400, 130, 81, 0, 0.01, 0, 0.1, 0, 0), (300, 65, 82, 1, 0.05, 0, 0.3, 1, 0),
                             (200, 64, 83, 0, 0.002, 0, 0.0, 0, 1)]):
        for tag in ("default", "globalskip"):
            add("synth%d__%s__file" % (k, tag), ["-q", "-i", "synth.vcf"] + FLAGS[tag], synth=list(cfg))
            add("synth%d__%s__stdin" % (k, tag), FLAGS[tag], synth=list(cfg))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_inbreeding_calculator executable")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    os.makedirs(os.path.join(HERE, "inbreeding"), exist_ok=True)
    for name, data in fixtures().items():
        with open(os.path.join(HERE, "inbreeding", name), "wb") as f:
            f.write(data)
    out = []
    for c in build_cases():
        stdin, cwd, tmp = b"", HERE, None
        if c["synth"]:
            import tempfile
            from vcfx_amd import synth
            buf = synth.generate(*c["synth"][:8], format_mode=c["synth"][8])
            tmp = tempfile.mkdtemp()
            with open(os.path.join(tmp, "synth.vcf"), "wb") as f:
                f.write(buf)
            cwd = tmp
            if "-i" not in c["argv"]:
                stdin = buf
        elif c["stdin"]:
            with open(os.path.join(HERE, c["stdin"]), "rb") as f:
                stdin = f.read()
        r = subprocess.run([ref] + c["argv"][1:], input=stdin, capture_output=True, cwd=cwd, timeout=120)
        c["rc"] = r.returncode
        c["stdout"] = base64.b64encode(r.stdout).decode()
        c["stderr"] = base64.b64encode(r.stderr).decode()
        out.append(c)
        if tmp:
            os.remove(os.path.join(tmp, "synth.vcf"))
            os.rmdir(tmp)
    blob = json.dumps({"tool": TOOL, "cases": out}, indent=0, sort_keys=True).encode()
    with open(os.path.join(HERE, "inbreeding_cases.json.gz"), "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "inbreeding_cases.json.gz"))))


if __name__ == "__main__":
    main()
