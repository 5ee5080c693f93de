#!/usr/bin/env python3
"""Golden vectors of VCFX_multiallelic_splitter: runs the REFERENCE executable (--ref-bin PATH, built
outside the repository with the flags of oracle/Makefile.ref) over the small fixtures this script
writes under tests/golden/multiallelic_splitter/, in -i, positional-file, stdin and -q forms.

Writes tests/golden/multiallelic_splitter_cases.json.gz: per case the argv, the stdin fixture, and
the reference's stdout, stderr (base64) and exit code.  The tool runs with cwd=tests/golden,
relative fixture paths and argv[0] = the tool's name, so the names it prints are stable.

No fixture holds a GT allele index of more than 9 digits or an ALT of 46,340 alleles: the
reference's int arithmetic overflows there, which is outside the tool's domain.
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

from tests import _multiallelic_splitter_ref as R  # noqa: E402  (the fixture generators only)

TOOL = R.TOOL
DIR = "multiallelic_splitter"
COLS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"

# AF = A and AC = R as INFO; AD declared G as INFO, then R as FORMAT; PL = G and XA = A as FORMAT
PROBE_HDR = [b"##fileformat=VCFv4.2",
             b"##INFO=<ID=AF,Number=A,Type=Float,Description=\"f\">",
             b"##INFO=<ID=AC,Number=R,Type=Integer,Description=\"c\">",
             b"##INFO=<ID=AD,Number=G,Type=Integer,Description=\"as info\">",
             b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"g\">",
             b"##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"as format\">",
             b"##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"p\">",
             b"##FORMAT=<ID=XA,Number=A,Type=Integer,Description=\"x\">"]


def vcf(hdr, names, body, eol=b"\n", final=True):
    lines = list(hdr) + [b"\t".join([COLS] + list(names))] + list(body)
    return eol.join(lines) + (eol if final else b"")


def probe():
    return vcf(PROBE_HDR, [b"S1", b"S2", b"S3"], [
        b"1\t100\t.\tA\tC,G\t50\tPASS\tAF=0.1,0.2;AC=5,6,7;DB;AD=1,2,3,4,5,6;;ZZ=1,2\tGT:AD:PL:XA\t"
        b"1/2:3,4,5:0,1,2,3,4,5:7,8\t0|2:1,2\t2/10/1:.:.:.:extra",
        b"1\t101\t.\tA\tC\t50\tPASS\tAF=0.1\tGT:AD\t0/1:3,4\t1/1:0,9\t./.",
        b"1\t102\t.\tA\tC,G,T\t.\t.\t;;\tGT\t3\t3/3\t./3\t"])


def gt_forms():
    forms = [b"0/1", b"1|2", b"./.", b".", b"1", b"1/2/3", b"/", b"1/", b"/1", b"00/1", b"1a/2", b"10/2", b"2/10", b"",
             b"0|0", b"2|1", b"01/2", b"1/02", b"./2", b"2/.", b"|", b"1|", b"|2", b"1/2|3", b"1|2/3", b"-1/2", b" 1/2",
             b"1/2 ", b"3/3", b"0/3", b"999999999/1", b"11/1", b"1/11"]
    names = [b"S%d" % i for i in range(len(forms))]
    body = []
    for n in (2, 3, 11):
        alts = b",".join([b"C", b"G", b"T", b"AA", b"AC", b"AG", b"AT", b"CA", b"CC", b"CG", b"CT"][:n])
        body.append(b"\t".join([b"1", b"%d" % (100 + n), b".", b"A", alts, b".", b".", b".", b"GT"] + forms))
        body.append(b"\t".join([b"1", b"%d" % (200 + n), b".", b"A", alts, b".", b".", b".", b"DP:GT"] +
                               [b"7:" + f for f in forms]))
    return vcf(PROBE_HDR, names, body)


def list_forms():
    """A / R / G lists short, long, ".", with empty values and a trailing comma; G exact, -1, +1"""
    body = []
    for n, alts in ((2, b"C,G"), (3, b"C,G,T")):
        g = (n + 1) * (n + 2) // 2

        def nums(k):
            return b",".join(b"%d" % (10 + i) for i in range(k))

        vals = [nums(k) for k in (0, 1, n - 1, n, n + 1, n + 2, g - 1, g, g + 1)] + \
            [b".", b",", b",,", b"1,", b",1", nums(n) + b",", nums(n + 1) + b",", nums(g - 1) + b",", b".,.", b"1,.,3",
             b".," + nums(g - 1), b"a=b,c", b"x:y"]
        for key in (b"XA", b"AD", b"PL", b"DP", b"ZZ"):
            samples = [v for v in vals if b":" not in v]
            body.append(b"\t".join([b"1", b"%d" % (100 * n), key, b"A", alts, b".", b".", b".", b"GT:" + key] +
                                   [b"0/1:" + v for v in samples]))
            body.append(b"\t".join([b"1", b"%d" % (100 * n + 1), key, b"A", alts, b".", b".", b".", key] + samples))
        for key in (b"AF", b"AC", b"AD", b"IG", b"ZZ"):
            for v in vals:
                if b";" not in v:
                    body.append(b"\t".join([b"2", b"%d" % (100 * n), key, b"A", alts, b".", b".",
                                            b"X=1;" + key + b"=" + v + b";Y", b"GT", b"0/1"]))
    hdr = PROBE_HDR + [b"##INFO=<ID=IG,Number=G,Type=Integer,Description=\"g as info\">"]
    return vcf(hdr, [b"S%d" % i for i in range(21)], body)


def sample_forms():
    """fewer and more sub-fields than keys, empty samples, FORMAT without GT, GT not first, a key
    declared only as INFO"""
    body = [b"\t".join([b"1", b"1", b".", b"A", b"C,G", b".", b".", b".", fmt] + samples) for fmt, samples in (
        (b"GT:AD:PL:XA", [b"1/2", b"1/2:1,2,3", b"1/2:1,2,3:0,1,2,3,4,5:7,8:extra:more", b"", b":", b":::", b"::::",
                          b"1/2:", b":1,2,3"]),
        (b"AD:PL", [b"1,2,3:0,1,2,3,4,5", b"1,2,3", b"", b".:."]),
        (b"DP:AD:GT", [b"5:1,2,3:1/2", b"5:1,2,3", b"5", b""]),
        (b"AF:AC:GT", [b"0.1,0.2:1,2,3:2|1", b"0.1,0.2"]),           # declared as INFO only: kept
        (b"GT:GT", [b"1/2:2/1", b"1/2"]),
        (b"", [b"1/2", b""]),
        (b":", [b"1/2:3", b""]),
        (b"GT:", [b"1/2:3", b""]),
        (b"gt:Gt:GT ", [b"1/2:1/2:1/2"]),
        (b"GT:AD:PL:XA", []))]
    return vcf(PROBE_HDR, [b"S%d" % i for i in range(9)], body)


def header_forms():
    """an ID declared in both sections in both orders, lines without Number= or ID=, Number= first,
    a ##FORMAT line after #CHROM, an unterminated value, an empty ID"""
    hdr = [b"##fileformat=VCFv4.2",
           b"##INFO=<ID=K1,Number=A,Type=Integer>", b"##FORMAT=<ID=K1,Number=R,Type=Integer>",   # FORMAT wins
           b"##FORMAT=<ID=K2,Number=R,Type=Integer>", b"##INFO=<ID=K2,Number=A,Type=Integer>",   # INFO wins
           b"##INFO=<ID=K3,Type=Integer,Description=\"no number\">",
           b"##INFO=<Number=A,Type=Integer,Description=\"no id\">",
           b"##INFO=<Number=A,ID=K4,Type=Integer>",                                               # Number= first
           b"##INFO=<ID=K5,Number=A", b"##INFO=<ID=K6,Number=A>", b"##INFO=<ID=K7,Number=R",
           b"##INFO=<ID=K8,Number=1>", b"##INFO=<ID=K8,Number=A>", b"##INFO=<ID=K9,Number=A>", b"##INFO=<ID=K9,Number=2>",
           b"##INFO=<ID=,Number=A>", b"##INFO =<ID=KA,Number=A>", b"##info=<ID=KB,Number=A>", b"#INFO=<ID=KC,Number=A>",
           b"##INFO=<ID=KD,Number=a>", b"##INFO=<ID=KE,Number=A >", b"##INFO=<ID=KF,Number=.>",
           b"##INFO=<ID=KG,Number=A,ID=KH,Number=R>", b"##contig=<ID=KI,Number=A>",
           b"##FORMAT=<ID=F1,Number=A>", b"", b"##FORMAT=<ID=F2,Number=G>"]
    info = b";".join(b"%s=1,2,3" % k for k in (b"K1", b"K2", b"K3", b"K4", b"K5", b"K6", b"K7", b"K8", b"K9", b"KA", b"KB",
                                               b"KC", b"KD", b"KE", b"KF", b"KG", b"KH", b"KI", b"F1", b"F3")) + b";=4,5,6"
    fmt = b"GT:K1:K2:F1:F2:F3:K6"
    s = b"1/2:1,2,3:1,2,3:1,2:0,1,2,3,4,5:1,2:1,2"
    body = [b"\t".join([b"1", b"1", b".", b"A", b"C,G", b".", b".", info, fmt, s]),
            b"##FORMAT=<ID=F3,Number=A>",                                                          # after #CHROM: not read
            b"\t".join([b"1", b"2", b".", b"A", b"C,G", b".", b".", info, fmt, s])]
    return vcf(hdr, [b"S1"], body)


def info_forms():
    infos = [b".", b"", b";;", b";", b"DB", b"DB;H2", b"AF=", b"AC=", b"K=", b"AF=1=2,3=4", b"ZZ=a=b", b"=", b"=1,2",
             b"AF", b"AF=0.1,0.2;", b";AF=0.1,0.2", b"AF=0.1,0.2;;AC=1,2,3", b"AF=.;AC=.", b"AF=.,.;AC=.,.,.",
             b"UNKNOWN=1,2,3", b"AF=0.1,0.2;AF=0.3,0.4", b"AD=1,2,3,4,5,6", b"af=0.1,0.2", b"AF =0.1,0.2", b" AF=0.1,0.2",
             b"AF=0.1,0.2 ", b"AC=1", b"AC=1,2", b"AC=1,2,3,4", b"AF=0.1", b"AF=0.1,0.2,0.3", b"A;B;C;D;E;F;G;H;I;J",
             b"AF=" + b",".join(b"0.%d" % i for i in range(1, 40))]
    body = [b"\t".join([b"1", b"%d" % i, b".", b"A", b"C,G", b".", b".", x, b"GT", b"1/2"]) for i, x in enumerate(infos)]
    return vcf(PROBE_HDR, [b"S1"], body)


def alt_forms():
    """nAlts of 2, 3, 9, 10 and 11 (two-digit allele indices), empty alleles"""
    pool = [b"C", b"G", b"T", b"AA", b"AC", b"AG", b"AT", b"CA", b"CC", b"CG", b"CT"]
    body = []
    for n in (2, 3, 9, 10, 11):
        g = (n + 1) * (n + 2) // 2
        gts = [b"%d/%d" % (a, b) for a, b in ((0, n), (n, n), (1, n), (n - 1, n), (n, 1), (n + 1, 1), (10, 1), (1, 10))]
        body.append(b"\t".join(
            [b"1", b"%d" % n, b".", b"A", b",".join(pool[:n]), b".", b".",
             b"AF=" + b",".join(b"0.%d" % i for i in range(n)) + b";AC=" + b",".join(b"%d" % i for i in range(n + 1)),
             b"GT:AD:PL:XA"] +
            [x + b":" + b",".join(b"%d" % i for i in range(n + 1)) + b":" + b",".join(b"%d" % i for i in range(g)) + b":" +
             b",".join(b"%d" % (50 + i) for i in range(n)) for x in gts]))
    for alt in (b"C,", b",", b",C", b",,", b"C,,G", b"<DEL>,<INS:ME>,*", b"C,C"):
        body.append(b"\t".join([b"2", b"5", b".", b"A", alt, b".", b".", b"AF=0.1,0.2,0.3", b"GT:AD", b"1/2:1,2,3", b"0/3"]))
    return vcf(PROBE_HDR, [b"S%d" % i for i in range(8)], body)


def field_counts():
    """8, 9 and 10 fields, each with and without a trailing tab; fewer; tabs only"""
    f = [b"1", b"5", b".", b"A", b"C,G", b".", b".", b"AF=0.1,0.2", b"GT:AD", b"1/2:1,2,3"]
    body = []
    for k in (4, 5, 7, 8, 9, 10):
        body += [b"\t".join(f[:k]), b"\t".join(f[:k]) + b"\t", b"\t".join(f[:k]) + b"\t\t"]
    body += [b"\t" * k for k in (1, 4, 7, 8, 9, 10)]
    body += [b"1\t5\t.\tA\t,\t\t\t\t", b"1\t5\t.\tA\t,\t\t\t\t\t", b"x", b" ", b"1\t5\t.\tA\tC,G"]
    return vcf(PROBE_HDR, [b"S1"], body)


def line_mix():
    rec = b"1\t5\t.\tA\tC,G\t.\t.\tAF=0.1,0.2\tGT:AD\t1/2:1,2,3"
    return vcf(PROBE_HDR[:3] + [b""] + PROBE_HDR[3:], [b"S1"],
               [rec, b"", b"#a comment among the data", rec, b"", b"", b"##FORMAT=<ID=ZQ,Number=A>",
                b"1\t6\t.\tA\tC\t.\t.\tAF=0.1\tGT:AD\t0/1:1,2", COLS + b"\tS1", rec, b"#", b"1\t7\t.\tA\tC,G\t.\t.\t.\tGT:ZQ\t1/2:8,9"])


def fixtures():
    rec = b"1\t5\t.\tA\tC,G\t.\t.\tAF=0.1,0.2\tGT:AD\t1/2:1,2,3\n"
    one = b"1\t6\t.\tA\tC\t.\t.\tAF=0.1\tGT:AD\t0/1:1,2\n"
    hdr = vcf(PROBE_HDR, [b"S1"], [])
    lm = line_mix()
    return {
        "probe.vcf": probe(),
        "probe_crlf.vcf": probe().replace(b"\n", b"\r\n"),
        "gt_forms.vcf": gt_forms(),
        "list_forms.vcf": list_forms(),
        "sample_forms.vcf": sample_forms(),
        "sample_forms_crlf.vcf": sample_forms().replace(b"\n", b"\r\n"),
        "header_forms.vcf": header_forms(),
        "info_forms.vcf": info_forms(),
        "alt_forms.vcf": alt_forms(),
        "field_counts.vcf": field_counts(),
        "field_counts_crlf.vcf": field_counts().replace(b"\n", b"\r\n"),
        "line_mix.vcf": lm,
        "line_mix_crlf.vcf": lm.replace(b"\n", b"\r\n"),
        "no_final_newline_copied.vcf": hdr + rec + one[:-1],
        "no_final_newline_split.vcf": hdr + one + rec[:-1],
        "no_final_newline_split_tab.vcf": hdr + one + rec[:-1] + b"\t",
        "no_final_newline_header.vcf": hdr[:-1],
        "no_chrom.vcf": b"\n".join(PROBE_HDR) + b"\n" + rec + b"\n" + one + b"#late\n" + hdr + rec,
        "no_chrom_no_final_newline.vcf": b"\n".join(PROBE_HDR) + b"\n\n" + rec + one[:-1],
        "data_before_chrom.vcf": b"\n".join(PROBE_HDR[:6]) + b"\n" + rec + b"\n".join(PROBE_HDR[6:]) + b"\n" +
        COLS + b"\tS1\n" + rec + b"1\t8\t.\tA\tC,G\t.\t.\t.\tGT:PL\t1/2:0,1,2,3,4,5\n",
        "data_only.vcf": rec + one + rec,
        "header_only.vcf": hdr,
        "hash_lines_only.vcf": b"\n".join(PROBE_HDR) + b"\n",
        "only_newlines.vcf": b"\n\n\n",
        "generated.vcf": R.gen_vcf(31, 40, 5, alts=(1, 2, 3, 4), keys=(b"GT", b"AD", b"DP", b"PL", b"XA"), odd=0.3, mix=True),
        "generated_crlf.vcf": R.gen_vcf(32, 30, 3, odd=0.3, mix=True, crlf=True, final_newline=False),
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
    add("i_wins_over_positional", ["-i", p("probe.vcf"), p("line_mix.vcf")])
    add("last_i_wins", ["-i", p("line_mix.vcf"), "-i", p("probe.vcf")])
    add("positional_before_q", [p("probe.vcf"), "-q"])
    add("two_positionals", [p("probe.vcf"), p("line_mix.vcf")])
    add("input_equals", ["--input=" + p("probe.vcf")])
    add("attached_value", ["-qi" + p("probe.vcf")])
    add("prefix_of_long", ["--inp", p("probe.vcf"), "--qu"])
    add("dash_is_a_file_name", ["-i", "-"], stdin=p("probe.vcf"))
    add("double_dash", ["--", p("probe.vcf")])
    add("missing_file", ["-i", p("does_not_exist.vcf")])
    add("missing_file_positional_quiet", ["-q", p("does_not_exist.vcf")])
    add("help", ["--help"])
    add("help_short", ["-h"])
    add("help_with_input", ["-i", p("probe.vcf"), "--help"])
    add("help_in_group", ["-qh"], stdin=p("probe.vcf"))
    add("help_prefix", ["--he"], stdin=p("probe.vcf"))
    add("version", ["--version"])
    add("version_short", ["-v"])
    add("bad_long", ["--bogus", "-i", p("probe.vcf")])
    add("bad_short", ["-i", p("probe.vcf"), "-x"])
    add("bad_short_stdin", ["-x"], stdin=p("probe.vcf"))
    add("missing_argument", ["-q", "-i"])
    add("missing_argument_long", ["--input"])
    add("quiet_with_value", ["--quiet=1"], stdin=p("probe.vcf"))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True, help="the reference VCFX_multiallelic_splitter executable")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref_bin)
    os.makedirs(os.path.join(HERE, DIR), exist_ok=True)
    for name, data in fixtures().items():
        assert len(data) < 100000, name
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
    path = os.path.join(HERE, "multiallelic_splitter_cases.json.gz")
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(blob)
    print("%d cases, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
