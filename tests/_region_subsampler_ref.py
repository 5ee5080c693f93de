"""VCFX_region_subsampler restated in plain Python (VCFX_region_subsampler.cpp): the CLI (run :254-324),
the BED loader (loadRegions :344-381), the merge (sortAndMergeIntervals :383-404), the file mode
(processVCFMmap :427-517) and the stdin mode (processVCF :519-564), plus the input generators of the
tests.  tests/test_region_subsampler_ref.py holds it to the compiled reference's recorded bytes
(tests/golden/region_subsampler_cases.json.gz); tests/test_gpu_rs.py checks the device against it on
generated inputs.

The two modes differ in the column rule (file: CHROM and POS present and not empty; stdin: eight
fields), in POS (file: every digit byte of the field accumulated in an int that wraps modulo 2^32;
stdin: std::stoi, a failure is a warning) and in -q (silences the file mode's warnings only).
Outside the domain: NUL bytes, a BED start or end of 2147483647."""
import base64
import bisect
import gzip
import json
import os
import random
import re

TOOL = "VCFX_region_subsampler"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HELP = (b"VCFX_region_subsampler: Keep only variants whose (CHROM,POS) is in a set of regions.\n\n"
        b"Usage:\n"
        b"  VCFX_region_subsampler -b FILE -i input.vcf > out.vcf\n"
        b"  VCFX_region_subsampler --region-bed FILE < input.vcf > out.vcf\n\n"
        b"Options:\n"
        b"  -h, --help             Show help.\n"
        b"  -b, --region-bed FILE  BED file listing multiple regions.\n"
        b"  -i, --input FILE       Input VCF file (uses mmap for better performance).\n"
        b"  -q, --quiet            Suppress warnings.\n\n"
        b"Description:\n"
        b"  Reads the BED, which is <chrom> <start> <end> in 0-based. This tool converts\n"
        b"  them to 1-based [start+1 .. end]. Then merges intervals per chrom.\n"
        b"  Then only lines in the VCF that fall in those intervals for that CHROM are printed.\n\n"
        b"Example:\n"
        b"  VCFX_region_subsampler --region-bed myregions.bed -i input.vcf > out.vcf\n")
VERSION = b"VCFX_region_subsampler version 1.1.4\n"
WARN_EARLY = b"Warning: data line encountered before #CHROM => skipping.\n"
WARN_SHORT_FILE = b"Warning: line has insufficient columns => skipping.\n"
WARN_SHORT_STDIN = b"Warning: line has <8 columns => skipping.\n"
WARN_POS = b"Warning: invalid POS => skipping.\n"
NO_BED = b"Error: Must specify --region-bed <FILE>.\n"

# vcfx_gpu.h VCFXG_RS_*
EMPTY, HEADER, IN, OUT, EARLY, SHORT, BADPOS = 0, 1, 2, 3, 4, 5, 6
WINDOW = 64  # VCFXG_RS_WINDOW: the bytes of a line the device's lane path looks at

LONG = {"help": ("h", False), "region-bed": ("b", True), "input": ("i", True), "quiet": ("q", False)}
SHORT_OPTS = {"h": False, "b": True, "i": True, "q": False}
SPACE = b" \t\n\v\f\r"
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def getopt_long(argv):
    """GNU getopt_long(argc, argv, "hb:i:q", long_opts) with argument permutation:
    ([(letter or '?', value, its stderr message)], operands)"""
    prog = argv[0].encode()
    opts, operands = [], []
    i = 1
    while i < len(argv):
        a = argv[i]
        i += 1
        if a == "--":
            operands += argv[i:]
            break
        if a.startswith("--"):
            name, eq, val = a[2:].partition("=")
            hits = [name] if name in LONG else [k for k in LONG if k.startswith(name)]
            if len(hits) != 1:
                if hits:
                    msg = prog + b": option '" + a.encode() + b"' is ambiguous; possibilities:" + \
                        b"".join(b" '--" + h.encode() + b"'" for h in hits) + b"\n"
                else:
                    msg = prog + b": unrecognized option '" + a.encode() + b"'\n"
                opts.append(("?", None, msg))
                continue
            k = hits[0]
            letter, takes = LONG[k]
            if takes:
                if eq:
                    opts.append((letter, val, b""))
                elif i < len(argv):
                    opts.append((letter, argv[i], b""))
                    i += 1
                else:
                    opts.append(("?", None, prog + b": option '--" + k.encode() + b"' requires an argument\n"))
            elif eq:
                opts.append(("?", None, prog + b": option '--" + k.encode() + b"' doesn't allow an argument\n"))
            else:
                opts.append((letter, None, b""))
        elif a.startswith("-") and len(a) > 1:
            j = 1
            while j < len(a):
                ch = a[j]
                j += 1
                if ch not in SHORT_OPTS:
                    opts.append(("?", None, prog + b": invalid option -- '" + ch.encode() + b"'\n"))
                elif SHORT_OPTS[ch]:
                    if j < len(a):
                        opts.append((ch, a[j:], b""))
                    elif i < len(argv):
                        opts.append((ch, argv[i], b""))
                        i += 1
                    else:
                        opts.append(("?", None, prog + b": option requires an argument -- '" + ch.encode() + b"'\n"))
                    break
                else:
                    opts.append((ch, None, b""))
        else:
            operands.append(a)
    return opts, operands


# ---- the BED -------------------------------------------------------------------------------------

_INT = re.compile(rb"[ \t\n\v\f\r]*([+-]?)([0-9]+)")
_NAME = re.compile(rb"[ \t\n\v\f\r]*([^ \t\n\v\f\r]+)")


def extract_int(line, p):
    """`stream >> int` at p: (value, the place after it), or None without a digit or outside int"""
    m = _INT.match(line, p)
    if not m:
        return None
    v = int(m.group(2))
    v = -v if m.group(1) == b"-" else v
    return (v, m.end()) if INT_MIN <= v <= INT_MAX else None


def load_bed(text):
    """loadRegions :344-381: (names in first-appearance order, [(name index, 1-based start, end)],
    the warnings' bytes)"""
    names, ids, ivs, warn = [], {}, [], b""
    for no, line in enumerate(text.split(b"\n")[:-1] if text.endswith(b"\n") else text.split(b"\n"), 1):
        if not line or line[:1] == b"#":
            continue
        m = _NAME.match(line)
        a = extract_int(line, m.end()) if m else None
        b = extract_int(line, a[1]) if a else None
        if not b:
            warn += b"Warning: skipping invalid bed line %d: " % no + line + b"\n"
            continue
        start, end = max(a[0], 0) + 1, b[0]
        if end < start:
            continue
        name = m.group(1)
        if name not in ids:
            ids[name] = len(names)
            names.append(name)
        ivs.append((ids[name], start, end))
    return names, ivs, warn


def merged(ivs):
    """sortAndMergeIntervals :383-404 in (name index, start) order: [(name index, start, end)]"""
    out = []
    for i, s, e in sorted(ivs, key=lambda x: (x[0], x[1])):
        if out and out[-1][0] == i and s <= out[-1][2] + 1:
            if e > out[-1][2]:
                out[-1] = (i, out[-1][1], e)
        else:
            out.append((i, s, e))
    return out


class Table:
    """the merged intervals per name, as the reference searches them"""

    def __init__(self, bed_text=b"", names=None, ivs=None):
        """from a BED's bytes, or (the raw ABI's view) from names and (name index, start, end) rows"""
        if names is None:
            self.names, self.ivs, self.warnings = load_bed(bed_text)
        else:
            self.names, self.ivs, self.warnings = list(names), list(ivs), b""
        self.rows = merged(self.ivs)
        self.by = {}
        for i, s, e in self.rows:
            st, en = self.by.setdefault(self.names[i], ([], []))
            st.append(s)
            en.append(e)

    def arrays(self):
        """what Engine.regions_load takes"""
        return self.names, [x[0] for x in self.ivs], [x[1] for x in self.ivs], [x[2] for x in self.ivs]

    def inside(self, chrom, pos):
        r = self.by.get(chrom)
        if not r:
            return False
        k = bisect.bisect_right(r[0], pos) - 1
        return k >= 0 and pos <= r[1][k]


# ---- the lines -----------------------------------------------------------------------------------

def pos_file(field):
    """parseIntFast :190-198: every digit byte, the int wrapping modulo 2^32"""
    v = 0
    for c in field:
        if 48 <= c <= 57:
            v = (v * 10 + c - 48) & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def pos_stdin(field):
    """std::stoi(field): None where it throws"""
    r = extract_int(field, 0)
    return r[0] if r else None


def line_spans(buf):
    """[ls, le) of every line: split at '\\n' only; bytes after the last one are a line"""
    out, p, n = [], 0, len(buf)
    while p < n:
        k = buf.find(b"\n", p)
        if k < 0:
            k = n
        out.append((p, k))
        p = k + 1
    return out


def statuses(buf, stdin, table):
    """per line its VCFXG_RS_* status"""
    st, seen = [], False
    for ls, le in line_spans(buf):
        line = buf[ls:le]
        if not line:
            st.append(EMPTY)
        elif line[:1] == b"#":
            st.append(HEADER)
            seen = seen or line.startswith(b"#CHROM")
        elif not seen:
            st.append(EARLY)
        else:
            f = line.split(b"\t")
            if stdin:
                if len(f) < 8:
                    st.append(SHORT)
                    continue
                pos = pos_stdin(f[1])
                if pos is None:
                    st.append(BADPOS)
                    continue
            else:
                if len(f) < 2 or not f[0] or not f[1]:
                    st.append(SHORT)
                    continue
                pos = pos_file(f[1])
            st.append(IN if table.inside(f[0], pos) else OUT)
    return st


def lane_path(line, stdin):
    """the line is settled by the class kernel's lane pass: it is no longer than the window, or its
    first two (stdin: seven) tabs lie inside the window (else the wave takes it)"""
    if len(line) <= WINDOW or line[:1] == b"#":
        return True
    return line[:WINDOW].count(b"\t") >= (7 if stdin else 2)


def subsample(buf, stdin, table, quiet=False):
    """(stdout, stderr) of one mode over the input bytes (the BED's warnings not included)"""
    st = statuses(buf, stdin, table)
    out = b"".join(buf[ls:le] + b"\n" for (ls, le), s in zip(line_spans(buf), st) if s in (EMPTY, HEADER, IN))
    if quiet and not stdin:
        return out, b""
    w = {EARLY: WARN_EARLY, SHORT: WARN_SHORT_STDIN if stdin else WARN_SHORT_FILE, BADPOS: WARN_POS}
    return out, b"".join(w[s] for s in st if s in w)


def run(argv, stdin=b"", cwd=None):
    """main :574-580 and run :254-324: (stdout, stderr, rc)"""
    args = argv[1:]
    if "--help" in args or "-h" in args:  # vcfx::handle_common_flags
        return HELP, b"", 0
    if "--version" in args or "-v" in args:
        return VERSION, b"", 0
    opts, _ = getopt_long(argv)
    path, bed, quiet, help_, err = "", "", False, False, b""
    for k, v, msg in opts:
        err += msg
        if k == "i":
            path = v
        elif k == "b":
            bed = v
        elif k == "q":
            quiet = True
        else:
            help_ = True
    if help_:
        return HELP, err, 0
    if not bed:
        return HELP, err + NO_BED, 1
    full = os.path.join(cwd, bed) if cwd else bed
    if os.path.isdir(full):
        text = b""  # (a directory opens and gives no line)
    else:
        try:
            with open(full, "rb") as f:
                text = f.read()
        except OSError:
            return b"", err + b"Error: cannot open BED " + bed.encode() + b"\nError: failed to load regions from " + \
                bed.encode() + b"\n", 1
    table = Table(text)
    err += table.warnings
    if path:
        full = os.path.join(cwd, path) if cwd else path
        try:
            with open(full, "rb") as f:
                buf = f.read()
        except OSError:
            return b"", err + b"Error: failed to process input file: " + path.encode() + b"\n", 1
        o, e = subsample(buf, False, table, quiet)
        return o, err + e, 0
    o, e = subsample(stdin or b"", True, table, quiet)
    return o, err + e, 0


# ---- golden cases --------------------------------------------------------------------------------

def load_cases():
    with gzip.open(os.path.join(GOLDEN, "region_subsampler_cases.json.gz"), "rb") as f:
        cases = json.loads(f.read())["cases"]
    for c in cases:
        c["stdout"] = base64.b64decode(c["stdout"])
        c["stderr"] = base64.b64decode(c["stderr"])
    return cases


def case_stdin(case):
    if case["stdin"]:
        with open(os.path.join(GOLDEN, case["stdin"]), "rb") as f:
            return f.read()
    return b""


# ---- generated inputs ----------------------------------------------------------------------------

HDR = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS0\tS1\tS2\n"
CHROMS = (b"1", b"2", b"chr10", b"X")
ABSENT = b"chrUn"  # never in a generated BED
SPAN = 6000


def record(chrom, pos, rest=b".\tA\tC\t.\tPASS\t.\tGT\t0/1\t1/1\t0|0"):
    return b"\t".join([chrom, pos, rest])


def gen_bed(seed, per_chrom=14):
    """per chromosome: intervals that overlap, nest, touch (end == the next start), nearly touch (one
    base between) and stand alone, in shuffled order, covering about half of [1, SPAN]"""
    rnd = random.Random(seed)
    rows = []
    for c in CHROMS:
        p = rnd.randrange(0, 200)
        for k in range(per_chrom):
            n = rnd.randrange(60, 400)
            rows.append((c, p, p + n))
            how = k % 5
            if how == 0:
                rows.append((c, p + n // 3, p + n + 40))      # overlapping
            elif how == 1:
                rows.append((c, p + 5, p + n - 5))            # nested
            elif how == 2:
                rows.append((c, p + n, p + n + 30))           # touching: its first base follows the last
                n += 30
            elif how == 3:
                rows.append((c, p + n + 1, p + n + 31))       # one base between the two
                n += 31
            p += n + rnd.randrange(100, 500)
    rnd.shuffle(rows)
    return b"".join(b"%s\t%d\t%d\n" % r for r in rows)


def gen_vcf(seed, n, bed, mix=False, crlf=False, final_newline=True):
    """n data lines over CHROMS and one absent name: a fifth of them at a boundary of a BED row (its
    start: outside, start + 1, end: inside, end + 1), the rest anywhere.  mix: '#' lines, empty lines,
    short lines of every kind and bad POS fields in between, data lines before the header, a second
    "#CHROM" line."""
    rnd = random.Random(seed)
    rows = [ln.split(b"\t") for ln in bed.split(b"\n") if ln]
    eol = b"\r\n" if crlf else b"\n"

    def tail():
        return b"rs%d\t%s\t%s\t.\tPASS\tDP=%d\tGT\t%s" % (rnd.randrange(10 ** 6), rnd.choice((b"A", b"ACGT", b"G")),
                                                             rnd.choice((b"C", b"T,G", b"<DEL>")), rnd.randrange(99),
                                                             b"\t".join(rnd.choice((b"0/0", b"0/1", b"1|1", b"./."))
                                                                        for _ in range(3)))

    lines = []
    for _ in range(n):
        r = rnd.random()
        if r < 0.2:
            c, s, e = rnd.choice(rows)
            pos = rnd.choice((int(s), int(s) + 1, int(e), int(e) + 1))
        elif r < 0.27:
            c, pos = ABSENT, rnd.randrange(1, SPAN)
        else:
            c, pos = rnd.choice(CHROMS), rnd.randrange(1, SPAN)
        lines.append(record(c, b"%d" % max(pos, 1), tail()))
    out = []
    if mix:
        out += [b"##fileformat=VCFv4.2", lines[0], b"", b"1\t5", HDR.split(b"\n")[1]]
    else:
        out += HDR.split(b"\n")[:2]
    for k, ln in enumerate(lines):
        if mix:
            r = rnd.random()
            if r < 0.04:
                out.append(b"")
            elif r < 0.08:
                out.append(b"#comment %d" % len(out))
            elif r < 0.14:
                out.append(rnd.choice((b"1\t5\t.\tA", b"1", b"x", b"1\t", b"\t5\t.\tA\tC\t.\t.\t.", b"1\t\t.\tA\tC\t.\t.\t.",
                                       b"1\t5\t.\tA\tC\t.\t.", b" ")))
            elif r < 0.18:
                out.append(record(rnd.choice(CHROMS), rnd.choice((b"abc", b"+", b"99999999999", b"-", b"x7")), tail()))
            elif r < 0.19:
                out.append(b"#CHROM again")
        out.append(ln)
    return eol.join(out) + (eol if final_newline else b"")


# the generated inputs the GPU tests use: name -> (BED seed, gen_vcf arguments)
GENERATED = {
    "g600": (1, dict(seed=600, n=600)),
    "n255": (2, dict(seed=255, n=253)),
    "n256": (2, dict(seed=256, n=254)),
    "n257": (3, dict(seed=257, n=255)),
    "n4097": (4, dict(seed=4097, n=4095)),
    "mix": (5, dict(seed=7, n=500, mix=True)),
    "mix_crlf": (6, dict(seed=8, n=300, mix=True, crlf=True)),
    "mix_no_final_newline": (7, dict(seed=9, n=300, mix=True, final_newline=False)),
    "routes": (8, dict(seed=10, n=2000, mix=True)),
    "collide": (3, dict(seed=11, n=400, mix=True)),
}


def generated(name):
    """(the VCF's bytes, the BED's bytes)"""
    bed_seed, kw = GENERATED[name]
    bed = gen_bed(bed_seed)
    return gen_vcf(bed=bed, **kw), bed


def nontrivial(buf, bed, stdin):
    """(decided data lines, kept lines, the lines at a BED row's start / start + 1 / end / end + 1, the
    lines whose CHROM the BED does not name)"""
    table = Table(bed)
    st = statuses(buf, stdin, table)
    edges = [set(), set(), set(), set()]
    for ln in bed.split(b"\n"):
        if ln:
            c, s, e = ln.split(b"\t")
            for k, v in enumerate((int(s), int(s) + 1, int(e), int(e) + 1)):
                edges[k].add((c, v))
    at, absent = [0, 0, 0, 0], 0
    for (ls, le), s in zip(line_spans(buf), st):
        if s in (IN, OUT):
            f = buf[ls:le].split(b"\t")
            if not f[1].isdigit():
                continue
            for k in range(4):
                at[k] += (f[0], int(f[1])) in edges[k]
            absent += f[0] not in table.by
    return st.count(IN) + st.count(OUT), st.count(IN), at, absent
