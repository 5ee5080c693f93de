"""VCFX_haplotype_extractor in plain Python: the reference tool's behaviour (VCFX_haplotype_extractor.cpp:
processVariantFast :376-568, phaseIsConsistent :303-349, the four readers :581-819, main :826-911)
restated line by line, the device's view of the same inputs (statuses, POS, member and block numbers,
the first flipping sample, the block table with 64-bit row offsets, the rows' text), fixture generators,
and the loader of the recorded cases (tests/golden/haplotype_extractor_cases.json.gz, written by
tests/golden/make_haplotype_extractor_golden.py from the compiled reference).

Outside the domain (no golden holds one): a POS above 2147483647 or a difference of two POS values
that does not fit an int; a NUL byte; a line of 2 GiB or more; a -b value std::stoi rejects (the
reference dies on the exception, the drop-in prints bad_block_size() and returns 1); a negative -b value
on an input that holds a member (the reference dies in its first reserve; the drop-in follows the signed
arithmetic of the model).
"""
import base64
import gzip
import json
import os
import random

TOOL = "VCFX_haplotype_extractor"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# printHelp :237-261
HELP = ("VCFX_haplotype_extractor\n"
        "Usage: VCFX_haplotype_extractor [OPTIONS] [input.vcf]\n\n"
        "Options:\n"
        "  -h, --help                 Display this help message and exit.\n"
        "  -i, --input FILE           Input VCF file (uses fast memory-mapped I/O).\n"
        "  -b, --block-size <int>     Maximum distance for grouping consecutive variants (default 100000).\n"
        "  -c, --check-phase-consistency  If set, try a minimal check across variants.\n"
        "  -s, --streaming            Enable streaming mode: output blocks immediately when complete.\n"
        "                             Uses O(block_size) memory instead of O(total_variants).\n"
        "  -q, --quiet                Suppress warning messages.\n"
        "  -d, --debug                Output verbose debug information.\n\n"
        "Description:\n"
        "  Extracts phased haplotype blocks from genotype data in a VCF file. "
        "It reconstructs haplotypes for each sample by analyzing phased genotype fields.\n\n"
        "Performance:\n"
        "  File input (-i): Uses memory-mapped I/O for 50-100x faster processing.\n"
        "  Streaming mode:  Outputs blocks immediately when complete. Enables\n"
        "                   processing of arbitrarily large files with bounded memory.\n\n"
        "Examples:\n"
        "  ./VCFX_haplotype_extractor -i phased.vcf > haplotypes.tsv\n"
        "  ./VCFX_haplotype_extractor -b 50000 < phased.vcf > haplotypes.tsv\n"
        "  ./VCFX_haplotype_extractor -s -i large_phased.vcf > haplotypes.tsv\n"
        "  ./VCFX_haplotype_extractor -s -b 10000 -i phased.vcf > haplotypes.tsv\n").encode()
VERSION = b"VCFX_haplotype_extractor version 1.1.4\n"
NO_SAMPLES = b"Error: VCF header does not contain sample columns.\n"
NO_CHROM = b"Error: no #CHROM header found before data.\n"
EMPTY_FILE = b"Error: empty file\n"
W_SHORT = b"Warning: skipping invalid VCF line (<10 fields)\n"
W_POS = b"Warning: invalid POS => skip variant\n"
BARE_HEADER = b"CHROM\tSTART\tEND\n"

# include/vcfx_gpu.h
EMPTY, HEADER, SHORT, BADPOS, NOGT, UNPHASED, MEMBER = 0, 1, 2, 3, 4, 5, 6
TILE_MEMBERS = 32    # the layout / emit tile: members
TILE_SAMPLES = 64    # ... and samples
MODE_FILE, MODE_STDIN = 0, 1

LONG = {"help": False, "input": True, "block-size": True, "check-phase-consistency": False, "streaming": False,
        "quiet": False, "debug": False}
SHORT_OPTS = {"h": False, "i": True, "b": True, "c": False, "s": False, "q": False, "d": False}
LONG_LETTER = {"help": "h", "input": "i", "block-size": "b", "check-phase-consistency": "c", "streaming": "s",
               "quiet": "q", "debug": "d"}


def getopt_long(argv):
    """GNU getopt_long(argc, argv, "hi:b:csqd", long_opts) with argument permutation:
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
            if LONG[k]:
                if eq:
                    opts.append((LONG_LETTER[k], val, b""))
                elif i < len(argv):
                    opts.append((LONG_LETTER[k], argv[i], b""))
                    i += 1
                else:
                    opts.append(("?", None, prog + b": option '--" + k.encode() + b"' requires an argument\n"))
            elif eq:
                opts.append(("?", None, prog + b": option '--" + k.encode() + b"' doesn't allow an argument\n"))
            else:
                opts.append((LONG_LETTER[k], None, b""))
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


def stoi(text):
    """std::stoi: white space, a sign, digits; None where it throws (no digit, or not an int)"""
    s = text.encode() if isinstance(text, str) else text
    p = 0
    while p < len(s) and s[p] in b" \t\n\v\f\r":
        p += 1
    neg = False
    if p < len(s) and s[p] in b"+-":
        neg = s[p] == 45
        p += 1
    q = p
    while q < len(s) and 48 <= s[q] <= 57:
        q += 1
    if q == p:
        return None
    v = int(s[p:q])
    v = -v if neg else v
    return v if -2147483648 <= v <= 2147483647 else None


def bad_block_size(text):
    return b"Error: invalid block size: " + text.encode() + b"\n"


# ---- one line ------------------------------------------------------------------------------------

def raw_lines(buf):
    """the lines of buf, split at '\\n' only; bytes after the last one are a line"""
    if not buf:
        return []
    lines = buf.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def gt_index(fmt):
    """findGTIndex :174-193: the first key that is exactly GT"""
    for i, k in enumerate(fmt.split(b":")):
        if k == b"GT":
            return i
    return -1


def nth_field(sample, n):
    """extractNthField :196-214"""
    f = sample.split(b":")
    return f[n] if 0 <= n < len(f) else b""


def body_of(line, stdin):
    """what the tool sees of a raw line: None when it is skipped as empty.  One trailing '\\r' is
    stripped; on stdin a line of '\\r' alone is not skipped (:739-744: the test for empty comes first)"""
    if not line:
        return None
    if line.endswith(b"\r"):
        line = line[:-1]
        if not line and not stdin:
            return None
    return line


def classify(body, ns):
    """a data line (not empty-skipped, no '#'): (status, pos, chrom, the ns GTs for a member)"""
    f = body.split(b"\t")
    if len(f) < 10:
        return SHORT, 0, b"", None
    if any(not 48 <= c <= 57 for c in f[1]):
        return BADPOS, 0, f[0], None
    pos = int(f[1]) if f[1] else 0
    gi = gt_index(f[8])
    if gi < 0:
        return NOGT, pos, f[0], None
    gts, ok = [], True
    for s in range(ns):
        g = nth_field(f[9 + s], gi) if 9 + s < len(f) else b""
        if not g or b"|" not in g:
            ok = False
        gts.append(g)
    return (MEMBER if ok else UNPHASED), pos, f[0], gts if ok else None


def flips(last, new):
    """the flip test of one sample :321-341"""
    if len(last) < 3 or len(new) < 3:
        return False
    a, b, c, d = last[0], last[-1], new[0], new[-1]
    return a != c and b != d and a == d and b == c


def is_fixed(body, ns):
    """the line is ns units "a|b\\t" after a FORMAT of exactly GT (the device's closed-form rows)"""
    f = body.split(b"\t")
    return len(f) == 9 + ns and f[8] == b"GT" and all(len(g) == 3 and g[1] == 124 for g in f[9:])


# ---- the tool ------------------------------------------------------------------------------------

def extract(buf, stdin, T=100000, check=False, streaming=False, quiet=False, debug=False):
    """the four readers :581-819: (stdout, stderr, rc)"""
    names, err = None, []
    blocks = []  # [chrom, start, end, [per sample list of GTs]]
    last = None
    for raw in raw_lines(buf):
        body = body_of(raw, stdin)
        if body is None:
            continue
        if body[:1] == b"#":
            if names is None and body[:6] == b"#CHROM":
                f = body.split(b"\t")
                if len(f) <= 9:
                    return b"", b"".join(err) + NO_SAMPLES, 1
                names = f[9:]
            continue
        if names is None:
            return b"", b"".join(err) + NO_CHROM, 1
        st, pos, chrom, gts = classify(body, len(names))
        if st == SHORT:
            if not quiet:
                err.append(W_SHORT)
        elif st == BADPOS:
            if not quiet:
                err.append(W_POS)
        elif st == UNPHASED:
            if not quiet:
                err.append(b"Warning: Not all samples phased at %s:%d.\n" % (chrom, pos))
        if st != MEMBER:
            continue
        can = bool(blocks) and chrom == blocks[-1][0] and pos - blocks[-1][2] <= T
        if can and check:
            if debug:
                err.append(b"Checking phase consistency\n")
            for s, (a, b) in enumerate(zip(last, gts)):
                if debug:
                    err.append(b"Sample %d last GT: %s new GT: %s\n" % (s, a, b))
                if len(a) < 3 or len(b) < 3:
                    continue
                if debug:
                    err.append(b"Comparing alleles: %c|%c vs %c|%c\n" % (a[0], a[-1], b[0], b[-1]))
                if flips(a, b):
                    if debug:
                        err.append(b"Phase flip detected in sample %d\n" % s)
                    can = False
                    break
            if can and debug:
                err.append(b"All phases consistent\n")
        if can:
            blocks[-1][2] = pos
            for s, g in enumerate(gts):
                blocks[-1][3][s].append(g)
        else:
            blocks.append([chrom, pos, pos, [[g] for g in gts]])
        last = gts
    if names is None:
        return (b"" if streaming else BARE_HEADER), b"".join(err), 0
    out = [b"\t".join([b"CHROM", b"START", b"END"] + names) + b"\n"]
    for chrom, start, end, haps in blocks:
        out.append(b"\t".join([chrom, b"%d" % start, b"%d" % end] + [b"|".join(h) for h in haps]) + b"\n")
    return b"".join(out), b"".join(err), 0


def run(argv, stdin=b"", cwd=None):
    """main :826-911: (stdout, stderr, rc)"""
    args = argv[1:]
    if "--help" in args or "-h" in args:  # vcfx::handle_common_flags
        return HELP, b"", 0
    if "--version" in args or "-v" in args:
        return VERSION, b"", 0
    opts, operands = getopt_long(argv)
    kw = dict(T=100000, check=False, streaming=False, quiet=False, debug=False)
    path, err = "", b""
    for k, v, msg in opts:
        err += msg
        if k == "h":
            return HELP, err, 0
        if k == "?":
            return HELP, err, 1
        if k == "i":
            path = v
        elif k == "b":
            kw["T"] = stoi(v)
            if kw["T"] is None:
                return b"", err + bad_block_size(v), 1
        else:
            kw[{"c": "check", "s": "streaming", "q": "quiet", "d": "debug"}[k]] = True
    if not path and operands:
        path = operands[0]
    if path:
        full = os.path.join(cwd, path) if cwd else path
        try:
            with open(full, "rb") as f:
                buf = f.read()
        except OSError:
            return b"", err + b"Error: could not open file: " + path.encode() + b"\n", 1
        if not buf:
            return b"", err + EMPTY_FILE, 1
        o, e, rc = extract(buf, False, **kw)
    else:
        o, e, rc = extract(stdin or b"", True, **kw)
    return o, err + e, rc


# ---- the device's view ---------------------------------------------------------------------------

def digits(v):
    return len(b"%d" % v)


def device_view(buf, stdin, T=100000, check=False):
    """The data part as the raw ABI sees it, or None when the tool never calls the device.  The data
    part starts at the first line that is neither skipped nor a '#' line.  A dict: start (its first
    byte), names, status / pos per line, member / block / flip per line (-1 off the members; flip = the
    first flipping sample of the pair (previous member, this one) that passed CHROM and distance, else
    ns), the block table (first and last member, start, end, row offset, row length), fixed (members
    that are fixed-stride) and text (the rows)."""
    lines = raw_lines(buf)
    names, k = None, 0
    while k < len(lines):
        body = body_of(lines[k], stdin)
        if body is None or body[:1] == b"#":
            if body is not None and names is None and body[:6] == b"#CHROM":
                names = body.split(b"\t")[9:]
                if not names:
                    return None
            k += 1
            continue
        break
    if k >= len(lines) or names is None:
        return None
    ns = len(names)
    v = dict(start=sum(len(ln) + 1 for ln in lines[:k]), names=names, status=[], pos=[], member=[], block=[], flip=[],
             blocks=[], fixed=[], text=b"")
    rows, last, last_pos, last_chrom, m = [], None, 0, None, 0
    for raw in lines[k:]:
        body = body_of(raw, stdin)
        if body is None or body[:1] == b"#":
            st, pos, gts = (EMPTY if body is None else HEADER), 0, None
        else:
            st, pos, chrom, gts = classify(body, ns)
        v["status"].append(st)
        v["pos"].append(pos)
        if st != MEMBER:
            v["member"].append(-1)
            v["block"].append(-1)
            v["flip"].append(-1)
            continue
        can = last is not None and chrom == last_chrom and pos - last_pos <= T
        flip = ns
        if can and check:
            flip = next((s for s in range(ns) if flips(last[s], gts[s])), ns)
            can = flip == ns
        if can:
            v["blocks"][-1][1] = m
            v["blocks"][-1][3] = pos
            for s in range(ns):
                rows[-1][1 + s].append(gts[s])
        else:
            v["blocks"].append([m, m, pos, pos, 0, 0])
            rows.append([chrom] + [[g] for g in gts])  # (the CHROM, then the samples)
        v["member"].append(m)
        v["block"].append(len(v["blocks"]) - 1)
        v["flip"].append(flip)
        v["fixed"].append(is_fixed(body, ns))
        last, last_pos, last_chrom = gts, pos, chrom
        m += 1
    off, text = 0, []
    for b, r in zip(v["blocks"], rows):
        chrom, haps = r[0], r[1:]
        row = b"\t".join([chrom, b"%d" % b[2], b"%d" % b[3]] + [b"|".join(h) for h in haps]) + b"\n"
        b[4], b[5] = off, len(row)
        off += len(row)
        text.append(row)
    v["text"] = b"".join(text)
    return v


# ---- golden cases --------------------------------------------------------------------------------

def load_cases():
    with gzip.open(os.path.join(GOLDEN, "haplotype_extractor_cases.json.gz"), "rb") as f:
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

COLS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"
NON_MEMBERS = (b"", b"#mid comment", b"1\t5\t.\tA\tC", b"chr1\t5x\t.\tA\tC\t.\t.\t.\tGT\t0|1", b"x")
LONG_GT = b"|".join(b"%d" % (i % 10) for i in range(150)) + b"|"  # 300 bytes


def chrom_line(ns):
    return b"\t".join([COLS] + [b"S%d" % i for i in range(ns)])


def record(chrom, pos, gts, fmt=b"GT", extra=None):
    """a data line; fmt's other keys get a number each"""
    keys = fmt.split(b":")
    cells = [b":".join(g if k == b"GT" else b"%d" % (7 + i) for i, k in enumerate(keys)) for g in gts]
    return b"\t".join([chrom, b"%d" % pos, b".", b"A", b"C", b".", b"PASS", b".", fmt] + cells + (extra or []))


def gen_gts(rnd, ns, widths):
    """ns phased GTs whose byte lengths are drawn from widths (1: "|", 3: "a|b", 4: "1a|b", 5: "a|b|c",
    300: LONG_GT)"""
    out = []
    for _ in range(ns):
        w = rnd.choice(widths)
        a, b, c = (b"%d" % rnd.randrange(2) for _ in range(3))
        out.append({1: b"|", 3: a + b"|" + b, 4: b"1" + a + b"|" + b, 5: a + b"|" + b + b"|" + c, 300: LONG_GT}[w])
    return out


def gen_blocks(seed, ns, lengths, widths=(3,), fmt=b"GT", between=0.0, crlf=False, final_newline=True, fixed_blocks=()):
    """a header and one run of members per entry of lengths: members of a run are 10 apart, runs
    200000 apart (further than the default block size) on alternating CHROMs.  between: the chance of
    a non-member line before each member; fixed_blocks: the runs whose GTs are all "a|b" whatever
    widths says"""
    rnd = random.Random(seed)
    eol = b"\r\n" if crlf else b"\n"
    out = [b"##fileformat=VCFv4.2", chrom_line(ns)]
    pos = 100
    for bi, n in enumerate(lengths):
        chrom = b"chr%d" % (1 + bi % 2)
        for _ in range(n):
            if rnd.random() < between:
                r = rnd.random()
                if r < 0.5:
                    out.append(rnd.choice(NON_MEMBERS))
                elif r < 0.75:
                    out.append(record(chrom, pos, [b"0/1"] * ns, fmt))  # unphased
                else:
                    out.append(record(chrom, pos, [b"0|1"] * ns, b"AD:DP"))  # no GT
            out.append(record(chrom, pos, gen_gts(rnd, ns, (3,) if bi in fixed_blocks else widths), fmt))
            pos += 10
        pos += 200000
    return eol.join(out) + (eol if final_newline else b"")


def gen_flips(ns, at, gap_lines=0, polyploid=False):
    """four members on one CHROM; the pair (1, 2) flips in the samples `at` ("0|1" then "1|0", or with
    polyploid "0|0|1" then "1|1|0"), with gap_lines non-members between them"""
    a, b = (b"0|0|1", b"1|1|0") if polyploid else (b"0|1", b"1|0")
    base = [a] * ns
    flipped = [b if s in at else a for s in range(ns)]
    out = [chrom_line(ns), record(b"1", 100, base), record(b"1", 110, base)]
    out += [NON_MEMBERS[1 + i % 4] for i in range(gap_lines)]
    out += [record(b"1", 120, flipped), record(b"1", 130, flipped)]
    return b"\n".join(out) + b"\n"


def bench_input(fmt=b"GT", records=20000, ns=2504, pool=32, seed=2026):
    """the measurement input (tools/hx_time.py): phased "a|b" records of ns samples, 100 apart"""
    rnd = random.Random(seed)
    recs = [record(b"chr1", 0, gen_gts(rnd, ns, (3,)), fmt).split(b"\t", 2)[2] for _ in range(pool)]
    out = [b"##fileformat=VCFv4.2\n" + chrom_line(ns) + b"\n"]
    out += [b"chr1\t%d\t%s\n" % (1000 + 100 * i, recs[i % pool]) for i in range(records)]
    return b"".join(out)
