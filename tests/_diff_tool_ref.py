"""VCFX_diff_tool restated in plain Python (VCFX_diff_tool.cpp): the line rule (parseVariantLine
:214-264), the key (generateVariantKey :168-200), the default mode (diffInMemoryMmap :333-404), the
sorted mode (compareChromNatural :269-307, compareKeys :312-328, diffStreamingMmap :409-506), the
CLI (run :705-761), and the input generators of the tests.  tests/test_diff_tool_ref.py holds it to
the compiled reference's recorded bytes (tests/golden/diff_tool_cases.json.gz);
tests/test_gpu_df.py checks the device against it.

The default mode here prints each side IN INPUT ORDER OF THE KEY'S FIRST LINE in that file, as the
drop-in does.  The reference prints each side in the iteration order of its C++ library's
unordered_set, so a recorded default-mode case whose sides hold more than one key (`ordered` false)
is compared by same_sections(): identical header lines and, per side, the same lines with no
repeats.  Every -s case and every other default-mode case is compared byte for byte.

Outside the domain (-s only): a POS or a natural-order digit prefix of more than 18 digits."""
import base64
import gzip
import json
import os
import random

TOOL = "VCFX_diff_tool"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HELP = (b"VCFX_diff_tool: Compare two VCF files and identify differences.\n\n"
        b"Usage:\n"
        b"  VCFX_diff_tool --file1 <file1.vcf> --file2 <file2.vcf> [options]\n\n"
        b"Options:\n"
        b"  -h, --help                Display this help message and exit\n"
        b"  -a, --file1 <file1.vcf>   Specify the first VCF file\n"
        b"  -b, --file2 <file2.vcf>   Specify the second VCF file\n"
        b"  -s, --assume-sorted       Assume inputs are sorted by (CHROM, POS).\n"
        b"                            Enables streaming mode with O(1) memory.\n"
        b"  -n, --natural-chr         Use natural chromosome ordering (chr1 < chr2 < chr10)\n"
        b"  -q, --quiet               Suppress warning messages\n\n"
        b"Modes:\n"
        b"  Default mode:     Loads both files into memory (works with unsorted files)\n"
        b"  Streaming mode:   Two-pointer merge diff with O(1) memory (requires sorted input)\n\n"
        b"Performance:\n"
        b"  Uses memory-mapped I/O with SIMD-accelerated parsing for ~20-50x speedup.\n\n"
        b"Example:\n"
        b"  VCFX_diff_tool --file1 file1.vcf --file2 file2.vcf\n"
        b"  VCFX_diff_tool -a sorted1.vcf -b sorted2.vcf --assume-sorted\n")
VERSION = b"VCFX_diff_tool version 1.1.4\n"

# vcfx_gpu.h VCFXG_DF_*
EMPTY, COMMON, UNIQUE, SKIPPED, HEADER, REPEAT = 0, 1, 2, 3, 4, 5
WINDOW = 64  # VCFXG_DF_WINDOW: the bytes of a line the device's lane path looks at
PATH_HASH, PATH_BOUNDS, PATH_WALK = 0, 1, 2

LONG = {"help": ("h", False), "file1": ("a", True), "file2": ("b", True), "assume-sorted": ("s", False),
        "natural-chr": ("n", False), "quiet": ("q", False)}
SHORT_OPTS = {"h": False, "a": True, "b": True, "s": False, "n": False, "q": False}
HDR = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def getopt_long(argv):
    """GNU getopt_long(argc, argv, "ha:b:snq", long_opts) with argument permutation:
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


# ---- lines and keys ----------------------------------------------------------------------------

def line_spans(buf):
    """[a, b) of every line: lines end at '\\n'; a final line without one still counts"""
    spans, a = [], 0
    while a < len(buf):
        b = buf.find(b"\n", a)
        if b < 0:
            b = len(buf)
        spans.append((a, b))
        a = b + 1
    return spans


def parse(line):
    """(status, fields): EMPTY / HEADER / SKIPPED with None, or None with (CHROM, POS, REF, ALT)"""
    if not line:
        return EMPTY, None
    if line[:1] == b"#":
        return HEADER, None
    if line[-1:] == b"\r":
        line = line[:-1]
    f = line.split(b"\t")
    if len(f) < 5:  # CHROM, POS, ID and REF each end at a tab
        return SKIPPED, None
    if any(not 48 <= c <= 57 for c in f[1]):  # an empty POS passes
        return SKIPPED, None
    return None, (f[0], f[1], f[3], f[4])


def key(chrom, pos, ref, alt):
    """CHROM:POS:REF:ALT', ALT's tokens (empty ones kept) as unsigned bytes, a prefix first"""
    return b":".join((chrom, pos, ref, b",".join(sorted(alt.split(b",")))))


def natural_parts(chrom):
    """compareChromNatural's view: (has a digit prefix, its value, the rest)"""
    if chrom[:3] in (b"chr", b"Chr", b"CHR"):
        chrom = chrom[3:]
    k = 0
    while k < len(chrom) and 48 <= chrom[k] <= 57:
        k += 1
    return (k > 0, int(chrom[:k]) if k else -1, chrom[k:])


def sort_key(fields, natural):
    """compareKeys as a tuple: equal tuples compare equal there, smaller ones less"""
    chrom, pos, ref, alt = fields
    if natural:
        has, val, rest = natural_parts(chrom)
        c = (0, val, rest) if has else (1, 0, rest)
    else:
        c = (chrom,)
    return (c, int(pos) if pos else 0, ref, alt)


def join(f1, f2):
    """the one text the device indexes, and where file 2 begins in it"""
    pad = b"\n" if f1 and f1[-1:] != b"\n" else b""
    return f1 + pad + f2, len(f1) + len(pad)


def lane_path(line):
    """the line is settled by the key kernel's lane pass: it is empty, a '#' line, no longer than the
    window, or its fifth tab lies inside the window"""
    return not line or line[:1] == b"#" or len(line) <= WINDOW or line[:WINDOW].count(b"\t") >= 5


def diff(f1, f2, assume_sorted=False, natural=False):
    """(statuses of the joined text's lines, side 1's printed keys, side 2's, the device path, the
    cut line, the number of lines off the lane path)"""
    buf, second = join(f1, f2)
    spans = line_spans(buf)
    cut = sum(1 for a, _ in spans if a < second)
    st, data = [], ([], [])  # data: (line number, fields, key) per side
    for i, (a, b) in enumerate(spans):
        s, f = parse(buf[a:b])
        st.append(s)
        if s is None:
            data[i >= cut].append((i, f, key(*f)))
    out = ([], [])
    if not assume_sorted:
        path = PATH_HASH
        sets = [set(k for _, _, k in d) for d in data]
        for side in (0, 1):
            seen = set()
            for i, _, k in data[side]:
                if k in seen:
                    st[i] = REPEAT
                elif k in sets[1 - side]:
                    st[i] = COMMON
                else:
                    st[i] = UNIQUE
                    out[side].append(k)
                seen.add(k)
    else:
        keys = [[sort_key(f, natural) for _, f, _ in d] for d in data]
        ordered = all(k[j] <= k[j + 1] for k in keys for j in range(len(k) - 1))
        path = PATH_BOUNDS if ordered else PATH_WALK
        p = [0, 0]
        while p[0] < len(data[0]) and p[1] < len(data[1]):
            a, b = keys[0][p[0]], keys[1][p[1]]
            if a < b:
                st[data[0][p[0]][0]] = UNIQUE
                p[0] += 1
            elif a > b:
                st[data[1][p[1]][0]] = UNIQUE
                p[1] += 1
            else:
                st[data[0][p[0]][0]] = st[data[1][p[1]][0]] = COMMON
                p[0] += 1
                p[1] += 1
        for side in (0, 1):
            for i, _, _ in data[side][p[side]:]:
                st[i] = UNIQUE
            out[side].extend(k for i, _, k in data[side] if st[i] == UNIQUE)
        if ordered:  # the multiset rule the bounds kernel applies gives the walk's answer
            for side in (0, 1):
                for j, (i, _, _) in enumerate(data[side]):
                    occ = j - keys[side].index(keys[side][j])
                    assert (st[i] == UNIQUE) == (occ >= keys[1 - side].count(keys[side][j]))
    waves = sum(not lane_path(buf[a:b]) for a, b in spans)
    return st, out[0], out[1], path, cut, waves


def output(path1, path2, side1, side2):
    return b"Variants unique to " + path1.encode() + b":\n" + b"".join(k + b"\n" for k in side1) + \
        b"\nVariants unique to " + path2.encode() + b":\n" + b"".join(k + b"\n" for k in side2)


def read_input(path, cwd=None):
    """the file's bytes as the drop-in reads them (gzip input inflated unless VCFX_GZIP=0), None when
    it cannot be opened or mapped"""
    full = os.path.join(cwd, path) if cwd else path
    if os.path.isdir(full):
        return None
    try:
        with open(full, "rb") as f:
            data = f.read()
    except OSError:
        return None
    if data[:2] == b"\x1f\x8b" and os.environ.get("VCFX_GZIP", "1")[:1] != "0":
        data = gzip.decompress(data)
    return data


def run(argv, cwd=None):
    """the tool's (stdout, stderr, exit code)"""
    if "--help" in argv[1:] or "-h" in argv[1:]:
        return HELP, b"", 0
    if "--version" in argv[1:] or "-v" in argv[1:]:
        return VERSION, b"", 0
    opts, _ = getopt_long(argv)
    err = b"".join(m for _, _, m in opts)
    got = {}
    for k, v, _ in opts:
        got[k] = v
    help_ = "h" in got or "?" in got
    if help_ or not got.get("a") or not got.get("b"):
        return HELP, err, 0 if help_ else 1
    files = []
    for p in (got["a"], got["b"]):
        data = read_input(p, cwd)
        if data is None:
            return b"", err + b"Error: Unable to open file " + p.encode() + b"\n", 1
        files.append(data)
    _, s1, s2, _, _, _ = diff(files[0], files[1], "s" in got, "n" in got)
    return output(got["a"], got["b"], s1, s2), err, 0


def sections(out):
    """(header 1, side 1's lines, header 2, side 2's lines) of an output, None when it has another shape"""
    lines = out.split(b"\n")
    if not out.endswith(b"\n") or not lines[0].startswith(b"Variants unique to "):
        return None
    lines.pop()
    cuts = [i for i in range(1, len(lines) - 1) if lines[i] == b"" and lines[i + 1].startswith(b"Variants unique to ")]
    if len(cuts) != 1:
        return None
    c = cuts[0]
    return lines[0], lines[1:c], lines[c + 1], lines[c + 2:]


def same_sections(got, want):
    """identical header lines and, per side, the same lines with no repeats (a key holds no '\\n'
    in the compared cases)"""
    g, w = sections(got), sections(want)
    if g is None or w is None or g[0] != w[0] or g[2] != w[2]:
        return False
    return all(len(set(g[k])) == len(g[k]) == len(w[k]) and set(g[k]) == set(w[k]) for k in (1, 3))


def load_cases():
    with gzip.open(os.path.join(GOLDEN, "diff_tool_cases.json.gz"), "rb") as f:
        cases = json.loads(f.read())["cases"]
    for c in cases:
        c["stdout"] = base64.b64decode(c["stdout"])
        c["stderr"] = base64.b64decode(c["stderr"])
    return cases


# ---- generators --------------------------------------------------------------------------------

REST = b"50\tPASS\tDP=7"


def rec(chrom, pos, ref=b"A", alt=b"T", id_=b"."):
    return b"\t".join((chrom, pos, id_, ref, alt, REST))


def gen_lines(seed, n, chroms=(b"1", b"2", b"chr3", b"X"), span=40):
    """n data lines over few keys (so that files share and repeat them), ALT of one to three tokens"""
    rnd = random.Random(seed)
    alts = (b"T", b"G", b"C,T", b"T,C", b"G,C,T", b"<DEL>", b"", b"T,")
    return [rec(rnd.choice(chroms), b"%d" % rnd.randrange(1, span), rnd.choice((b"A", b"AC", b"")), rnd.choice(alts),
                b"id%d" % i) for i in range(n)]


def gen_file(seed, n, mix=False, final_newline=True, ordered=False, natural=False, **kw):
    lines = gen_lines(seed, n, **kw)
    if ordered:
        lines.sort(key=lambda l: sort_key(parse(l)[1], natural))
    if mix and lines:
        rnd = random.Random(seed + 1)
        for extra in (b"", b"#comment", b"short\t1\t.", b"1\tx5\t.\tA\tT", b"\r"):
            for _ in range(3):
                lines.insert(rnd.randrange(len(lines) + 1), extra)
    buf = HDR + b"\n".join(lines) + b"\n"
    return buf if final_newline else buf[:-1]
