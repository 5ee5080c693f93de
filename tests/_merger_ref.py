"""VCFX_merger restated in plain Python (VCFX_merger.cpp): the CLI (run :94-148), the line rules
(parseChromPos :77-92 with std::stol), both comparators (:17-40, :223-248 with parseChromNat :43-74),
the default mode (mergeVCFInMemory :176-254) as a STABLE sort, the -s mode (mergeVCFStreaming
:257-345) as the heap process that pops the EARLIEST FILE among equal least heads, the status of
every line of the joined text, and a tie detector.  tests/test_merger_ref.py holds it to the compiled
reference's recorded bytes (tests/golden/merger_cases.json.gz); tests/test_gpu_mg.py checks the
device against it.

Equal keys: the reference leaves them to std::sort and to its heap; the drop-in and this file put
them in (file list order, line order).  A recorded case that may hold equal keys (`ordered` false:
the ties_* cases) is compared by same_under_ties(): the same header, the same key sequence and the
same multiset of lines in every run of equal keys.  Every other case is compared byte for byte.

Outside the domain: -n with a CHROM digit run of more than 18 digits."""
import base64
import gzip
import json
import os
import random

TOOL = "VCFX_merger"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HELP = (b"VCFX_merger: Merge multiple VCF files by variant position.\n\n"
        b"Usage:\n"
        b"  VCFX_merger --merge file1.vcf,file2.vcf,... [options]\n\n"
        b"Options:\n"
        b"  -m, --merge          Comma-separated list of VCF files to merge\n"
        b"  -s, --assume-sorted  Assume input files are already sorted (enables streaming\n"
        b"                       merge with O(num_files) memory for large files)\n"
        b"  -n, --natural-chr    Use natural chromosome order (chr1 < chr2 < chr10)\n"
        b"  -h, --help           Display this help message and exit\n\n"
        b"Description:\n"
        b"  By default, loads all variants into memory and sorts them. This works for\n"
        b"  small to medium files but may run out of memory for very large files.\n\n"
        b"  With --assume-sorted, uses streaming K-way merge that only keeps one line\n"
        b"  per input file in memory. This enables merging files larger than RAM.\n"
        b"  Input files MUST be sorted by (CHROM, POS) for correct results.\n\n"
        b"Examples:\n"
        b"  # Default mode (loads all into memory, sorts)\n"
        b"  VCFX_merger --merge sample1.vcf,sample2.vcf > merged.vcf\n\n"
        b"  # Streaming mode for large pre-sorted files\n"
        b"  VCFX_merger --merge sorted1.vcf,sorted2.vcf --assume-sorted > merged.vcf\n\n"
        b"  # With natural chromosome ordering\n"
        b"  VCFX_merger --merge f1.vcf,f2.vcf --assume-sorted -n > merged.vcf\n")
VERSION = b"VCFX_merger version 1.1.4\n"

# vcfx_gpu.h VCFXG_MG_*
EMPTY, KEPT, BAD, HEADER, DROPPED = 0, 1, 2, 3, 4
WINDOW = 64  # VCFXG_MG_WINDOW: the bytes of a line the device's lane path looks at
PATH_SORT, PATH_WALK = 0, 1

LONG = {"merge": ("m", True), "assume-sorted": ("s", False), "natural-chr": ("n", False), "help": ("h", False)}
SHORT_OPTS = {"m": True, "s": False, "n": False, "h": False}
HDR = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def getopt_long(argv):
    """GNU getopt_long(argc, argv, "m:snh", long_opts) with argument permutation:
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


def stol(field):
    """std::stol: C white space, one sign, decimal digits, the rest ignored; None when it throws"""
    i = 0
    while i < len(field) and field[i] in b" \t\n\v\f\r":
        i += 1
    neg = False
    if i < len(field) and field[i] in b"+-":
        neg = field[i] == 0x2D
        i += 1
    j = i
    while j < len(field) and 48 <= field[j] <= 57:
        j += 1
    if j == i:
        return None
    v = int(field[i:j])
    v = -v if neg else v
    return v if -2 ** 63 <= v <= 2 ** 63 - 1 else None


def parse(line):
    """(status, CHROM, POS): EMPTY, a '#' line as HEADER, BAD, or KEPT with its fields"""
    if not line:
        return EMPTY, None, None
    if line[:1] == b"#":
        return HEADER, None, None
    f = line.split(b"\t", 2)
    if len(f) < 3:
        return BAD, None, None
    pos = stol(f[1])
    if pos is None:
        return BAD, None, None
    return KEPT, f[0], pos


def nat_parts(chrom):
    """parseChromNat: (prefix as written, 0 numeric / 1 not, num, suffix)"""
    prefix = b""
    if chrom[:3].upper() == b"CHR" and len(chrom) >= 3:
        prefix, chrom = chrom[:3], chrom[3:]
    k = 0
    while k < len(chrom) and 48 <= chrom[k] <= 57:
        k += 1
    return (prefix, 0, int(chrom[:k]), chrom[k:]) if k else (prefix, 1, 0, chrom)


def sort_key(chrom, pos, natural):
    """the comparators as a tuple: equal tuples compare equal there, smaller ones less"""
    return (nat_parts(chrom), pos) if natural else (chrom, pos)


def join(files):
    """the one text the device indexes and the len(files) + 1 offsets where the files begin"""
    text, starts = b"", []
    for f in files:
        starts.append(len(text))
        text += f + (b"\n" if f and f[-1:] != b"\n" else b"")
    return text, starts + [len(text)]


def lane_path(line):
    """the line is settled by the key kernel's lane pass: it is empty, a '#' line, no longer than the
    window, or its second tab lies inside the window"""
    return not line or line[:1] == b"#" or len(line) <= WINDOW or line[:WINDOW].count(b"\t") >= 2


class Merged:
    """what merge() found: statuses per line of the joined text, order (the input line of every
    output line), text, path, hdr (the header's file, len(files) without one), bad per file,
    first_line per file (+ the line count), waves (lines off the lane path), ties (equal keys met:
    two kept lines in the default mode, two least heads at a pop under -s), keys (the output data
    lines' keys)"""


def merge(files, assume_sorted=False, natural=False):
    buf, starts = join(files)
    K = len(files)
    spans = line_spans(buf)
    first_line = [sum(1 for a, _ in spans if a < s) for s in starts]
    file_of = [max(f for f in range(K) if first_line[f] <= i) for i in range(len(spans))] if K else []
    st, key = [], {}
    for i, (a, b) in enumerate(spans):
        s, chrom, pos = parse(buf[a:b])
        st.append(s)
        if s == KEPT:
            key[i] = sort_key(chrom, pos, natural)
    # the header: per file its '#' lines (-s: those before its first line that is neither empty nor '#')
    hdr, header = K, []
    for f in range(K):
        cand = []
        for i in range(first_line[f], first_line[f + 1]):
            if st[i] == HEADER:
                cand.append(i)
            elif st[i] != EMPTY and assume_sorted:
                break
        if cand:
            hdr, header = f, cand
            break
    keep = set(header)
    for i, s in enumerate(st):
        if s == HEADER and i not in keep:
            st[i] = DROPPED
    per_file = [[i for i in range(first_line[f], first_line[f + 1]) if st[i] == KEPT] for f in range(K)]
    ordered = all(key[l[j]] <= key[l[j + 1]] for l in per_file for j in range(len(l) - 1))
    m = Merged()
    m.path = PATH_WALK if assume_sorted and not ordered else PATH_SORT
    ties = False
    if not assume_sorted:
        data = sorted((i for l in per_file for i in l), key=lambda i: key[i])  # (stable)
        ties = len(set(key.values())) != len(key)
    else:
        data, cur = [], [0] * K
        while True:
            heads = [(key[per_file[f][cur[f]]], f) for f in range(K) if cur[f] < len(per_file[f])]
            if not heads:
                break
            k, f = min(heads)  # the least key, the earliest file among equals
            ties = ties or sum(1 for h in heads if h[0] == k) > 1
            data.append(per_file[f][cur[f]])
            cur[f] += 1
        if ordered:
            assert data == sorted((i for l in per_file for i in l), key=lambda i: key[i])
    m.statuses, m.order, m.hdr, m.ties = st, header + data, hdr, ties
    m.text = b"".join(buf[spans[i][0]:spans[i][1]] + b"\n" for i in m.order)
    m.bad = [sum(1 for i in range(first_line[f], first_line[f + 1]) if st[i] == BAD) for f in range(K)]
    m.first_line = first_line
    m.file_of = file_of
    m.waves = sum(not lane_path(buf[a:b]) for a, b in spans)
    m.keys = [key[i] for i in data]
    m.counts = tuple(st.count(s) for s in range(5)) + (m.waves, m.path, hdr)
    return m


def split_names(values):
    """every -m value split at every comma, all appended; empty names kept"""
    names = []
    for v in values:
        names += v.split(",")
    return names


def read_input(path, cwd=None):
    """the file's bytes as the drop-in reads them (a directory: no bytes; gzip input inflated unless
    VCFX_GZIP=0), None when it cannot be opened"""
    full = os.path.join(cwd, path) if cwd else path
    if path and os.path.isdir(full):
        return b""
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
    letters = [k for k, _, _ in opts]
    names = split_names([v for k, v, _ in opts if k == "m"])
    if "h" in letters or "?" in letters or not names:
        return HELP, err, 0
    assume_sorted, natural = "s" in letters, "n" in letters
    data = [read_input(p, cwd) for p in names]
    m = merge([d for d in data if d is not None], assume_sorted, natural)
    k = 0
    for p, d in zip(names, data):
        if d is None:
            err += b"Failed to open file: " + p.encode() + b"\n"
            continue
        if not assume_sorted:
            err += (b"Warning: skipping malformed line in " + p.encode() + b"\n") * m.bad[k]
        k += 1
    return m.text, err, 0


def out_parts(out, natural):
    """(the leading '#' lines, [(key, line)] of the rest) of an output; None when a line is no data line"""
    lines = out.split(b"\n")
    if lines.pop() != b"":
        return None
    h = 0
    while h < len(lines) and lines[h][:1] == b"#":
        h += 1
    rest = []
    for l in lines[h:]:
        s, chrom, pos = parse(l)
        if s != KEPT:
            return None
        rest.append((sort_key(chrom, pos, natural), l))
    return lines[:h], rest


def same_under_ties(got, want, natural):
    """the same header, the same key sequence, and in every run of equal keys the same multiset of lines"""
    g, w = out_parts(got, natural), out_parts(want, natural)
    if g is None or w is None or g[0] != w[0] or [k for k, _ in g[1]] != [k for k, _ in w[1]]:
        return False
    runs = {}
    for sign, part in ((1, g[1]), (-1, w[1])):
        for k, l in part:
            runs[(k, l)] = runs.get((k, l), 0) + sign
    return not any(runs.values())


def load_cases():
    with gzip.open(os.path.join(GOLDEN, "merger_cases.json.gz"), "rb") as f:
        cases = json.loads(f.read())["cases"]
    for c in cases:
        c["stdout"] = base64.b64decode(c["stdout"])
        c["stderr"] = base64.b64decode(c["stderr"])
    return cases


# ---- generators --------------------------------------------------------------------------------

REST = b".\tA\tT\t50\tPASS\tDP=7"


def rec(chrom, pos, tag=b""):
    """a data line; pos: bytes as written"""
    return chrom + b"\t" + pos + b"\t" + REST + tag


def gen_records(seed, n, chroms=(b"1", b"2", b"10", b"chr3", b"chrX", b"X", b"MT"), span=10 ** 6, tag=b""):
    """n data lines with distinct (CHROM, POS) pairs"""
    rnd = random.Random(seed)
    seen, out = set(), []
    while len(out) < n:
        c, p = rnd.choice(chroms), rnd.randrange(1, span)
        if (c, p) not in seen:
            seen.add((c, p))
            out.append(rec(c, b"%d" % p, tag))
    return out


def deal(lines, k, natural=None, header=HDR):
    """the lines dealt round-robin into k files with the header; natural not None: each file sorted"""
    files = []
    for f in range(k):
        part = lines[f::k]
        if natural is not None:
            part = sorted(part, key=lambda l: sort_key(*parse(l)[1:], natural))
        files.append(header + b"".join(l + b"\n" for l in part))
    return files
