"""VCFX_sorter restated in plain Python (VCFX_sorter.cpp): the CLI, the file mode (sortFileMmap
:321-459), the stdin mode (sortExternal :601-674), chromToId (:43-146), and the input generators
of the tests.  tests/test_sorter_ref.py holds it to the compiled reference's recorded bytes
(tests/golden/sorter_cases.json.gz); tests/test_gpu_srt.py checks the device against it.

The sort here is STABLE: lines with equal keys keep their input order.  The reference's std::sort
and priority_queue leave them in whatever order its C++ library does (stable up to 16 kept lines
with libstdc++), so its bytes equal these whenever no two kept lines share a key or at most 16
lines are kept; a case that has ties among 17 or more kept lines (the fixtures named ties_*) is
compared by same_up_to_ties(): the same header block, the same key sequence, the same lines inside
every run of equal keys.

Outside the domain: a non-numeric -m, an unwritable -t, a digit run in CHROM (natural order) or a
stdin POS past what int holds where the reference's own arithmetic is undefined."""
import base64
import gzip
import json
import os
import random

TOOL = "VCFX_sorter"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HELP = (b"VCFX_sorter: Sort a VCF by chromosome and position.\n\n"
        b"Usage:\n"
        b"  VCFX_sorter [options] [input.vcf] > output.vcf\n"
        b"  VCFX_sorter [options] < input.vcf > output.vcf\n\n"
        b"Options:\n"
        b"  -h, --help              Show help.\n"
        b"  -n, --natural-chr       Use natural chromosome order (chr1 < chr2 < chr10).\n"
        b"  -m, --max-memory <MB>   Max memory for in-memory sorting (default: 100MB).\n"
        b"                          Files larger than this use external merge sort.\n"
        b"  -t, --temp-dir <DIR>    Directory for temporary files (default: /tmp).\n\n"
        b"Description:\n"
        b"  Sorts VCF by (CHROM, POS). For small files, sorts in memory.\n"
        b"  For large files (>max-memory), uses external merge sort with\n"
        b"  temporary files, enabling sorting of files larger than RAM.\n\n"
        b"  When a file argument is provided, uses memory-mapped I/O for\n"
        b"  optimal performance (26x faster than stdin processing).\n\n"
        b"Performance:\n"
        b"  - File argument with mmap: ~30 seconds for 1GB files\n"
        b"  - Stdin processing: ~10 minutes for 1GB files\n"
        b"  - Uses pre-computed chromosome IDs for O(1) comparisons\n"
        b"  - Compact 20-byte sort keys (vs 9KB per variant)\n\n"
        b"Examples:\n"
        b"  1) Fast file sorting (recommended):\n"
        b"     VCFX_sorter input.vcf > sorted.vcf\n"
        b"  2) Stdin processing (slower):\n"
        b"     VCFX_sorter < input.vcf > sorted.vcf\n"
        b"  3) Natural chromosome order:\n"
        b"     VCFX_sorter -n input.vcf > sorted.vcf\n"
        b"  4) Large file with custom temp directory:\n"
        b"     VCFX_sorter -t /data/tmp input.vcf > sorted.vcf\n")
VERSION = b"VCFX_sorter version 1.1.4\n"
WARN_PRE = b"Warning: data line before #CHROM => skipping.\n"
WARN_BAD = b"Warning: skipping malformed line.\n"

# vcfx_gpu.h VCFXG_SRT_*
EMPTY, KEPT, PRE, BAD, HEADER = 0, 1, 2, 3, 4
WINDOW = 64  # VCFXG_SRT_WINDOW: the bytes of a line the device's lane path looks at

LONG = {"help": False, "natural-chr": False, "max-memory": True, "temp-dir": True}
SHORT_OPTS = {"h": False, "n": False, "m": True, "t": True}
SPACE = b" \t\n\v\f\r"


def getopt_long(argv):
    """GNU getopt_long(argc, argv, "hnm:t:", long_opts) with argument permutation:
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
                    opts.append((k[0], val, b""))
                elif i < len(argv):
                    opts.append((k[0], argv[i], b""))
                    i += 1
                else:
                    opts.append(("?", None, prog + b": option '--" + k.encode() + b"' requires an argument\n"))
            elif eq:
                opts.append(("?", None, prog + b": option '--" + k.encode() + b"' doesn't allow an argument\n"))
            else:
                opts.append((k[0], None, b""))
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


# ---- the key -------------------------------------------------------------------------------------

def i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def _upper(b):
    return b - 32 if 97 <= b <= 122 else b


def _suffix_hash(bs):
    h = 0
    for b in bs:
        h = i32(h * 31 + b)
    return (h & 0x7FFF) + 1


def chrom_to_id(c):
    """chromToId(chrom, len, naturalOrder = true) :43-146, int arithmetic wrapping at 32 bits"""
    if not c:
        return 999999
    p, prefix = c, False
    if len(c) >= 3 and c[0] in b"cC" and c[1] in b"hH" and c[2] in b"rR":
        p, prefix = c[3:], True
    if not p:
        return 999999
    num = nd = 0
    while nd < len(p) and 48 <= p[nd] <= 57:
        num = i32(num * 10 + (p[nd] - 48))
        nd += 1
    sh = _suffix_hash(p[nd:nd + 8]) if nd < len(p) else 0
    base = off = 0
    if prefix:
        base = 5000000
        off = 10000 if c[:3] == b"CHR" else 20000 if c[:2] == b"Ch" else 30000
    if nd > 0 and 1 <= num <= 22:
        return i32(base + num * 100000 + off + sh)
    if nd == 0:
        u0 = _upper(p[0])
        if len(p) >= 2 and u0 == 77 and _upper(p[1]) == 84:  # MT
            if len(p) > 2:
                sh = _suffix_hash(p[2:10])
            return base + 2300000 + off + sh
        if len(p) == 1 and u0 in (77, 88, 89):
            return base + {77: 2300000, 88: 2400000, 89: 2500000}[u0] + off + sh
    h = 3000000
    for b in c[:16]:
        h = (h * 31 + b) & 0xFFFFFFFF
    return i32(base + (h & 0x3FFFFFFF) + 3000000)


def pos_file(line, tab):
    """parseChromPosFast :249-270: the digits after the first tab in a wrapping int; None when that
    is 0.  (The source says `pos > 0`; the compiled reference keeps a value that wrapped negative and
    sorts it as a negative int: its compiler knows a sum of digits cannot be negative.)"""
    v, p = 0, tab + 1
    while p < len(line) and 48 <= line[p] <= 57:
        v = i32(v * 10 + (line[p] - 48))
        p += 1
    return v if v != 0 else None


def stoi(f):
    """std::stoi of the field: None when it throws (no digits, outside int)"""
    p = 0
    while p < len(f) and f[p] in SPACE:
        p += 1
    neg = False
    if p < len(f) and f[p] in b"+-":
        neg = f[p:p + 1] == b"-"
        p += 1
    q = p
    while q < len(f) and 48 <= f[q] <= 57:
        q += 1
    if q == p:
        return None
    v = int(f[p:q])
    v = -v if neg else v
    return v if -(1 << 31) <= v < (1 << 31) else None


def line_spans(buf):
    """[ls, le) of every line: they end at '\\n' only; a final line without one counts"""
    spans, p, n = [], 0, len(buf)
    while p < n:
        e = buf.find(b"\n", p)
        if e < 0:
            e = n
        spans.append((p, e))
        p = e + 1
    return spans


def data_key(line, stdin, natural):
    """the sort key of a data line, None for a malformed one"""
    t0 = line.find(b"\t")
    if t0 < 0:
        return None
    if stdin:
        t1 = line.find(b"\t", t0 + 1)
        if t1 < 0:
            return None
        pos = stoi(line[t0 + 1:t1])
    else:
        pos = pos_file(line, t0)
    if pos is None:
        return None
    chrom = line[:t0]
    if natural:
        return (chrom_to_id(chrom), pos)
    # (stdin mode: chromToId gives an empty CHROM 999999 before the mode check, compareById :307-316)
    return (1 if stdin and not chrom else 0, chrom, pos)


def statuses(buf, stdin, natural=False):
    """per line its VCFXG_SRT_* status and (kept lines) its key"""
    st, keys, found = [], [], False
    for ls, le in line_spans(buf):
        line = buf[ls:le]
        k = None
        if not line:
            s = EMPTY
        elif line[:1] == b"#":
            s = HEADER
            found = found or line[:6] == b"#CHROM"
        elif not stdin and not found:
            s = PRE
        else:
            k = data_key(line, stdin, natural)
            s = BAD if k is None else KEPT
        st.append(s)
        keys.append(k)
    return st, keys


def order(buf, stdin, natural=False):
    """the input line number of every output line: the header lines (stdin mode: and the empty
    ones) in input order, then the kept lines by key, equal keys in input order"""
    st, keys = statuses(buf, stdin, natural)
    head = [i for i, s in enumerate(st) if s == HEADER or (stdin and s == EMPTY)]
    kept = sorted((i for i, s in enumerate(st) if s == KEPT), key=lambda i: keys[i])
    return head + kept


def sort_bytes(buf, stdin, natural=False):
    """(stdout, stderr, rc) of one input"""
    if not buf:
        return b"", b"", 0
    st, _ = statuses(buf, stdin, natural)
    spans = line_spans(buf)
    out = b"".join(buf[spans[i][0]:spans[i][1]] + b"\n" for i in order(buf, stdin, natural))
    err = b"".join(WARN_PRE if s == PRE else WARN_BAD for s in st if s in (PRE, BAD))
    return out, err, 0


def run(argv, stdin=b"", cwd=None):
    """main :753-761 and run :676-743: (stdout, stderr, rc)"""
    args = argv[1:]
    if "--help" in args or "-h" in args:  # vcfx::handle_common_flags
        return HELP, b"", 0
    if "--version" in args or "-v" in args:
        return VERSION, b"", 0
    opts, operands = getopt_long(argv)
    natural, help_, err = False, False, b""
    for k, v, msg in opts:
        err += msg
        if k == "n":
            natural = True
        elif k in ("m", "t"):
            pass
        else:
            help_ = True
    if help_:
        return HELP, err, 0
    if operands:
        out = b""
        for path in operands:
            full = os.path.join(cwd, path) if cwd else path
            try:
                with open(full, "rb") as f:
                    buf = f.read()
            except OSError:
                return out, err + b"Error: cannot open file '" + path.encode() + b"'\n", 1
            o, e, _ = sort_bytes(buf, False, natural)
            out += o
            err += e
        return out, err, 0
    o, e, rc = sort_bytes(stdin or b"", True, natural)
    return o, err + e, rc


def split_output(out, stdin, natural):
    """(header block bytes, [(key, line)] of the data lines) of a sorter output"""
    lines = out.split(b"\n")
    assert lines[-1] == b"", "output does not end in a newline"
    lines = lines[:-1]
    h = 0
    while h < len(lines) and (not lines[h] or lines[h][:1] == b"#"):
        h += 1
    head = b"".join(x + b"\n" for x in lines[:h])
    return head, [(data_key(x, stdin, natural), x) for x in lines[h:]]


def same_up_to_ties(a, b, stdin, natural):
    """the weaker rule of the ties_* cases: the same header block, the same key sequence and the
    same multiset of lines inside every run of equal keys"""
    ha, da = split_output(a, stdin, natural)
    hb, db = split_output(b, stdin, natural)
    if ha != hb or [k for k, _ in da] != [k for k, _ in db] or any(k is None for k, _ in da):
        return False
    i = 0
    while i < len(da):
        j = i
        while j < len(da) and da[j][0] == da[i][0]:
            j += 1
        if sorted(x for _, x in da[i:j]) != sorted(x for _, x in db[i:j]):
            return False
        i = j
    return True


def tie_profile(buf, stdin, natural):
    """(kept lines, kept lines whose key another kept line shares)"""
    st, keys = statuses(buf, stdin, natural)
    kept = [k for s, k in zip(st, keys) if s == KEPT]
    seen = {}
    for k in kept:
        seen[k] = seen.get(k, 0) + 1
    return len(kept), sum(v for v in seen.values() if v > 1)


# ---- golden cases --------------------------------------------------------------------------------

def load_cases():
    with gzip.open(os.path.join(GOLDEN, "sorter_cases.json.gz"), "rb") as f:
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


def case_mode(case):
    """(stdin mode, natural order) of a recorded sort"""
    opts, operands = getopt_long(case["argv"])
    return not operands, any(k == "n" for k, _, _ in opts)


# ---- generated inputs ----------------------------------------------------------------------------

HDR = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
CHROMS = (b"1", b"2", b"10", b"22", b"X", b"Y", b"MT", b"chr1", b"chr2", b"chr10", b"chrX", b"chrM", b"GL000220.1")


def record(chrom, pos, id_=b".", rest=b"A\tC\t50\tPASS\tDP=7"):
    return b"\t".join([chrom, pos, id_, rest])


def gen_vcf(seed, n, ties=False, mix=False, header=True, final_newline=True, chroms=CHROMS, pad=0):
    """n data lines in random order, every one with its own ID.  ties False: no two lines share
    (CHROM, POS) nor (chromToId, POS); ties True: positions drawn from a few values, so most lines
    share their key with others.  mix: '#' lines, empty lines and malformed lines in between.  pad:
    up to that many extra bytes in INFO (varied line lengths)."""
    rnd = random.Random(seed)
    lines, used = [], set()
    while len(lines) < n:
        c = rnd.choice(chroms)
        p = rnd.randrange(1, 9 if ties else 1000000)
        k = (chrom_to_id(c), p)
        if not ties:
            if k in used or (c, p) in used:
                continue
            used.add(k)
            used.add((c, p))
        info = b"DP=%d" % rnd.randrange(100) + (b";X=" + b"x" * rnd.randrange(pad) if pad else b"")
        lines.append(record(c, b"%d" % p, b"id%d" % len(lines), b"A\tC\t50\tPASS\t" + info))
    out = []
    for ln in lines:
        if mix:
            r = rnd.random()
            if r < 0.05:
                out.append(b"")
            elif r < 0.10:
                out.append(b"#comment %d" % len(out))
            elif r < 0.14:
                out.append(rnd.choice((b"1", b"x\ty", b"1\t\t.", b"1\tabc\t.", b"1\t+\t.")))  # (malformed in both modes)
        out.append(ln)
    return (HDR if header else b"") + b"\n".join(out) + (b"\n" if final_newline and out else b"")


# the generated inputs the GPU tests use: name -> gen_vcf arguments
GENERATED = {
    "n1": dict(seed=1, n=1), "n2": dict(seed=2, n=2),
    "n16": dict(seed=16, n=16), "n17": dict(seed=17, n=17),
    "n255": dict(seed=255, n=255), "n256": dict(seed=256, n=256),
    "n257": dict(seed=257, n=257), "n4097": dict(seed=4097, n=4097, pad=40),
    "mix": dict(seed=7, n=500, mix=True), "mix_ties": dict(seed=8, n=500, mix=True, ties=True),
    "routes": dict(seed=10, n=2000, mix=True, pad=300),
}


def generated(name):
    return gen_vcf(**GENERATED[name])
