"""A plain-Python restatement of VCFX_field_extractor, written from its behaviour: both of its modes
(file mode: -i FILE or a positional FILE; stdin mode: no file, or "-"), which disagree in the '\\r'
strip, in what an empty value prints, in which of two equal INFO keys wins and in whether INFO is asked
before a sample field.  tests/test_field_extractor_ref.py holds it to the golden cases recorded from
the compiled reference; the GPU tests then use it as their checker.  Everything is computed as the
matrix of cells first (cells()), and the text is made from the cells, so the two cannot disagree.

Also here: the fixture generators the golden script and the GPU tests share."""
import base64
import gzip
import json
import os
import random

TOOL = "VCFX_field_extractor"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HELP = (b"VCFX_field_extractor\n"
        b"Usage: VCFX_field_extractor --fields \"FIELD1,FIELD2,...\" [OPTIONS] [input.vcf]\n\n"
        b"Description:\n"
        b"  Extracts specified fields from each VCF record. Fields can be:\n"
        b"    - Standard fields: CHROM, POS, ID, REF, ALT, QUAL, FILTER, INFO\n"
        b"    - Subkeys in INFO (e.g. DP, AF, ANN). These are extracted from the INFO column.\n"
        b"    - Sample subfields: e.g. SampleName:GT or S2:DP, referencing the second sample's DP.\n"
        b"      You can use sample name as it appears in #CHROM line, or 'S' plus 1-based sample index.\n"
        b"If a requested field is not found or invalid, '.' is output.\n\n"
        b"Options:\n"
        b"  --fields, -f   Comma-separated list of fields to extract\n"
        b"  --input, -i    Input VCF file (uses fast memory-mapped I/O)\n"
        b"  --help, -h     Show this help message\n\n"
        b"Performance:\n"
        b"  File input (-i) uses memory-mapped I/O for 10-20x faster processing.\n"
        b"  Features include:\n"
        b"  - SIMD-optimized line scanning (AVX2/SSE2 on x86_64)\n"
        b"  - Zero-copy field extraction\n"
        b"  - 1MB output buffering\n"
        b"  - Direct INFO key lookup without full parsing\n\n"
        b"Example:\n"
        b"  VCFX_field_extractor --fields \"CHROM,POS,ID,REF,ALT,DP,Sample1:GT\" -i input.vcf > out.tsv\n")
VERSION = b"VCFX_field_extractor version 1.1.4\n"
NO_FIELDS = b"No fields specified. Use --fields or -f to specify.\nUse --help for usage.\n"

# include/vcfx_gpu.h
EMPTY, HEADER, ROW = 0, 1, 2
STD, INFO, SAMPLE, NONE = 0, 1, 2, 3
DOT, ONE, NOKEY = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF
CELL_BYTES, TABLE_LDS, TILE_ROWS, STAGE = 8, 16384, 64, 8192
CELL_DOT, CELL_ONE = (0, DOT), (0, ONE)

STANDARD = ("CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO")
LONG = {"help": ("h", False), "fields": ("f", True), "input": ("i", True)}
SHORT_OPTS = {"h": False, "f": True, "i": True}
INT_MAX = (1 << 31) - 1


def getopt_long(argv):
    """GNU getopt_long(argc, argv, "hf:i:", long_opts) with argument permutation:
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
            letter, takes = LONG[hits[0]]
            if takes:
                if eq:
                    opts.append((letter, val, b""))
                elif i < len(argv):
                    opts.append((letter, argv[i], b""))
                    i += 1
                else:
                    opts.append(("?", None, prog + b": option '--" + hits[0].encode() + b"' requires an argument\n"))
            elif eq:
                opts.append(("?", None, prog + b": option '--" + hits[0].encode() + b"' doesn't allow an argument\n"))
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


# ---- the fields ----------------------------------------------------------------------------------

def sample_index(part):
    """the sample part of "sample:subfield": None = a name, an int = 'S' and digits, "bad" = 'S' and
    digits on which the reference's std::stoi throws ('S' alone, a value outside int)"""
    if not part.startswith("S") or any(c not in "0123456789" for c in part[1:]):
        return None
    if len(part) == 1 or int(part[1:]) > INT_MAX:
        return "bad"
    return int(part[1:])


def bad_field(fields):
    """the first field the drop-in rejects before it reads any input, or None"""
    for f in fields:
        if f not in STANDARD and ":" in f and sample_index(f.split(":", 1)[0]) == "bad":
            return f
    return None


def split_spans(line, sep, a, b):
    """the spans of line[a:b] split at every byte sep"""
    out, s = [], a
    while True:
        e = line.find(sep, s, b)
        if e < 0:
            out.append((s, b))
            return out
        out.append((s, e))
        s = e + 1


def info_cell(line, cols, key, stdin):
    """the cell of INFO key `key`, or None when INFO does not hold it"""
    if len(cols) <= 7:
        return None
    a, b = cols[7]
    if stdin:
        if a == b or line[a:a + 1] == b".":
            return None
        pairs = [(s, d) for s, d in split_spans(line, b";", a, b) if d > s]  # a map of the non-empty pairs:
        pairs.reverse()                                                      # the later pair overwrites
    else:
        if a == b or line[a:b] == b".":
            return None
        pairs = split_spans(line, b";", a, b)  # a walk that stops at the first match ...
        if pairs[-1] == (b, b):
            pairs.pop()  # ... and at the field's end: no pair starts there
    for s, d in pairs:
        e = line.find(b"=", s, d)
        if line[s:e if e >= 0 else d] == key:
            return (e + 1, d - e - 1) if e >= 0 else CELL_ONE
    return None


def sample_cell(line, cols, col, sub):
    """the colon token of column col whose index is that of FORMAT's first token equal to sub"""
    if col is None or col < 9 or col >= len(cols):
        return None
    fmt = [line[s:e] for s, e in split_spans(line, b":", *cols[8])]
    if sub not in fmt:
        return None
    toks = split_spans(line, b":", *cols[col])
    k = fmt.index(sub)
    return (toks[k][0], toks[k][1] - toks[k][0]) if k < len(toks) else None


def line_cells(line, fields, names, stdin):
    cols = split_spans(line, b"\t", 0, len(line))
    row = []
    for f in fields:
        fb = f.encode()
        cell = None
        if f in STANDARD:
            k = STANDARD.index(f)
            if k < len(cols):
                cell = (cols[k][0], cols[k][1] - cols[k][0])
        elif ":" not in f:
            cell = info_cell(line, cols, fb, stdin)
        else:
            if stdin:
                cell = info_cell(line, cols, fb, True)  # the map of INFO is asked first
            if cell is None:
                part, sub = f.split(":", 1)
                idx = sample_index(part)
                assert idx != "bad"
                if idx is None:
                    col = names.get(part.encode())
                elif stdin:
                    col = 9 + idx - 1  # (index 0: column 8, below the samples)
                else:
                    col = 9 + idx - 1 if idx > 0 else names.get(b"")  # (index 0 falls to the name "")
                cell = sample_cell(line, cols, col, sub.encode())
        if cell is None or (not stdin and cell[1] == 0):
            cell = CELL_DOT
        row.append(cell)
    return row


def line_spans(buf):
    """(start, end) of every line as the device indexes them: ends at '\\n', a last line without one"""
    out, s = [], 0
    while s < len(buf):
        e = buf.find(b"\n", s)
        if e < 0:
            e = len(buf)
        out.append((s, e))
        s = e + 1
    return out


def scan(buf, fields, stdin):
    """per line (status, start, the row's cells or None)"""
    names, seen, out = {}, False, []
    for a, b in line_spans(buf):
        line = buf[a:b]
        if not stdin and line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            out.append((EMPTY, a, None))
        elif line[:1] == b"#":
            if not seen and line.startswith(b"#CHROM"):
                seen = True
                for i, (s, e) in enumerate(split_spans(line, b"\t", 0, len(line))):
                    if i >= 9:
                        names[line[s:e]] = i  # (of two equal names the later column wins)
            out.append((HEADER, a, None))
        else:
            out.append((ROW, a, line_cells(line, fields, names, stdin)))
    return out


def statuses(buf, fields, stdin):
    return [s for s, _, _ in scan(buf, fields, stdin)]


def cells(buf, fields, stdin):
    """the expected matrix: per row its cells (offset from the line's start, length or DOT / ONE)"""
    return [row for s, _, row in scan(buf, fields, stdin) if s == ROW]


def cell_text(buf, a, cell):
    return b"." if cell[1] == DOT else b"1" if cell[1] == ONE else buf[a + cell[0]:a + cell[0] + cell[1]]


def rows(buf, fields, stdin):
    return b"".join(b"\t".join(cell_text(buf, a, c) for c in row) + b"\n"
                    for s, a, row in scan(buf, fields, stdin) if s == ROW)


def header_row(fields):
    return "\t".join(fields).encode() + b"\n"


def run(argv, stdin=b"", cwd=None):
    """(stdout, stderr, rc) of the drop-in"""
    args = argv[1:]
    if "--help" in args or "-h" in args:  # vcfx::handle_common_flags
        return HELP, b"", 0
    if "--version" in args or "-v" in args:
        return VERSION, b"", 0
    opts, operands = getopt_long(argv)
    path, fields, help_, err = "", [], False, b""
    for k, v, msg in opts:
        err += msg
        if k == "f":
            fields += v.split(",")
        elif k == "i":
            path = v
        else:
            help_ = True
    if not path and operands:
        path = operands[0]
    if help_:
        return HELP, err, 0
    if not fields:
        return b"", err + NO_FIELDS, 1
    bad = bad_field(fields)
    if bad is not None:
        return b"", err + b"Error: invalid sample index in field '" + bad.encode() + b"'\n", 1
    if path and path != "-":
        try:
            with open(os.path.join(cwd, path) if cwd else path, "rb") as f:
                buf = f.read()
        except OSError:
            return b"", err + b"Error: Cannot open file: " + path.encode() + b"\n", 1
        if not buf:
            return b"", err, 0
        return header_row(fields) + rows(buf, fields, False), err, 0
    return header_row(fields) + rows(stdin or b"", fields, True), err, 0


# ---- the table the host builds (vcfxg_fx_col) ----------------------------------------------------

def table(fields, names, stdin):
    """(cols, pool) as fx_build makes them: per field (kind, col, named, key_off, key_len, sub_off,
    sub_len); names = the "#CHROM" line's name -> column"""
    cols, pool = [], b""
    for f in fields:
        fb = f.encode()
        if f in STANDARD:
            cols.append((STD, STANDARD.index(f), 0, 0, NOKEY, 0, 0))
        elif ":" not in f:
            cols.append((INFO, 0, 0, len(pool), len(fb), 0, 0))
            pool += fb
        else:
            part, sub = f.split(":", 1)
            idx = sample_index(part)
            col, named = 0, 0
            if idx is None or (idx == 0 and not stdin):
                named, col = 1, names.get(part.encode() if idx is None else b"", 0)
            elif idx > 0:
                col = 9 + idx - 1
            so = len(pool)
            pool += sub.encode()
            ko, kl = 0, NOKEY
            if stdin:
                ko, kl = len(pool), len(fb)
                pool += fb
            cols.append((SAMPLE, col, named, ko, kl, so, len(sub.encode())))
    return cols, pool


def names_of(buf, stdin):
    """(name -> column of the first "#CHROM" line, the byte after that line's first byte), or ({}, ~0)"""
    for a, b in line_spans(buf):
        line = buf[a:b]
        if not stdin and line.endswith(b"\r"):
            line = line[:-1]
        if line.startswith(b"#CHROM"):
            return {line[s:e]: i for i, (s, e) in enumerate(split_spans(line, b"\t", 0, len(line))) if i >= 9}, a + 1
    return {}, 0xFFFFFFFFFFFFFFFF


# ---- golden cases --------------------------------------------------------------------------------

def load_cases():
    with gzip.open(os.path.join(GOLDEN, "field_extractor_cases.json.gz"), "rb") as f:
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

SAMPLES = (b"NA1", b"NA2", b"dup", b"S3", b"dup")
HDR = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + b"\t".join(SAMPLES) + b"\n"
INFOS = (b"DP=12;AF=0.5;DB", b".", b"", b"DP4=1,2,3,4;ADP=9;DP=3", b"X=DP=3;AF=", b"AF=0.1;AF=0.9;DB;DB=7", b".;DP=2",
         b"DP=1;;AF=2;", b";DP=5", b"=e;DP=6", b"NA1:GT=zz;DP=7", b"DB;H2", b"AF=0.25", b"S1:GT=info;AF=3")
FORMATS = (b"GT", b"GT:DP", b"DP:GT:GQ", b"GT::DP", b"GQ", b"", b"GT:GT", b"DP:")
GEN_FIELDS = "CHROM,POS,ID,REF,ALT,QUAL,FILTER,INFO,DP,AF,DB,DP4,ADP,X,,NA1:GT,NA2:DP,dup:GT,S1:GT,S5:DP,S6:GT,S0:GT,S3:GQ," \
             "absent:GT,NA1:,S2:,H2"


def sample_value(rnd, fmt):
    n = fmt.count(b":") + 1
    toks = [rnd.choice((b"0/1", b"1|1", b".", b"", b"35", b"0|0")) for _ in range(n)]
    return b":".join(toks[:rnd.choice((n, n, n, max(n - 1, 1), 1))])


def record(rnd, chrom=b"1", pos=100, ncols=None):
    fmt = rnd.choice(FORMATS)
    f = [chrom, b"%d" % pos, rnd.choice((b"rs%d" % pos, b".", b"")), rnd.choice((b"A", b"ACGT")), rnd.choice((b"C", b"G,T", b"")),
         rnd.choice((b"50", b".", b"9.5")), rnd.choice((b"PASS", b"q10;s50", b"")), rnd.choice(INFOS), fmt]
    f += [sample_value(rnd, fmt) for _ in SAMPLES]
    return b"\t".join(f[:ncols] if ncols else f)


def gen_vcf(seed, n, crlf=False, final_newline=True, mix=True, header=True):
    """n lines: records with every INFO and FORMAT form, and with mix ragged lines of 1, 2, 8, 9 and 10
    fields, '#' and empty lines, a data line before the header and a second "#CHROM" line"""
    rnd = random.Random(seed)
    lines = []
    if mix:
        lines.append(record(rnd, b"early", 1))
    if header:
        lines += HDR.split(b"\n")[:2]
    pos = 100
    while len(lines) < n:
        pos += rnd.randrange(1, 50)
        r = rnd.random() if mix else 1.0
        if r < 0.05:
            lines.append(b"")
        elif r < 0.10:
            lines.append(rnd.choice((b"##comment\tDP=1", b"#", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tother\tNA1")))
        elif r < 0.25:
            lines.append(record(rnd, rnd.choice((b"1", b"chrX")), pos, rnd.choice((1, 2, 8, 9, 10))))
        elif r < 0.28:
            lines.append(record(rnd, b"2", pos) + b"\t")
        else:
            lines.append(record(rnd, rnd.choice((b"1", b"chrX", b"")), pos))
    nl = b"\r\n" if crlf else b"\n"
    return nl.join(lines[:n]) + (nl if final_newline else b"")


GENERATED = {
    "g300": lambda: gen_vcf(1, 300),
    "g300_crlf": lambda: gen_vcf(2, 300, crlf=True),
    "g300_no_final_newline": lambda: gen_vcf(3, 300, final_newline=False),
    "g300_crlf_no_final_newline": lambda: gen_vcf(4, 300, crlf=True, final_newline=False),
    "routes": lambda: gen_vcf(5, 1500),
}


def generated(name):
    return GENERATED[name]()
