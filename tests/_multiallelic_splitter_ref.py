"""VCFX_multiallelic_splitter restated in plain Python (VCFX_multiallelic_splitter.cpp): the CLI, the
file mode (processFileMmap :422-646) and the stdin mode (splitMultiAllelicVariants :652-758), plus
the input generators of the tests.  tests/test_multiallelic_splitter_ref.py holds it to the compiled
reference's recorded bytes (tests/golden/multiallelic_splitter_cases.json.gz); tests/test_gpu_ms.py
checks the device against it on generated inputs.

The two modes differ in how they count fields (file: a line that ends in a tab has no trailing
empty field; stdin: it has), in empty lines (file drops them, stdin writes them) and in what
happens without a "#CHROM" line (file copies the rest as it is, stdin goes on splitting).  Outside
the domain: a GT allele index of more than 9 digits, an ALT of 46,340 or more alleles."""
import base64
import gzip
import json
import os
import random

from tests._duplicate_remover_ref import getopt_long  # the same options: "hi:q", help / input / quiet

TOOL = "VCFX_multiallelic_splitter"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# displayHelp :206-224
HELP = (b"VCFX_multiallelic_splitter: Split multi-allelic variants into multiple lines.\n\n"
        b"Usage:\n"
        b"  VCFX_multiallelic_splitter [options] [input.vcf]\n"
        b"  VCFX_multiallelic_splitter [options] < input.vcf > output.vcf\n\n"
        b"Options:\n"
        b"  -i, --input FILE    Input VCF file (uses mmap for best performance)\n"
        b"  -q, --quiet         Suppress warning messages\n"
        b"  -h, --help          Display this help message and exit\n\n"
        b"Description:\n"
        b"  Splits multi-allelic variants into multiple lines, rewriting GT/AD/PL\n"
        b"  and other Number=A/R/G fields for each split variant.\n\n"
        b"Performance:\n"
        b"  When using -i/--input, the tool uses memory-mapped I/O for\n"
        b"  ~15x faster processing of large files.\n\n"
        b"Example:\n"
        b"  VCFX_multiallelic_splitter -i input.vcf > split.vcf\n"
        b"  VCFX_multiallelic_splitter < input.vcf > split.vcf\n")
# printHelp :764-774
COMMON_HELP = (b"VCFX_multiallelic_splitter:\n"
               b"  Splits multi-allelic variants into multiple lines, rewriting GT/AD/PL.\n"
               b"Usage:\n"
               b"  VCFX_multiallelic_splitter [options] < input.vcf > output.vcf\n"
               b"  VCFX_multiallelic_splitter -i input.vcf > output.vcf\n"
               b"Options:\n"
               b"  -i, --input FILE    Input VCF file (uses mmap for best performance)\n"
               b"  -q, --quiet         Suppress warnings\n"
               b"  --help, -h          Show this help\n")
VERSION = b"VCFX_multiallelic_splitter version 1.1.4\n"

# vcfx_gpu.h VCFXG_MS_*
EMPTY, COPY, SPLIT, HEADER = 0, 1, 2, 4
INFO, FORMAT = 0, 1
NUM_OTHER, NUM_A, NUM_R, NUM_G = 0, 1, 2, 3
KEYS_LDS = 32      # FORMAT keys whose classes the device keeps in LDS
TABLE_LDS = 16384  # table bytes the device keeps in LDS
NUMBERS = {b"A": NUM_A, b"R": NUM_R, b"G": NUM_G}


# ---- the header table ----------------------------------------------------------------------------

def parse_header_line(line):
    """parseHeaderLine :226-245: (id, section, number bytes) or None"""
    if line.startswith(b"##INFO="):
        section = INFO
    elif line.startswith(b"##FORMAT="):
        section = FORMAT
    else:
        return None
    vals = []
    for tag in (b"ID=", b"Number="):
        i = line.find(tag)
        if i < 0:
            return None
        sub = line[i + len(tag):]
        ends = [k for k in (sub.find(b","), sub.find(b">")) if k >= 0]
        if not ends:
            return None
        vals.append(sub[:min(ends)])
    return vals[0], section, vals[1]


def table_entries(decls):
    """the declarations as vcfxg_ms_entry tuples (id, section, number class), in order"""
    return [(i, s, NUMBERS.get(n, NUM_OTHER)) for i, s, n in decls]


def table_bytes(decls):
    """the bytes of the device's table: 12 per ID that recodes + its bytes rounded up to 4"""
    last = {}
    for i, s, n in decls:
        last[i] = n
    return sum(12 + (len(i) + 3) // 4 * 4 for i, n in last.items() if n in NUMBERS)


# ---- the recode ----------------------------------------------------------------------------------

def rec_a(vals, k):
    return vals[k] if k < len(vals) else b"."


def rec_r(vals, k):
    if len(vals) == 1 and vals[0] == b".":
        return b"."
    return vals[0] + b"," + (vals[k] if k < len(vals) else b".")


def rec_g(vals, j, n):
    if len(vals) != (n + 1) * (n + 2) // 2:
        return b"."
    return b",".join((vals[0], vals[j], vals[(2 * n + 1 - j) * j // 2]))


def recode_value(num, val, j, n):
    vals = val.split(b",")
    if num == b"A":
        return rec_a(vals, j - 1)
    if num == b"R":
        return rec_r(vals, j)
    if num == b"G":
        return rec_g(vals, j, n)
    return val


def recode_info(info, j, n, meta):
    """recodeInfoField :247-316 for allele j (1-based) of n"""
    if info in (b".", b""):
        return b"."
    out = []
    for item in info.split(b";"):
        if not item:
            continue
        key, eq, val = item.partition(b"=")
        m = meta.get(key)
        if not eq or m is None or m[0] != INFO:
            out.append(item)
        else:
            out.append(key + b"=" + recode_value(m[1], val, j, n))
    return b";".join(out) or b"."


def conv_allele(x, j):
    if x in (b"0", b"."):
        return x
    if not all(48 <= c <= 57 for c in x):
        return b"."
    return b"1" if int(x or b"0") == j else b"."


def recode_sample(sample, keys, j, n, meta):
    """recodeSample :318-420"""
    subs = sample.split(b":")
    subs += [b"."] * (len(keys) - len(subs))
    out = []
    for key, sub in zip(keys, subs):
        if key == b"GT":
            g = sub.replace(b"|", b"/")
            d = g.find(b"/")
            if d < 0:
                out.append(b".")
                continue
            a, b = conv_allele(g[:d], j), conv_allele(g[d + 1:], j)
            out.append(b"." if a == b == b"." else a + b"/" + b)
        else:
            m = meta.get(key)
            out.append(sub if m is None or m[0] != FORMAT else recode_value(m[1], sub, j, n))
    return b":".join(out)


def fields_of(line, stdin):
    """the line's fields as the mode counts them: splitTabsView :22-38 / vcfx::split_tabs"""
    f = line.split(b"\t")
    if not stdin and f[-1] == b"":
        f.pop()
    return f


def split_line(line, stdin, meta):
    """the output lines of a non-empty data line (itself when it is not split)"""
    f = fields_of(line, stdin)
    if len(f) < 9 or b"," not in f[4]:
        return [line]
    alts, keys = f[4].split(b","), f[8].split(b":")
    n = len(alts)
    return [b"\t".join(f[:4] + [alts[a]] + f[5:7] + [recode_info(f[7], a + 1, n, meta), f[8]] +
                       [recode_sample(s, keys, a + 1, n, meta) for s in f[9:]]) for a in range(n)]


def raw_lines(buf):
    """the lines of buf, split at '\\n' only; bytes after the last one are a line"""
    if not buf:
        return []
    lines = buf.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def header_part(lines):
    """(the lines read before the data part, the header table, whether a "#CHROM" line ended them)"""
    meta, decls, k = {}, [], 0
    while k < len(lines):
        ln = lines[k]
        if ln and ln[:1] != b"#":
            return k, meta, decls, False
        k += 1
        if ln[:2] == b"##":
            d = parse_header_line(ln)
            if d:
                decls.append(d)
                meta[d[0]] = (d[1], d[2])
        if ln[:6] == b"#CHROM":
            return k, meta, decls, True
    return k, meta, decls, False


def split(buf, stdin):
    """the tool's stdout over the input bytes in one mode"""
    lines = raw_lines(buf)
    k, meta, _, chrom = header_part(lines)
    out = [ln for ln in lines[:k] if ln or stdin]
    if not stdin and not chrom:
        return b"".join(ln + b"\n" for ln in out + lines[k:])
    for ln in lines[k:]:
        if not ln:
            if stdin:
                out.append(ln)
        elif ln[:1] == b"#":
            out.append(ln)
        else:
            out += split_line(ln, stdin, meta)
    return b"".join(ln + b"\n" for ln in out)


def device_view(buf, stdin):
    """what the raw ABI reports for the data part: (its first byte, the table's declarations, per
    line (status, nAlts, the rows' bytes)); None for the first when the tool never calls the device"""
    lines = raw_lines(buf)
    k, meta, decls, chrom = header_part(lines)
    start = sum(len(ln) + 1 for ln in lines[:k])
    if start >= len(buf) or (not stdin and not chrom):
        return None, decls, []
    per = []
    for ln in lines[k:]:
        if not ln:
            per.append((EMPTY, 0, b""))
        elif ln[:1] == b"#":
            per.append((HEADER, 0, b""))
        else:
            rows = split_line(ln, stdin, meta)
            f = fields_of(ln, stdin)
            if len(f) >= 9 and b"," in f[4]:
                per.append((SPLIT, len(rows), b"".join(r + b"\n" for r in rows)))
            else:
                per.append((COPY, 0, b""))
    return start, decls, per


def run(argv, stdin=b"", cwd=None):
    """main :788-795 and run :153-204: (stdout, stderr, rc)"""
    args = argv[1:]
    if "--help" in args or "-h" in args:  # vcfx::handle_common_flags
        return COMMON_HELP, b"", 0
    if "--version" in args or "-v" in args:
        return VERSION, b"", 0
    opts, operands = getopt_long(argv)
    path, help_, err = None, False, b""
    for k, v, msg in opts:
        err += msg
        if k == "i":
            path = v
        elif k != "q":
            help_ = True
    if path is None and operands:
        path = operands[0]
    if help_:
        return HELP, err, 0
    if path is not None:
        full = os.path.join(cwd, path) if cwd else path
        try:
            with open(full, "rb") as f:
                buf = f.read()
        except OSError:
            return b"", err + b"Error: Cannot open file: " + path.encode() + b"\n", 1
        return split(buf, False), err, 0
    return split(stdin or b"", True), err, 0


# ---- golden cases --------------------------------------------------------------------------------

def load_cases():
    with gzip.open(os.path.join(GOLDEN, "multiallelic_splitter_cases.json.gz"), "rb") as f:
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

BASES = (b"A", b"C", b"G", b"T", b"AC", b"GTT", b"<DEL>", b"*")


def header(ns, extra=(), eol=b"\n"):
    """AF = A and AC = R as INFO, AD = R, PL = G and XA = A as FORMAT, DP a plain number"""
    h = [b"##fileformat=VCFv4.2",
         b"##INFO=<ID=AF,Number=A,Type=Float,Description=\"f\">",
         b"##INFO=<ID=AC,Number=R,Type=Integer,Description=\"c\">",
         b"##INFO=<ID=DP,Number=1,Type=Integer,Description=\"d\">",
         b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"g\">",
         b"##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"a\">",
         b"##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"d\">",
         b"##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"p\">",
         b"##FORMAT=<ID=XA,Number=A,Type=Integer,Description=\"x\">"] + list(extra)
    h.append(b"\t".join([b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT"] +
                        [b"S%d" % i for i in range(ns)]))
    return eol.join(h) + eol


def gen_sample(rnd, keys, n, odd):
    """one sample for the FORMAT keys at n ALT alleles; odd: the chance of a malformed sub-field"""
    out = []
    for key in keys:
        r = rnd.random()
        if key == b"GT":
            if r < odd:
                out.append(rnd.choice((b".", b"", b"1", b"/", b"1/", b"/1", b"00/1", b"1a/2", b"1/2/3", b"./.")))
            else:
                a, b = (rnd.choice([b"."] + [b"%d" % k for k in range(n + 2)]) for _ in range(2))
                out.append(a + rnd.choice((b"/", b"|")) + b)
            continue
        want = {b"AD": n + 1, b"PL": (n + 1) * (n + 2) // 2, b"XA": n, b"AF": n, b"AC": n + 1}.get(key, 1)
        if r < odd:
            want = rnd.choice((0, 1, max(want - 1, 0), want + 1))
        if r > 1 - odd / 2:
            out.append(b".")
        else:
            out.append(b",".join(rnd.choice((b".", b"")) if rnd.random() < odd / 4 else b"%d" % rnd.randrange(200)
                                 for _ in range(want)))
    k = len(out)
    if rnd.random() < odd:
        k = rnd.randrange(0, len(out) + 3)
    return b":".join((out + [b"extra", b"9"])[:k])


def gen_record(rnd, i, ns, n, keys=(b"GT", b"AD", b"DP", b"PL"), odd=0.1):
    alts = b",".join(rnd.choice(BASES) for _ in range(n))
    info = b";".join(x for x in (b"AF=" + b",".join(b"0.%d" % rnd.randrange(99) for _ in range(n)),
                                 b"AC=" + b",".join(b"%d" % rnd.randrange(99) for _ in range(n + 1)),
                                 b"DB" if rnd.random() < 0.5 else b"", b"DP=%d" % rnd.randrange(999),
                                 b"ZZ=1,2" if rnd.random() < 0.3 else b"") if x or rnd.random() < 0.2)
    return b"\t".join([b"chr%d" % (1 + i % 3), b"%d" % (100 + i), b"rs%d" % i, rnd.choice(BASES[:4]), alts,
                       b"%d" % rnd.randrange(99), b"PASS", info, b":".join(keys)] +
                      [gen_sample(rnd, keys, n, odd) for _ in range(ns)])


def gen_vcf(seed, records, ns, alts=(1, 2, 3), keys=(b"GT", b"AD", b"DP", b"PL"), odd=0.1, mix=False, crlf=False,
            final_newline=True, extra_header=()):
    """`records` data lines of ns samples whose ALT counts cycle through `alts`; mix: empty lines,
    '#' lines, short lines and trailing tabs in between"""
    rnd = random.Random(seed)
    eol = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(records):
        if mix:
            r = rnd.random()
            if r < 0.06:
                out.append(b"")
            elif r < 0.12:
                out.append(b"#comment %d" % i)
            elif r < 0.18:
                out.append(rnd.choice((b"1\t5\t.\tA\tC,G", b"1\t5\t.\tA\tC,G\t.\t.\t.", b"1\t5\t.\tA\tC,G\t.\t.\t.\t",
                                       b"1\t5\t.\tA\tC,G\t.\t.\tAF=1,2\tGT\t")))
        ln = gen_record(rnd, i, ns, alts[i % len(alts)], keys, odd)
        if mix and rnd.random() < 0.05:
            ln += b"\t"
        out.append(ln)
    return header(ns, extra_header, eol) + eol.join(out) + (eol if final_newline and out else b"")


def bench_input(share, total_bytes=1 << 30, ns=2504, pool=32, seed=2026):
    """the measurement input (tools/ms_time.py): records of ns samples, FORMAT GT:AD:DP:PL, of
    which `share` per cent are tri-allelic (two ALT alleles) and the rest bi-allelic, well-formed
    throughout, up to total_bytes.  `pool` distinct records of each kind come from gen_record;
    they repeat under rising POS values until the size is reached."""
    rnd = random.Random(seed)
    pools = {n: [gen_record(rnd, i, ns, n, odd=0.0).split(b"\t", 2)[2] for i in range(pool)] for n in (1, 2)}
    out, size, i = [header(ns)], 0, 0
    size = len(out[0])
    while size < total_bytes:
        n = 2 if (i * share) // 100 != ((i + 1) * share) // 100 else 1
        ln = b"chr1\t%d\t%s\n" % (1000 + i, pools[n][i % pool])
        out.append(ln)
        size += len(ln)
        i += 1
    return b"".join(out)
