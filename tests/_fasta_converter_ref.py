"""VCFX_fasta_converter in plain Python: the reference tool's behaviour (VCFX_fasta_converter.cpp:
convertVCFtoFastaStreaming :291-424 for a file, convertVCFtoFasta :433-523 for stdin, run :230-258,
main :533-539) restated line by line, the device's view of the same inputs (statuses, column
numbers, the base of every sample, which lines are fixed-stride), fixture generators, and the loader
of the recorded cases (tests/golden/fasta_converter_cases.json.gz, written by
tests/golden/make_fasta_converter_golden.py from the compiled reference).
"""
import base64
import gzip
import json
import os
import random

from tests._duplicate_remover_ref import getopt_long  # the same options: "hi:q", help / input / quiet

TOOL = "VCFX_fasta_converter"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# displayHelp :260-273 (also what --help / -h as a whole argument print: show_help runs `--help`)
HELP = ("VCFX_fasta_converter: Convert VCF to per-sample FASTA.\n\n"
        "Usage: VCFX_fasta_converter [OPTIONS] [FILE]\n\n"
        "Options:\n"
        "  -i, --input FILE    Input VCF file (fastest with mmap)\n"
        "  -q, --quiet         Suppress warnings\n"
        "  -h, --help          Show this help\n\n"
        "Algorithm: Two-pass with contiguous memory buffer.\n"
        "  Pass 1: Count variants (fast scan)\n"
        "  Pass 2: Parse genotypes into pre-allocated buffer\n"
        "  Output: Sequential memory access, perfect cache locality\n\n"
        "Memory: O(variants × samples) - pre-allocated, no reallocations\n"
        "Speed: ~200 MB/s VCF throughput on modern hardware\n\n").encode()
VERSION = b"VCFX_fasta_converter version 1.1.4\n"
NO_CHROM = b"Error: #CHROM header not found before data lines\n"

# include/vcfx_gpu.h
EMPTY, COLUMN, SKIPPED, HEADER, CHROM = 0, 1, 3, 4, 7
LINE = 60            # bases per FASTA line
TILE_SAMPLES = 64    # the transpose tile: samples
TILE_COLUMNS = 240   # ... and columns
TABLE = 16           # alleles whose base the scan tabulates; later ones walk the ALT text

IUPAC = b"AMRWMCSYRSGKWYKT"
N = 78  # 'N'


# ---- one base -------------------------------------------------------------------------------------

def ref_base(ref, stdin):
    """the REF base :365 / :486"""
    if len(ref) != 1:
        return N
    c = ref[0]
    if stdin:
        return c - 32 if 97 <= c <= 122 else c  # toupper, C locale
    return c - 32 if 97 <= c <= 127 else c      # (char)c >= 'a' ? c - 32 : c


def allele_base(k, refb, alt):
    """parseAlleleBase :180-196"""
    if k == 0:
        return refb
    idx, p = 1, 0
    while p < len(alt) and idx < k:
        if alt[p] == 44:
            idx += 1
        p += 1
    if idx != k or p >= len(alt):
        return N
    s = p
    while p < len(alt) and alt[p] != 44:
        p += 1
    if p - s != 1:
        return N
    c = alt[s]
    return c if 65 <= c <= 90 else c - 32 if 97 <= c <= 122 else N


def base_idx(c):
    return {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}.get(c, -1)


def gt_index(fmt):
    """findGTIndex :158-169"""
    idx, p = 0, 0
    while p < len(fmt):
        if fmt[p:p + 2] == b"GT" and (p + 2 >= len(fmt) or fmt[p + 2] == 58):
            return idx
        while p < len(fmt) and fmt[p] != 58:
            p += 1
        if p < len(fmt):
            p += 1
        idx += 1
    return -1


def genotype_base(sample, gi, refb, alt):
    """parseGenotype :198-224 over extractGT :171-178"""
    p, e = 0, len(sample)
    for _ in range(gi):
        if p >= e:
            break
        while p < e and sample[p] != 58:
            p += 1
        if p < e:
            p += 1
    if p >= e or sample[p] == 46:
        return N
    a1 = 0
    while p < e and 48 <= sample[p] <= 57:
        a1 = a1 * 10 + sample[p] - 48
        p += 1
    if p >= e or sample[p] not in b"/|":
        return N
    p += 1
    if p >= e or sample[p] == 46:
        return N
    a2 = 0
    while p < e and 48 <= sample[p] <= 57:
        a2 = a2 * 10 + sample[p] - 48
        p += 1
    b1, b2 = allele_base(a1, refb, alt), allele_base(a2, refb, alt)
    if b1 == N or b2 == N:
        return N
    if b1 == b2:
        return b1
    i1, i2 = base_idx(b1), base_idx(b2)
    return N if i1 < 0 or i2 < 0 else IUPAC[i1 * 4 + i2]


# ---- lines ----------------------------------------------------------------------------------------

def raw_lines(buf):
    """the lines of buf, split at '\\n' only; bytes after the last one are a line"""
    if not buf:
        return []
    lines = buf.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def header_names(line):
    """fields 10 onward of a "#CHROM" line :314-324 / :448-455 (no empty field after a final tab)"""
    f = line.split(b"\t")
    if line.endswith(b"\t"):
        f.pop()
    return f[9:]


def fixed_stride(samples_region, gi):
    """the sample region is N units "a s b \\t" (the last without its tab), s the first unit's '/'
    or '|', a and b digits or '.', and GT is the first FORMAT key: the device's fast path"""
    r = samples_region
    if gi != 0 or len(r) < 3 or (len(r) + 1) % 4:
        return False
    s = r[1]
    if s not in b"/|":
        return False
    for k in range(0, len(r), 4):
        u = r[k:k + 4]
        if u[1] != s or u[0] not in b"0123456789." or u[2] not in b"0123456789." or (len(u) == 4 and u[3] != 9):
            return False
    return True


def column_of(line, stdin, ns):
    """a column line's ns bases (0 for a sample the line does not have) and whether the device
    takes it on the fixed-stride path"""
    end = len(line) - (1 if not stdin and line.endswith(b"\r") else 0)
    body = line[:end]
    tabs = [i for i, c in enumerate(body) if c == 9]
    if len(tabs) < 9:
        return bytes(ns), False
    f = [body[a + 1:b] for a, b in zip([-1] + tabs[:8], tabs[:9])]
    region = body[tabs[8] + 1:]
    refb, alt, gi = ref_base(f[3], stdin), f[4], gt_index(f[8])
    out, p = [], 0
    while p < len(region) and len(out) < ns:
        q = region.find(b"\t", p)
        q = len(region) if q < 0 else q
        out.append(genotype_base(region[p:q], gi, refb, alt) if gi >= 0 else N)
        p = q + 1
    return bytes(out + [0] * (ns - len(out))), fixed_stride(region, gi)


def line_status(line, stdin, ns):
    """the device's status of a line when the samples so far are ns"""
    if not line:
        return EMPTY if stdin else COLUMN
    if line[:1] == b"#":
        return CHROM if line[:6] == b"#CHROM" else HEADER
    if stdin:
        fields = line.count(b"\t") + 1 - (1 if line.endswith(b"\t") else 0)
        return COLUMN if fields >= 9 + ns else SKIPPED
    return COLUMN


def wrap(seq):
    return b"".join(seq[i:i + LINE] + b"\n" for i in range(0, len(seq), LINE))


def convert_file(buf):
    """convertVCFtoFastaStreaming :291-424: stdout"""
    lines = raw_lines(buf)
    names = []
    for ln in lines:
        if ln[:6] == b"#CHROM":
            names += header_names(ln)
    cols = [column_of(ln, False, len(names))[0] for ln in lines if ln[:1] != b"#"]
    if not names or not cols:
        return b""
    return b"".join(b">" + nm + b"\n" + wrap(bytes(c[s] for c in cols)) for s, nm in enumerate(names))


def convert_stdin(buf):
    """convertVCFtoFasta :433-523: (stdout, stderr)"""
    names, seqs, parsed = [], [], False
    for ln in raw_lines(buf):
        if not ln:
            continue
        if ln[:1] == b"#":
            if ln[:6] == b"#CHROM":
                names += header_names(ln)
                seqs += [bytearray() for _ in range(len(names) - len(seqs))]
                parsed = True
            continue
        if not parsed:
            return b"", NO_CHROM
        if line_status(ln, True, len(names)) != COLUMN:
            continue
        col = column_of(ln, True, len(names))[0]
        for s, b in enumerate(col):
            seqs[s].append(b)
    if not seqs or not seqs[0]:
        return b"", b""
    return b"".join(b">" + nm + b"\n" + wrap(bytes(q)) for nm, q in zip(names, seqs)), b""


def device_view(buf, stdin):
    """the data part as the raw ABI sees it: (its first byte, the names before it, whether a "#CHROM"
    line stands before it, per line (status, the samples the status was taken with)); the first is
    None when the tool never calls the device.
    The data part starts at the first line that is a column candidate: in file mode the first line
    that does not start with '#', on stdin the first non-empty one."""
    lines = raw_lines(buf)
    names, k, seen = [], 0, False
    while k < len(lines):
        ln = lines[k]
        if ln[:1] == b"#" or (stdin and not ln):
            if ln[:6] == b"#CHROM":
                names += header_names(ln)
                seen = True
            k += 1
            continue
        break
    start = sum(len(ln) + 1 for ln in lines[:k])
    if k >= len(lines):
        return None, names, seen, []
    per, cur = [], list(names)
    for ln in lines[k:]:
        per.append((line_status(ln, stdin, len(cur)), len(cur)))
        if ln[:6] == b"#CHROM":
            cur += header_names(ln)
    return start, names, seen, per


def sequences(buf, stdin):
    """what the device is asked for: (the names, each sample's sequence, the column lines that are
    not fixed-stride), or None where the tool prints nothing.  Sample s's row of the device text is
    wrap(sequence s)."""
    lines = raw_lines(buf)
    names, cols, general = [], [], 0  # cols: (the samples the column was parsed against, its bases)
    if not stdin:
        for ln in lines:
            if ln[:6] == b"#CHROM":
                names += header_names(ln)
    seen = not stdin
    for ln in lines:
        if stdin and ln[:6] == b"#CHROM":
            names += header_names(ln)
            seen = True
        if line_status(ln, stdin, len(names)) != COLUMN:
            continue
        if not seen:
            return None
        bases, fixed = column_of(ln, stdin, len(names))
        cols.append(bases)
        general += not fixed
    seqs = [bytes(c[s] for c in cols if s < len(c)) for s in range(len(names))]
    if not names or not cols or not seqs[0]:
        return None
    return names, seqs, general


def run(argv, stdin=b"", cwd=None):
    """main :533-539 and run :230-258: (stdout, stderr, rc)"""
    args = argv[1:]
    if "--help" in args or "-h" in args:  # vcfx::handle_common_flags: show_help runs `--help`
        return HELP, b"", 0
    if "--version" in args or "-v" in args:
        return VERSION, b"", 0
    opts, operands = getopt_long(argv)
    path, err = None, b""
    for k, v, msg in opts:
        err += msg
        if k == "i":
            path = v
        elif k != "q":
            return HELP, err, 0  # the first -h or unknown option ends the argument loop
    if not path and operands:  # (an empty -i value counts as none)
        path = operands[0]
    if path:
        full = os.path.join(cwd, path) if cwd else path
        try:
            with open(full, "rb") as f:
                buf = f.read()
        except OSError:
            return b"", err + b"Error: Cannot open " + path.encode() + b"\n", 1
        return convert_file(buf), err, 0
    out, e = convert_stdin(stdin or b"")
    return out, err + e, 0


# ---- golden cases --------------------------------------------------------------------------------

def load_cases():
    with gzip.open(os.path.join(GOLDEN, "fasta_converter_cases.json.gz"), "rb") as f:
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
ALTS = (b"A", b"C", b"G", b"T", b"a", b"t", b"AC", b"<DEL>", b"*", b".", b"")


def chrom_line(names):
    return b"\t".join([COLS] + list(names))


def gen_gt(rnd, n_alt, odd):
    r = rnd.random()
    if r < odd:
        return rnd.choice((b".", b"", b"1", b"/", b"1/", b"/1", b"0/.", b"./0", b"00/1", b"1a/1", b"0/1/2", b"0/x", b"10|2",
                           b"0|", b"./."))
    hi = n_alt + 1
    return b"%d" % rnd.randrange(hi + 1) + rnd.choice((b"/", b"|")) + b"%d" % rnd.randrange(hi + 1)


def gen_record(rnd, i, ns, n_alt, fmt=b"GT", odd=0.0, clean=False):
    """a data line of ns samples; clean: single-digit diploid GTs of one separator (fixed-stride when
    fmt is GT)"""
    keys = fmt.split(b":")
    alt = b",".join(rnd.choice(ALTS[:4] if clean else ALTS) for _ in range(n_alt))
    sep = rnd.choice((b"/", b"|"))
    samples = []
    for _ in range(ns):
        sub = []
        for k in keys:
            if k == b"GT":
                if clean:
                    sub.append(bytes([rnd.choice(b"012.")]) + sep + bytes([rnd.choice(b"012.")]))
                else:
                    sub.append(gen_gt(rnd, n_alt, odd))
            elif k == b"AD":
                sub.append(b"%d,%d" % (rnd.randrange(50), rnd.randrange(50)))
            else:
                sub.append(b"%d" % rnd.randrange(99))
        if not clean and rnd.random() < odd:
            sub = sub[:rnd.randrange(len(sub) + 1)]
        samples.append(b":".join(sub))
    ref = rnd.choice((b"A", b"C", b"G", b"T") if clean else (b"A", b"C", b"G", b"T", b"a", b"g", b"AT", b".", b"N"))
    return b"\t".join([b"chr%d" % (1 + i % 3), b"%d" % (100 + i), b".", ref, alt, b".", b"PASS", b".", fmt] + samples)


def gen_vcf(seed, records, ns, fmt=b"GT", alts=(1, 2, 3), odd=0.0, clean=False, mix=False, crlf=False,
            final_newline=True, second_header=None, extra=0):
    """a header and `records` data lines of ns samples.  mix: empty, '#', short, long and ragged lines
    in between; second_header = (after record k, names): another "#CHROM" line there, the records
    after it carrying ns + len(names) samples; extra: more samples than names on every line"""
    rnd = random.Random(seed)
    eol = b"\r\n" if crlf else b"\n"
    out = [b"##fileformat=VCFv4.2", chrom_line([b"S%d" % i for i in range(ns)])]
    width = ns
    for i in range(records):
        if second_header and i == second_header[0]:
            out.append(chrom_line(second_header[1]))
            width += len(second_header[1])
        if mix:
            r = rnd.random()
            if r < 0.06:
                out.append(b"")
            elif r < 0.12:
                out.append(b"#comment %d" % i)
            elif r < 0.18:
                out.append(rnd.choice((b"1\t5\t.\tA\tC", b"1\t5\t.\tA\tC\t.\t.\t.\tGT", b"1\t5\t.\tA\tC\t.\t.\t.\tGT\t",
                                       b"x", b"1\t5\t.\tA\tC\t.\t.\t.\tGT\t0/1")))
        w = width + extra
        if mix and rnd.random() < 0.1:
            w = rnd.randrange(0, width + 3)
        ln = gen_record(rnd, i, w, alts[i % len(alts)], fmt, odd, clean) if w else \
            b"\t".join(gen_record(rnd, i, 1, 1, fmt).split(b"\t")[:9])
        if mix and rnd.random() < 0.05:
            ln += b"\t"
        out.append(ln)
    return eol.join(out) + (eol if final_newline else b"")


def bench_input(fmt, total_bytes=1 << 30, ns=2504, pool=32, seed=2026):
    """the measurement input (tools/fa_time.py): well-formed bi-allelic records of ns samples in the
    given FORMAT up to total_bytes; `pool` distinct records repeat under rising POS values"""
    rnd = random.Random(seed)
    recs = [gen_record(rnd, i, ns, 1, fmt, clean=True).split(b"\t", 2)[2] for i in range(pool)]
    out = [b"##fileformat=VCFv4.2\n" + chrom_line([b"S%d" % i for i in range(ns)]) + b"\n"]
    size, i = len(out[0]), 0
    while size < total_bytes:
        ln = b"chr1\t%d\t%s\n" % (1000 + i, recs[i % pool])
        out.append(ln)
        size += len(ln)
        i += 1
    return b"".join(out)
