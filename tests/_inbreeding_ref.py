"""numpy restatement of VCFX_inbreeding_calculator (test infrastructure: the checker of the
device results where the compiled reference is not available; never imported by vcfx_amd/).

A record loop, vectorised over the samples (the parse of an input is kept for the next flag set), with the reference's operation order: per record
and sample `freq = altEx / (2.0 * validEx)`, `eHet = (2.0 * freq) * (1.0 - freq)`, added to the
sample's sumExp in record order (IEEE doubles, nothing contracted).  Both input modes are
restated as they are, including the file mode's reused genotype-code buffer: a sample past a
short record's columns keeps the code the last parsed record left there.

tests/test_inbreeding_ref.py holds it to the compiled reference's recorded bytes."""
import functools
import os

import numpy as np

HEADER = b"Sample\tInbreedingCoefficient\n"

HELP = (b"VCFX_inbreeding_calculator: Compute individual inbreeding coefficients (F)\n"
        b"based on biallelic sites in a VCF.\n\n"
        b"Usage:\n"
        b"  VCFX_inbreeding_calculator [options] [input.vcf]\n"
        b"  VCFX_inbreeding_calculator [options] < input.vcf\n\n"
        b"Options:\n"
        b"  -i, --input FILE          Input VCF file (uses memory-mapping for best performance)\n"
        b"  -q, --quiet               Suppress informational messages\n"
        b"  -h, --help                Show this help.\n"
        b"  --freq-mode <mode>        'excludeSample' (default) or 'global'\n"
        b"  --skip-boundary           Skip boundary freq sites. By default, they are used.\n"
        b"  --count-boundary-as-used  If also skipping boundary, still increment usedCount.\n\n"
        b"Description:\n"
        b"  Reads a VCF in a single pass, ignoring multi-allelic lines (ALT with commas).\n"
        b"  For each biallelic variant, we parse each sample's genotype code:\n"
        b"       0/0 => 0,   0/1 => 1,   1/1 => 2, else => -1 (ignored)\n\n"
        b"  Then, depending on --freq-mode:\n"
        b"    * excludeSample => Each sample excludes its own genotype when computing p.\n"
        b"    * global        => Compute a single global p from all samples' genotypes.\n\n"
        b"  The --skip-boundary option, if set, ignores boundary freq p=0 or p=1.\n"
        b"    BUT if you also specify --count-boundary-as-used, those boundary sites\n"
        b"    increment usedCount (forcing F=1) without contributing to sumExp.\n\n"
        b"  If sumExp=0 for a sample but usedCount>0, we output F=1.\n"
        b"  If usedCount=0, we output NA.\n\n"
        b"Performance:\n"
        b"  Uses memory-mapped I/O and SIMD for ~20x speedup over stdin mode.\n"
        b"  When a file is provided directly, uses mmap for faster processing.\n\n"
        b"Example:\n"
        b"  VCFX_inbreeding_calculator -i input.vcf > inbreeding.txt\n"
        b"  VCFX_inbreeding_calculator < input.vcf > inbreeding.txt\n")

_DIGITS = b"0123456789"


def gt_code(field):
    """parseGenotypeCode: the GT prefix up to ':', leading ' ' / CR skipped, digits, '/' or '|',
    digits; the rest is ignored.  0/0 -> 0, 0/1 -> 1, 1/1 -> 2, anything else -> -1."""
    c = field.find(b":")
    if c >= 0:
        field = field[:c]
    n, i = len(field), 0
    while i < n and field[i] in b" \r":
        i += 1
    if i >= n or field[i] not in _DIGITS:
        return -1
    a1 = 0
    while i < n and field[i] in _DIGITS:
        a1 = a1 * 10 + field[i] - 48
        i += 1
    if i >= n or field[i] not in b"/|":
        return -1
    i += 1
    if i >= n or field[i] not in _DIGITS:
        return -1
    a2 = 0
    while i < n and field[i] in _DIGITS:
        a2 = a2 * 10 + field[i] - 48
        i += 1
    if a1 > 1 or a2 > 1:
        return -1
    return a1 + a2


class _Codes:
    """gt_code with a cache per distinct field text"""

    def __init__(self):
        self.cache = {}

    def row(self, cols):
        cache = self.cache
        out = []
        for f in cols:
            v = cache.get(f)
            if v is None:
                v = cache[f] = gt_code(f)
            out.append(v)
        return np.array(out, np.int64)


def _lines(buf):
    parts = buf.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    return parts


def _strip_cr(line):
    return line[:-1] if line.endswith(b"\r") else line


class Acc:
    def __init__(self, names):
        n = len(names)
        self.names = names
        self.sum_exp = np.zeros(n, np.float64)
        self.obs_het = np.zeros(n, np.uint64)
        self.used = np.zeros(n, np.uint64)
        self.variants = 0
        self.parsed = 0

    def record(self, code, alt_sum, n_good, glob, skipb, countb):
        """the per-sample loop of one used record (code: every sample's code, stale ones included)"""
        self.variants += 1
        ok = code >= 0
        if glob:
            freq = np.full(len(code), np.float64(alt_sum) / (2.0 * n_good))
        else:
            freq = (alt_sum - code).astype(np.float64) / (2.0 * (n_good - 1))
        bnd = (freq <= 0.0) | (freq >= 1.0)
        if skipb:
            if countb:
                self.used[ok & bnd] += np.uint64(1)
            ok = ok & ~bnd
        e_het = (2.0 * freq) * (1.0 - freq)
        self.used[ok] += np.uint64(1)
        self.sum_exp[ok] = self.sum_exp[ok] + e_het[ok]
        self.obs_het[ok & (code == 1)] += np.uint64(1)


@functools.lru_cache(maxsize=8)
def _parse_file(buf):
    """calculateInbreedingMmap's header and parse: (names, [(codes of every sample, altSum,
    nGood)] per parsed record), None when there is no '#CHROM' line or no sample"""
    lines = _lines(buf)
    names, found, k = [], False, 0
    while k < len(lines):
        line = _strip_cr(lines[k])
        if line and line[:1] != b"#":
            break
        if line[:6] == b"#CHROM":
            found = True
            f = line.split(b"\t")
            if f[-1] == b"":
                f.pop()  # a field that would start at the line end is not there
            names += [x[:-1] if x.endswith(b"\r") else x for x in f[9:]]
        k += 1
    if not found or not names:
        return None
    ns = len(names)
    codes = np.zeros(ns, np.int64)  # the reused buffer
    cache = _Codes()
    recs = []
    for raw in lines[k:]:
        line = _strip_cr(raw)
        if not line or line[:1] == b"#":
            continue
        f = line.split(b"\t")
        if len(f) < 5 or f[4] == b"" or b"," in f[4]:
            continue
        cols = f[9:]
        if cols and cols[-1] == b"":
            cols.pop()  # the column after a trailing tab starts at the line end
        if not cols:
            continue
        row = cache.row(cols[:ns])
        codes[:len(row)] = row
        recs.append((codes.copy(), int(row[row >= 0].sum()), int((row >= 0).sum())))
    return names, recs


@functools.lru_cache(maxsize=8)
def _parse_stdin(buf):
    """calculateInbreedingStdin's header and parse; "nochrom" / "nosamples" on its errors"""
    lines = _lines(buf)
    k, names = 0, None
    while k < len(lines):
        line = lines[k]
        k += 1
        if not line:
            continue
        line = _strip_cr(line)
        if line[:1] == b"#" and b"#CHROM" in line:
            names = line.split(b"\t")[9:]
            break
    if names is None:
        return "nochrom"
    if not names:
        return "nosamples"
    ns = len(names)
    cache = _Codes()
    recs = []
    for raw in lines[k:]:
        if not raw:
            continue
        line = _strip_cr(raw)
        if not line or line[:1] == b"#":
            continue
        f = line.split(b"\t")
        if len(f) < 10 or b"," in f[4]:
            continue
        cols = f[9:9 + ns]
        code = np.full(ns, -1, np.int64)
        code[:len(cols)] = cache.row(cols)
        recs.append((code, int(code[code >= 0].sum()), int((code >= 0).sum())))
    return names, recs


def _accumulate(parsed, glob, skipb, countb):
    if parsed is None or isinstance(parsed, str):
        return parsed
    names, recs = parsed
    acc = Acc(names)
    acc.parsed = len(recs)
    for code, alt_sum, n_good in recs:
        if n_good >= 2:
            acc.record(code, alt_sum, n_good, glob, skipb, countb)
    return acc


def accumulate_file(buf, glob=False, skipb=False, countb=False):
    """calculateInbreedingMmap's accumulators: None when there is no '#CHROM' line or sample"""
    return _accumulate(_parse_file(bytes(buf)), glob, skipb, countb)


def accumulate_stdin(buf, glob=False, skipb=False, countb=False):
    """calculateInbreedingStdin's accumulators: the string "nochrom" / "nosamples" on its errors"""
    return _accumulate(_parse_stdin(bytes(buf)), glob, skipb, countb)


def append_double(val):
    """OutputBuffer::appendDouble: six decimals, truncated"""
    out = b""
    val = float(val)
    if val < 0:
        out += b"-"
        val = -val
    ip = int(val)
    frac = val - float(ip)
    out += str(ip).encode() + b"."
    for _ in range(6):
        frac *= 10.0
        d = int(frac)
        out += bytes([48 + d])
        frac -= d
    return out


def rows(acc):
    out = []
    for s, name in enumerate(acc.names):
        if acc.used[s] == 0:
            out.append(name + b"\tNA\n")
        elif acc.sum_exp[s] <= 0.0:
            out.append(name + b"\t1.000000\n")
        else:
            f = 1.0 - (float(acc.obs_het[s]) / float(acc.sum_exp[s]))
            out.append(name + b"\t" + append_double(f) + b"\n")
    return b"".join(out)


def _report(acc, quiet):
    if acc.variants == 0:
        err = b"" if quiet else b"No biallelic variants found.\n"
        return HEADER + b"".join(n + b"\tNA\n" for n in acc.names), err
    return HEADER + rows(acc), b""


def parse_args(argv):
    """parseArgs for well-formed command lines (options may follow the positional file)"""
    a = {"input": None, "glob": False, "skipb": False, "countb": False, "quiet": False, "help": False, "err": b""}
    pos = []
    i = 1
    while i < len(argv):
        x = argv[i]
        i += 1
        val = None
        if x.startswith("--") and "=" in x:
            x, val = x.split("=", 1)
        if x in ("-i", "--input", "--freq-mode") and val is None:
            val = argv[i]
            i += 1
        if x.startswith("-i") and len(x) > 2 and not x.startswith("--"):
            x, val = "-i", x[2:]
        if x in ("-i", "--input"):
            a["input"] = val
        elif x in ("-q", "--quiet"):
            a["quiet"] = True
        elif x in ("-h", "--help"):
            a["help"] = True
        elif x == "--freq-mode":
            if val == "global":
                a["glob"] = True
            elif val == "excludeSample":
                a["glob"] = False
            else:
                a["err"] += ("Warning: unrecognized freq-mode='%s'. Using 'excludeSample' by default.\n" % val).encode()
        elif x == "--skip-boundary":
            a["skipb"] = True
        elif x == "--count-boundary-as-used":
            a["countb"] = True
        elif x.startswith("-") and x != "-":
            raise ValueError("option not restated: %s" % x)
        else:
            pos.append(x)
    if a["input"] is None and pos:
        a["input"] = pos[0]
    return a


def run(argv, stdin=b"", cwd=None):
    """(stdout, stderr, exit code) of `argv` with stdin, as the reference executable gives them"""
    if "--help" in argv[1:] or "-h" in argv[1:]:
        return HELP, b"", 0
    if "--version" in argv[1:] or "-v" in argv[1:]:
        return b"VCFX_inbreeding_calculator version 1.1.4\n", b"", 0
    a = parse_args(argv)
    err = a["err"]
    if a["help"]:
        return HELP, err, 0
    if a["input"] is not None:
        path = os.path.join(cwd, a["input"]) if cwd else a["input"]
        try:
            with open(path, "rb") as f:
                buf = f.read()
        except OSError:
            return b"", err + b"Error: Cannot open file: " + a["input"].encode() + b"\n", 1
        if not a["quiet"]:
            err += ("Processing %s (%d bytes)...\n" % (a["input"], len(buf))).encode()
        if not buf:
            return HEADER, err + b"Error: Empty file.\n", 0
        acc = accumulate_file(buf, a["glob"], a["skipb"], a["countb"])
        if acc is None:
            return HEADER, err + b"Error: No #CHROM line or no samples found.\n", 0
    else:
        acc = accumulate_stdin(stdin, a["glob"], a["skipb"], a["countb"])
        if acc == "nochrom":
            return HEADER, err + b"Error: No #CHROM line found.\n", 0
        if acc == "nosamples":
            return HEADER, err + b"Error: No sample columns found.\n", 0
    out, e2 = _report(acc, a["quiet"])
    return out, err + e2, 0


ODD_GT = [b"./.", b".", b"0/.", b"./1", b"2/1", b"0/1/1", b" 0/1", b"1|0:5", b"0/1x", b"10/0", b"01/1", b"", b"1",
          b"0|", b"|1", b"\r1/1", b"1/1:.:3", b"0/0 "]
PLAIN_GT = [b"0/0", b"0/1", b"1/0", b"1/1", b"0|0", b"0|1", b"1|0", b"1|1"]


def ragged_vcf(seed, n_records, n_samples, crlf=False, odd=0.1, short=0.15, junk=0.1):
    """a seeded VCF with the shapes the two modes treat differently: short records (the first
    one among them), lines ending in a tab, multi-allelic and empty ALT, '#' and empty lines
    between the records, odd genotype fields, records with fewer than two calls"""
    rng = np.random.default_rng(seed)
    eol = b"\r\n" if crlf else b"\n"
    out = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" +
           b"\t".join(b"S%d" % i for i in range(n_samples))]
    for r in range(n_records):
        u = rng.random()
        if u < junk / 4:
            out.append(b"#comment %d" % r)
            continue
        if u < junk / 2:
            out.append(b"")
            continue
        alt = b"T"
        if u < junk * 0.75:
            alt = b"T,G"
        elif u < junk:
            alt = b""
        p = rng.choice([0.0, 0.02, 0.2, 0.5, 0.9, 1.0], p=[0.05, 0.15, 0.3, 0.3, 0.15, 0.05])
        fmt = b"GT:DP" if rng.random() < 0.3 else b"GT"
        n = n_samples
        v = rng.random()
        if r == 0 or v < short:
            n = int(rng.integers(0, n_samples + 1))
        elif v < short + 0.03:
            n = n_samples + int(rng.integers(1, 4))  # more columns than the header
        a = (rng.random((n, 2)) < p).sum(axis=1)
        sep = rng.random(n) < 0.5
        cols = []
        oddm = rng.random(n) < (odd if rng.random() < 0.8 else 0.95)
        for s in range(n):
            if oddm[s]:
                g = ODD_GT[int(rng.integers(0, len(ODD_GT)))]
            else:
                g = PLAIN_GT[(4 if sep[s] else 0) + (0, 1 + int(rng.integers(0, 2)), 3)[a[s]]]
            if fmt == b"GT:DP" and b":" not in g:
                g += b":%d" % int(rng.integers(0, 60))
            cols.append(g)
        line = b"\t".join([b"1", b"%d" % (1000 + r), b".", b"A", alt, b".", b"PASS", b".", fmt] + cols)
        if rng.random() < 0.05:
            line += b"\t"
        out.append(line)
    return eol.join(out) + (eol if rng.random() < 0.8 else b"")
