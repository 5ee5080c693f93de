"""Plain-Python restatement of VCFX_cross_sample_concordance (both modes, the file mode's row
order included), the loader of its golden cases and the generators of test inputs.

Held byte for byte to the compiled reference's recorded runs by tests/test_concordance_ref.py;
the checker of generated inputs in tests/test_gpu_cc.py.  Line numbers refer to
src/VCFX_cross_sample_concordance/VCFX_cross_sample_concordance.cpp of the reference."""
import base64
import gzip
import json
import os
import random

TOOL = "VCFX_cross_sample_concordance"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HELP = (b"VCFX_cross_sample_concordance: Check variant concordance across multiple samples.\n\n"
        b"Usage:\n"
        b"  VCFX_cross_sample_concordance [options] < input.vcf > concordance_results.txt\n"
        b"  VCFX_cross_sample_concordance -i input.vcf > concordance_results.txt\n\n"
        b"Options:\n"
        b"  -i, --input FILE        Input VCF file (uses mmap for best performance)\n"
        b"  -s, --samples LIST      Comma-separated list of samples to check\n"
        b"  -t, --threads N         Number of processing threads (default: auto)\n"
        b"  -q, --quiet             Suppress summary statistics to stderr\n"
        b"  -h, --help              Display this help message and exit\n\n"
        b"Description:\n"
        b"  Reads a multi-sample VCF, normalizes each sample's genotype\n"
        b"  (including multi-allelic variants), and determines if all samples that\n"
        b"  have a parseable genotype are in complete agreement.\n\n"
        b"Performance:\n"
        b"  Uses multi-threaded parallel processing with memory-mapped I/O\n"
        b"  and early-termination optimization for extreme performance.\n\n"
        b"Example:\n"
        b"  VCFX_cross_sample_concordance -i input.vcf -t 8 > results.tsv\n")
VERSION = b"VCFX_cross_sample_concordance version 1.1.4\n"
HEADER = b"CHROM\tPOS\tID\tREF\tALT\tNum_Samples\tUnique_Normalized_Genotypes\tConcordance_Status\n"
E_NOCHROM = b"Error: VCF header with #CHROM not found.\n"
W_NONE = b"Warning: none of the requested samples were found in the VCF header.\n"
NONE, CONCORDANT, DISCORDANT, NO_GENOTYPES = 0, 1, 2, 3
WORD = {CONCORDANT: b"CONCORDANT", DISCORDANT: b"DISCORDANT", NO_GENOTYPES: b"NO_GENOTYPES"}

LONG = {"help": False, "input": True, "samples": True, "threads": True, "quiet": False}
SHORT_OPTS = {"h": False, "i": True, "s": True, "t": True, "q": False}


def getopt_long(argv):
    """GNU getopt_long(argc, argv, "hi:s:t:q", longOpts) with argument permutation, one option at
    a time as the caller's loop sees them: ([(letter or '?', value, its stderr message)], operands)"""
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


def atoi(s):
    """std::atoi for the values the tests pass (optional sign, leading digits, else 0)"""
    s = s.strip()
    k = 1 if s[:1] in ("+", "-") else 0
    j = k
    while j < len(s) and s[j].isdigit():
        j += 1
    return int(s[:j]) if j > k else 0


# ---- the per-record rules ------------------------------------------------------------------------

def num_alt(alt):
    """countAltAlleles :170-178"""
    if not alt or alt[:1] == b".":
        return 0
    return alt.count(b",") + 1


def gt_key(field, max_allele):
    """parseGenotypeToId :130-167: (lo, hi), or None for an invalid key"""
    gt = field.split(b":", 1)[0]
    if not gt or gt[:1] == b".":
        return None
    p, a = 0, [0, 0]
    while p < len(gt) and 48 <= gt[p] <= 57:
        a[0] = a[0] * 10 + gt[p] - 48
        p += 1
    if p >= len(gt) or gt[p] not in b"/|":
        return None
    p += 1
    if p >= len(gt) or gt[p:p + 1] == b".":
        return None
    while p < len(gt) and 48 <= gt[p] <= 57:
        a[1] = a[1] * 10 + gt[p] - 48
        p += 1
    assert max(a) < 2 ** 31, "an allele that overflows int is undefined in the reference"
    if a[0] > max_allele or a[1] > max_allele or a[0] > 127 or a[1] > 127:
        return None
    return (min(a), max(a))


def reduce_keys(keys):
    """(Num_Samples, Unique_Normalized_Genotypes, status) of a record's valid keys"""
    if not keys:
        return 0, 0, NO_GENOTYPES
    u = len(set(keys))
    return len(keys), u, CONCORDANT if u == 1 else DISCORDANT


def row(f, n, u, st):
    return b"\t".join(f[:5]) + b"\t%d\t%d\t" % (n, u) + WORD[st] + b"\n"


def file_fields(line):
    """the tab loop of processVariantLine :242-248: a trailing tab opens no field"""
    f = line.split(b"\t")
    if f and f[-1] == b"" and line:
        f.pop()
    return f if line else []


def file_line(line, indices):
    """processVariantLine :229-319 on a collected data line: (fields, N, U, status); status NONE
    when the line gives no row"""
    f = file_fields(line)
    if len(f) < 5 or not f[0]:
        return f, 0, 0, NONE
    na = num_alt(f[4])
    keys = []
    for idx in indices:
        if idx >= len(f):
            continue
        k = gt_key(f[idx], na)
        if k is not None:
            keys.append(k)
    return (f,) + reduce_keys(keys)


def stdin_line(line, n_names, indices):
    """calculateConcordance :649-716 on a line after the header (indices count from field 9)"""
    if not line or line[:1] == b"#":
        return None, 0, 0, NONE
    f = line.split(b"\t")
    if len(f) < 8 or len(f) < 9 + n_names:
        return f, 0, 0, NONE
    na = num_alt(f[4])
    keys = [k for k in (gt_key(f[9 + i], na) for i in indices) if k is not None]
    return (f,) + reduce_keys(keys)


def output_order(n, threads):
    """the data-line numbers in output order (:498-499, :521, :579-581): T = threads clamped to
    [1, n] workers, worker t takes lines t, t + T, ..., the workers' rows follow one another"""
    t = max(1, min(threads, n))
    return [i for w in range(t) for i in range(w, n, t)]


def rank_of(i, n, threads):
    """the closed form of output_order's inverse that the device uses"""
    t = max(1, min(threads, n))
    q, r = divmod(n, t)
    w = i % t
    return w * q + min(w, r) + i // t


def summary(conc, disc, nogt):
    return (b"Total Variants with >=1 parseable genotype: %d\n"
            b"   Concordant (all same genotype): %d\n"
            b"   Discordant (>=2 distinct genotypes): %d\n"
            b"Variants with no parseable genotypes (skipped): %d\n" % (conc + disc, conc, disc, nogt))


def split_lines(buf):
    lines = buf.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def file_scan(buf, want):
    """phase 1 of calculateConcordanceMmapParallel :445-475: (found, selected columns over every
    '#CHROM' line, the collected data lines)"""
    indices, data, found = [], [], False
    for ln in split_lines(buf):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if not ln:
            continue
        if ln[:1] == b"#":
            if ln[:6] == b"#CHROM":
                for col, name in enumerate(file_fields(ln)):
                    if col >= 9 and (not want or name in want):
                        indices.append(col)
                found = True
        elif found:
            data.append(ln)
    return found, indices, data


def file_mode(buf, want, threads, quiet):
    """calculateConcordanceMmapParallel :416-593 on an opened file: (stdout, stderr, rc)"""
    if not buf:
        return b"", b"", 0
    found, indices, data = file_scan(buf, want)
    if not found:
        return b"", E_NOCHROM, 1
    err = W_NONE if (not indices and want) else b""
    if not data:
        return HEADER, err + (b"" if quiet else b"Total Variants with >=1 parseable genotype: 0\n"), 0
    rows, cnt = [], {CONCORDANT: 0, DISCORDANT: 0, NO_GENOTYPES: 0}
    for i in output_order(len(data), threads):
        f, n, u, st = file_line(data[i], indices)
        if st == NONE:
            continue
        cnt[st] += 1
        rows.append(row(f, n, u, st))
    if not quiet:
        err += summary(cnt[CONCORDANT], cnt[DISCORDANT], cnt[NO_GENOTYPES])
        err += b"Threads used: %d\n" % max(1, min(threads, len(data)))
    return HEADER + b"".join(rows), err, 0


def stdin_scan(buf, want):
    """the header loop of calculateConcordance :622-642: (found, names, indices, the lines after)"""
    lines = split_lines(buf)
    for k, ln in enumerate(lines):
        if ln[:6] == b"#CHROM":
            names = ln.split(b"\t")[9:]
            indices = [i for i, nm in enumerate(names) if not want or nm in want]
            return True, names, indices, lines[k + 1:]
    return False, [], [], []


def stdin_mode(buf, want, quiet):
    """calculateConcordance :598-724: (stdout, stderr, rc)"""
    found, names, indices, lines = stdin_scan(buf, want)
    if not found:
        return HEADER, E_NOCHROM, 0
    rows, cnt = [], {CONCORDANT: 0, DISCORDANT: 0, NO_GENOTYPES: 0}
    for ln in lines:
        f, n, u, st = stdin_line(ln, len(names), indices)
        if st == NONE:
            continue
        cnt[st] += 1
        rows.append(row(f, n, u, st))
    err = b"" if quiet else summary(cnt[CONCORDANT], cnt[DISCORDANT], cnt[NO_GENOTYPES])
    return HEADER + b"".join(rows), err, 0


def run(argv, stdin=b"", cwd=None, default_threads=None):
    """main :731-750: (stdout, stderr, rc).  default_threads stands for hardware_concurrency()"""
    args = argv[1:]
    if "--help" in args or "-h" in args:  # vcfx::handle_common_flags
        return HELP, b"", 0
    if "--version" in args or "-v" in args:
        return VERSION, b"", 0
    opts, operands = getopt_long(argv)
    path, want, threads, quiet, err = "", set(), 0, False, b""
    for k, v, msg in opts:
        err += msg
        if k == "h":
            return HELP, err, 0
        if k == "?":
            return b"", err, 0
        if k == "i":
            path = v
        elif k == "s":
            want.update(x.encode() for x in v.split(","))
        elif k == "t":
            threads = atoi(v)
        elif k == "q":
            quiet = True
    if not path and operands:
        path = operands[0]
    if threads <= 0:
        threads = default_threads or os.cpu_count() or 4
    if path:
        full = os.path.join(cwd, path) if cwd else path
        try:
            with open(full, "rb") as f:
                buf = f.read()
        except OSError:
            return b"", err + b"Error: Cannot open file " + path.encode() + b"\n", 1
        o, e, rc = file_mode(buf, want, threads, quiet)
        return o, err + e, rc
    o, e, rc = stdin_mode(stdin or b"", want, quiet)
    return o, err + e, rc


# ---- per-line expectations of the raw ABI ----------------------------------------------------------

def region_file(buf, want=None):
    """file mode from the byte after the first '#CHROM' line: (data_start, multiplicities per
    sample column, per line of the region (N, U, status), the collected data lines' count)"""
    found, indices, data = file_scan(buf, want or set())
    assert found
    k = buf.index(b"#CHROM") if buf[:6] == b"#CHROM" else buf.index(b"\n#CHROM") + 1
    nl = buf.find(b"\n", k)
    ds = len(buf) if nl < 0 else nl + 1
    mult = [0] * (max(indices) - 8 if indices else 0)
    for c in indices:
        mult[c - 9] += 1
    per = []
    for ln in split_lines(buf[ds:]):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if not ln or ln[:1] == b"#":
            per.append((0, 0, NONE))
        else:
            per.append(file_line(ln, indices)[1:])
    return ds, mult, per, len(data)


# ---- golden cases --------------------------------------------------------------------------------

def load_cases():
    with gzip.open(os.path.join(GOLDEN, "concordance_cases.json.gz"), "rb") as f:
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

HDR9 = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"


def names(ns):
    return [b"S%d" % i for i in range(ns)]


def header(ns, eol=b"\n"):
    return b"##fileformat=VCFv4.2" + eol + b"\t".join([HDR9] + names(ns)) + eol


def record(pos, fields, alt=b"T", fmt=b"GT", chrom=b"1"):
    return b"\t".join([chrom, b"%d" % pos, b"rs%d" % pos, b"A", alt, b".", b"PASS", b".", fmt] + list(fields))


def alt_of(n):
    return b"," .join([b"T", b"G", b"C", b"TT", b"TG", b"TC", b"GG", b"GC", b"CC", b"TTT"][:n]) if n else b"."


def clean_vcf(seed, nrec, ns, missing=0.0, max_alt=1, phased=None):
    """fixed-stride records: one-digit alleles, one separator per record, FORMAT GT; a record is
    all the same genotype, mostly the same, or mixed"""
    rnd = random.Random(seed)
    out = [header(ns)]
    for r in range(nrec):
        na = rnd.randrange(1, max_alt + 1)
        sep = (b"|" if phased else b"/") if phased is not None else rnd.choice([b"/", b"|"])
        kind = rnd.random()
        base = b"%d%s%d" % (rnd.randrange(na + 1), sep, rnd.randrange(na + 1))
        f = []
        for _ in range(ns):
            if rnd.random() < missing:
                f.append(b"." + sep + b".")
            elif kind < 0.3 or (kind < 0.6 and rnd.random() < 0.97):
                f.append(base)
            else:
                f.append(b"%d%s%d" % (rnd.randrange(min(na + 2, 10)), sep, rnd.randrange(min(na + 2, 10))))
        out.append(record(100 + r, f, alt=alt_of(na)) + b"\n")
    return b"".join(out)


def ragged_vcf(seed, nrec, ns, crlf=False, final_newline=True):
    """records of odd sample fields (the traps of parseGenotypeToId), mixed separators, some cut
    short (down to 3 fields), some over-wide, some ending in a tab, some with an empty CHROM or
    ALT, with '#', '#CHROM'-less comment and empty lines among them"""
    rnd = random.Random(seed)
    eol = b"\r\n" if crlf else b"\n"
    gts = [b"0/0", b"0|1", b"1/0", b"1/1", b"./.", b".", b"0/.", b"./1", b"/0", b"0/x", b"0/", b"1", b"0/1/1",
           b"0/1:12,3:15", b"1|1:0,9", b"", b"10/2", b"2/10", b"127/0", b"128/0", b"3|3", b"01/1", b":0/1", b"0/2"]
    out = [header(ns, eol)]
    for r in range(nrec):
        x = rnd.random()
        if x < 0.04:
            out.append(eol)
            continue
        if x < 0.08:
            out.append(b"#comment %d\tx" % r + eol)
            continue
        pick = gts if rnd.random() < 0.7 else gts[:4]
        f = [rnd.choice(pick) for _ in range(ns)]
        na = rnd.choice([0, 1, 1, 2, 3, 9, 130])
        alt = b",".join([b"T"] * na) if na else rnd.choice([b".", b""])
        line = record(1000 + r, f, alt=alt, chrom=b"" if rnd.random() < 0.03 else b"chr%d" % rnd.randrange(1, 4))
        y = rnd.random()
        if y < 0.25:
            parts = line.split(b"\t")
            line = b"\t".join(parts[:rnd.randrange(3, len(parts) + 1)])
        elif y < 0.30:
            line += b"\t"
        elif y < 0.35:
            line += b"\t0/1\t1/1"
        out.append(line + eol)
    buf = b"".join(out)
    if not final_newline:
        buf = buf[:-len(eol)]
    return buf
