"""Plain-Python restatement of VCFX_sample_extractor (the reference's
src/VCFX_sample_extractor/VCFX_sample_extractor.cpp): the CLI, file mode (extractSamplesMmap) and
stdin mode (extractSamples), byte for byte.  tests/test_sample_extractor_ref.py holds it to the
compiled reference's recorded runs; the GPU tests check generated inputs against it.

run(argv, stdin=b"", cwd=None) -> (stdout, stderr, rc).  lines(buf, cols, stdin_mode, seen) gives
the per-line statuses and output pieces of the data part alone (the raw ABI's contract)."""
import os
import random

TOOL = "VCFX_sample_extractor"
VERSION = b"VCFX_sample_extractor version 1.1.4\n"
HELP = (
    b"VCFX_sample_extractor: Subset a VCF to a chosen set of samples.\n\n"
    b"Usage:\n"
    b"  VCFX_sample_extractor --samples \"Sample1,Sample2\" [options] [input.vcf]\n"
    b"  VCFX_sample_extractor --samples \"Sample1,Sample2\" < input.vcf > output.vcf\n\n"
    b"Options:\n"
    b"  -h, --help              Print this help.\n"
    b"  -s, --samples <LIST>    Comma or space separated list of sample names.\n"
    b"  -i, --input FILE        Input VCF file (uses fast memory-mapped I/O)\n\n"
    b"Performance:\n"
    b"  File input (-i) uses memory-mapped I/O for 10-20x faster processing.\n"
    b"  Features include:\n"
    b"  - SIMD-optimized line scanning (AVX2/SSE2 on x86_64)\n"
    b"  - Zero-copy field extraction\n"
    b"  - 1MB output buffering\n\n"
    b"Description:\n"
    b"  Reads #CHROM line to identify sample columns. Keeps only user-specified samples.\n"
    b"  Rewrites #CHROM line with that subset. For each variant data line, we keep only the\n"
    b"  chosen sample columns. If a sample isn't found in the header, logs a warning.\n\n"
    b"Example:\n"
    b"  VCFX_sample_extractor --samples \"IndivA,IndivB\" -i input.vcf > subset.vcf\n")
W_PRE = b"Warning: data line encountered before #CHROM => skipping.\n"
W_SHORT = b"Warning: line has <8 columns => skipping.\n"
W_NOSAMP = b"Warning: data line with no sample columns => skipping.\n"
E_NOSAMPLES = b"Error: must specify at least one sample with --samples.\n"

# per-line statuses of the device pass (include/vcfx_gpu.h VCFXG_SX_*)
EMPTY, ROW, SHORT, HEADER, NO_SAMPLES, PRE, CHROM = 0, 1, 3, 4, 5, 6, 7
WARNINGS = {SHORT: W_SHORT, NO_SAMPLES: W_NOSAMP, PRE: W_PRE}

LONG = {"help": False, "samples": True, "input": True}
SHORT_OPTS = {"h": False, "s": True, "i": True}
KEY = {"help": "h", "samples": "s", "input": "i"}


def getopt_long(argv):
    """GNU getopt_long(argc, argv, "hs:i:", {help, samples, input}) with argument permutation:
    ([(option letter or '?', value)], operands, its stderr messages)"""
    prog = argv[0].encode()
    opts, operands, err = [], [], b""
    i = 1
    while i < len(argv):
        a = argv[i]
        i += 1
        if a == "--":
            operands += argv[i:]
            break
        if a.startswith("--"):
            name, eq, val = a[2:].partition("=")
            hits = [k for k in LONG if k.startswith(name)]
            if name in LONG:
                hits = [name]
            if len(hits) != 1:
                if hits:
                    err += prog + b": option '" + a.encode() + b"' is ambiguous; possibilities:" + \
                        b"".join(b" '--" + h.encode() + b"'" for h in hits) + b"\n"
                else:
                    err += prog + b": unrecognized option '" + a.encode() + b"'\n"
                opts.append(("?", None))
                continue
            k = hits[0]
            if LONG[k]:
                if eq:
                    opts.append((KEY[k], val))
                elif i < len(argv):
                    opts.append((KEY[k], argv[i]))
                    i += 1
                else:
                    err += prog + b": option '--" + k.encode() + b"' requires an argument\n"
                    opts.append(("?", None))
            elif eq:
                err += prog + b": option '--" + k.encode() + b"' doesn't allow an argument\n"
                opts.append(("?", None))
            else:
                opts.append((KEY[k], None))
        elif a.startswith("-") and len(a) > 1:
            j = 1
            while j < len(a):
                ch = a[j]
                j += 1
                if ch not in SHORT_OPTS:
                    err += prog + b": invalid option -- '" + ch.encode() + b"'\n"
                    opts.append(("?", None))
                elif SHORT_OPTS[ch]:
                    if j < len(a):
                        opts.append((ch, a[j:]))
                    elif i < len(argv):
                        opts.append((ch, argv[i]))
                        i += 1
                    else:
                        err += prog + b": option requires an argument -- '" + ch.encode() + b"'\n"
                        opts.append(("?", None))
                    break
                else:
                    opts.append((ch, None))
        else:
            operands.append(a)
    return opts, operands, err


def split_samples(arg):
    """-s: whitespace-separated tokens, each split at commas, empty pieces dropped"""
    out = []
    for tok in arg.encode().split():  # (bytes.split(): the C locale's isspace set)
        out += [p for p in tok.split(b",") if p]
    return out


def select(fields, samples):
    """(kept column numbers, stderr) of a '#CHROM' line's fields"""
    want = set(samples)
    cols = [i for i in range(9, len(fields)) if fields[i] in want]
    kept = {fields[i] for i in cols}
    err = b"".join(b"Warning: sample '" + s + b"' not found in header.\n" for s in samples if s not in kept)
    return cols, err


def data_line(line, cols, stdin_mode):
    """(status, output bytes) of a data line (not empty, not '#') under the kept columns"""
    f = line.split(b"\t")
    if len(f) < 8:
        return SHORT, b""
    if len(f) == 8 and stdin_mode:
        return NO_SAMPLES, b""
    out = b"\t".join(f[:9])
    for c in cols:
        out += b"\t" + (f[c] if c < len(f) else b".")
    return ROW, out + b"\n"


def split_lines(buf):
    """the lines of buf as getline / the mmap loop see them (a last line without '\\n' counts)"""
    if not buf:
        return []
    ls = buf.split(b"\n")
    if ls[-1] == b"":
        ls.pop()
    return ls


def lines(buf, cols, stdin_mode, seen=True):
    """per line of buf: (status, output bytes) as vcfxg_sample_extract defines them"""
    out = []
    for line in split_lines(buf):
        if not stdin_mode and line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            out.append((EMPTY, b"\n"))
        elif line[:1] == b"#":
            if stdin_mode and line[:6] == b"#CHROM":
                out.append((CHROM, b""))
            else:
                out.append((HEADER, line + b"\n"))
        elif not seen:
            out.append((PRE, b""))
        else:
            out.append(data_line(line, cols, stdin_mode))
    return out


def extract_file(buf, samples):
    """extractSamplesMmap: (stdout, stderr)"""
    out, err, cols, found = [], [], [], False
    for line in split_lines(buf):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            out.append(b"\n")
        elif line[:1] == b"#":
            if not found and line[:6] == b"#CHROM":
                found = True
                f = line.split(b"\t")
                cols, e = select(f, samples)
                err.append(e)
                out.append(b"\t".join(f[:9] + [f[c] for c in cols]) + b"\n")
            else:
                out.append(line + b"\n")
        elif not found:
            err.append(W_PRE)
        else:
            st, o = data_line(line, cols, False)
            out.append(o)
            err.append(WARNINGS.get(st, b""))
    return b"".join(out), b"".join(err)


def extract_stdin(buf, samples):
    """extractSamples: (stdout, stderr)"""
    out, err, cols, found = [], [], [], False
    for line in split_lines(buf):
        if not line:
            out.append(b"\n")
        elif line[:1] == b"#":
            if line[:6] == b"#CHROM":
                found = True
                f = line.split(b"\t")
                cols = []
                if len(f) < 9:
                    out.append(line + b"\n")
                    continue
                cols, e = select(f, samples)
                err.append(e)
                out.append(b"\t".join(f[:9] + [f[c] for c in cols]) + b"\n")
            else:
                out.append(line + b"\n")
        elif not found:
            err.append(W_PRE)
        else:
            st, o = data_line(line, cols, True)
            out.append(o)
            err.append(WARNINGS.get(st, b""))
    return b"".join(out), b"".join(err)


def run(argv, stdin=b"", cwd=None):
    """main + VCFXSampleExtractor::run: (stdout, stderr, rc)"""
    args = argv[1:]
    if "--help" in args or "-h" in args:  # vcfx::handle_common_flags
        return HELP, b"", 0
    if "--version" in args or "-v" in args:
        return VERSION, b"", 0
    if len(argv) == 1:
        return HELP, b"", 0
    opts, operands, err = getopt_long(argv)
    help_, samples, path = False, [], ""
    for k, v in opts:
        if k == "h" or k == "?":
            help_ = True
        elif k == "s":
            samples += split_samples(v)
        elif k == "i":
            path = v
    if not path and operands:
        path = operands[0]
    if help_:
        return HELP, err, 0
    if not samples:
        return b"", err + E_NOSAMPLES, 1
    if path and path != "-":
        full = os.path.join(cwd, path) if cwd else path
        try:
            with open(full, "rb") as f:
                buf = f.read()
        except OSError:
            return b"", err + b"Error: Cannot open file: " + path.encode() + b"\n", 1
        o, e = extract_file(buf, samples)
        return o, err + e, 0
    o, e = extract_stdin(stdin or b"", samples)
    return o, err + e, 0


# ---- generated inputs ---------------------------------------------------------------------

HDR9 = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"


def names(ns):
    return [b"S%d" % i for i in range(ns)]


def header(ns, eol=b"\n"):
    return b"##fileformat=VCFv4.2" + eol + b"\t".join([HDR9] + names(ns)) + eol


def record(pos, fields, info=b".", fmt=b"GT"):
    return b"\t".join([b"1", b"%d" % pos, b".", b"A", b"T", b".", b"PASS", info, fmt] + list(fields))


def ragged_vcf(seed, nrec, ns, crlf=False, final_newline=True):
    """records of varied sample fields, some cut short (down to 6 fields), some ending in a tab,
    some with empty fields, with '#' and empty lines among them"""
    rnd = random.Random(seed)
    eol = b"\r\n" if crlf else b"\n"
    gts = [b"0/0", b"0|1", b"1/1", b"./.", b".", b"0/1:12,3:15", b"1|1:0,9:9", b"", b"10/2", b"0"]
    out = [header(ns, eol)]
    for r in range(nrec):
        x = rnd.random()
        if x < 0.04:
            out.append(eol)
            continue
        if x < 0.08:
            out.append(b"#comment %d\tx" % r + eol)
            continue
        f = [rnd.choice(gts) for _ in range(ns)]
        line = record(1000 + r, f, info=b"DP=%d" % rnd.randrange(10 ** rnd.randrange(1, 9)))
        y = rnd.random()
        if y < 0.25:  # fewer columns than the header: down to 6 fields
            parts = line.split(b"\t")
            line = b"\t".join(parts[:rnd.randrange(6, len(parts) + 1)])
        elif y < 0.30:
            line += b"\t"
        elif y < 0.35:
            line += b"\tEXTRA\tMORE"
        out.append(line + eol)
    buf = b"".join(out)
    if not final_newline:
        buf = buf[:-len(eol)]
    return buf


def sized_vcf(ns, lengths, field=b"0|1", seed=0):
    """one record per requested line length (bytes without the '\\n'): the INFO field is padded
    so that the line is exactly that long"""
    out = [header(ns)]
    for k, want in enumerate(lengths):
        base = record(7 + k, [field] * ns, info=b"")
        pad = want - len(base)
        assert pad >= 1, (want, len(base))
        out.append(record(7 + k, [field] * ns, info=b"X" * pad) + b"\n")
    return b"".join(out)
