"""VCFX_duplicate_remover restated in plain Python (VCFX_duplicate_remover.cpp): the CLI, the file
mode (processFileMmap :226-382) and the stdin mode (removeDuplicates :182-214), plus the input
generators of the tests.  tests/test_duplicate_remover_ref.py holds it to the compiled reference's
recorded bytes (tests/golden/duplicate_remover_cases.json.gz); tests/test_gpu_dd.py checks the
device against it on generated inputs.

The two modes differ in POS (stdin: std::stoi of the field, any exception 0; file: strtol from the
field's first byte, cast to int, so its white-space skip crosses tabs and newlines and its value
saturates at LONG_MAX / LONG_MIN before the cast) and in empty ALT tokens (stdin keeps, file
drops).  Outside the domain: NUL bytes, and a file-mode POS scan that reaches the input's end."""
import base64
import gzip
import json
import os
import random

TOOL = "VCFX_duplicate_remover"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HELP = (b"VCFX_duplicate_remover: Remove duplicate variants from VCF files.\n\n"
        b"Usage:\n"
        b"  VCFX_duplicate_remover [options] [input.vcf]\n"
        b"  VCFX_duplicate_remover [options] < input.vcf > output.vcf\n\n"
        b"Options:\n"
        b"  -i, --input FILE    Input VCF file (uses mmap for best performance)\n"
        b"  -q, --quiet         Suppress warning messages\n"
        b"  -h, --help          Display this help message and exit\n\n"
        b"Description:\n"
        b"  Removes duplicate variants from a VCF file based on the combination of\n"
        b"  chromosome, position, REF, and ALT alleles. For multi-allelic records, the\n"
        b"  ALT field is normalized by sorting the comma-separated alleles so that the\n"
        b"  ordering does not affect duplicate detection.\n\n"
        b"Performance:\n"
        b"  When using -i/--input, the tool uses memory-mapped I/O for\n"
        b"  ~10-20x faster processing of large files.\n\n"
        b"Example:\n"
        b"  VCFX_duplicate_remover -i input.vcf > unique_variants.vcf\n"
        b"  VCFX_duplicate_remover < input.vcf > unique_variants.vcf\n")
VERSION = b"VCFX_duplicate_remover version 1.1.4\n"
WARN = b"Warning: Skipping invalid VCF line.\n"

# vcfx_gpu.h VCFXG_DD_*
EMPTY, KEPT, DUP, SHORT, HEADER = 0, 1, 2, 3, 4
WINDOW = 64  # VCFXG_DD_WINDOW: the bytes of a line the device's lane path looks at

LONG = {"help": False, "input": True, "quiet": False}
SHORT_OPTS = {"h": False, "i": True, "q": False}
SPACE = b" \t\n\v\f\r"


def getopt_long(argv):
    """GNU getopt_long(argc, argv, "hi:q", long_options) with argument permutation:
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

def strtol(buf, p):
    """strtol(buf + p, &end, 10) on a buffer that goes on past the field: (any digits, value)"""
    n = len(buf)
    while p < n and buf[p] in SPACE:
        p += 1
    neg = False
    if p < n and buf[p] in b"+-":
        neg = buf[p:p + 1] == b"-"
        p += 1
    q = p
    while q < n and 48 <= buf[q] <= 57:
        q += 1
    if q == p:
        return False, 0
    v = int(buf[p:q])
    v = -v if neg else v
    return True, max(-(1 << 63), min((1 << 63) - 1, v))


def pos_file(buf, p):
    """static_cast<int>(strtol(posStart, ...)) :146"""
    v = strtol(buf, p)[1] & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def pos_stdin(field):
    """std::stoi(pos), 0 on any exception :115-119"""
    ok, v = strtol(field, 0)
    return v if ok and -(1 << 31) <= v < (1 << 31) else 0


def tab_offsets(buf, ls, le, want=5):
    t, p = [], ls
    while len(t) < want:
        k = buf.find(b"\t", p, le)
        if k < 0:
            break
        t.append(k)
        p = k + 1
    return t


def line_key(buf, ls, le, stdin):
    """the VariantKey of the data line buf[ls:le], None with fewer than four tabs"""
    t = tab_offsets(buf, ls, le)
    if len(t) < 4:
        return None
    alt = buf[t[3] + 1:t[4] if len(t) == 5 else le]
    if stdin:
        pos, toks = pos_stdin(buf[t[0] + 1:t[1]]), alt.split(b",")
    else:
        pos, toks = pos_file(buf, t[0] + 1), [x for x in alt.split(b",") if x]
    return buf[ls:t[0]], pos, buf[t[2] + 1:t[3]], tuple(sorted(toks))


def line_spans(buf):
    """[ls, le) of every line: split at '\\n' only; bytes after the last one are a line"""
    out, p, n = [], 0, len(buf)
    while p < n:
        k = buf.find(b"\n", p)
        if k < 0:
            k = n
        out.append((p, k))
        p = k + 1
    return out


def statuses(buf, stdin):
    """per line its VCFXG_DD_* status, and per line the line its key first stood on (else None)"""
    seen, st, first = {}, [], []
    for i, (ls, le) in enumerate(line_spans(buf)):
        first.append(None)
        if le == ls:
            st.append(EMPTY)
        elif buf[ls:ls + 1] == b"#":
            st.append(HEADER)
        else:
            k = line_key(buf, ls, le, stdin)
            if k is None:
                st.append(SHORT)
            elif k in seen:
                st.append(DUP)
                first[-1] = seen[k]
            else:
                seen[k] = i
                st.append(KEPT)
    return st, first


def dedupe(buf, stdin, quiet=False):
    """(stdout, stderr, rc) of one mode over the input bytes"""
    st, _ = statuses(buf, stdin)
    out = b"".join(buf[ls:le] + b"\n" for (ls, le), s in zip(line_spans(buf), st) if s in (KEPT, HEADER))
    return out, b"" if quiet else WARN * st.count(SHORT), 0


def run(argv, stdin=b"", cwd=None):
    """main :393-399 and run :31-86: (stdout, stderr, rc)"""
    args = argv[1:]
    if "--help" in args or "-h" in args:  # vcfx::handle_common_flags
        return HELP, b"", 0
    if "--version" in args or "-v" in args:
        return VERSION, b"", 0
    opts, operands = getopt_long(argv)
    path, quiet, help_, err = None, False, False, b""
    for k, v, msg in opts:
        err += msg
        if k == "i":
            path = v
        elif k == "q":
            quiet = True
        else:
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
        o, e, rc = dedupe(buf, False, quiet)
        return o, err + e, rc
    o, e, rc = dedupe(stdin or b"", True, quiet)
    return o, err + e, rc


# ---- golden cases --------------------------------------------------------------------------------

def load_cases():
    with gzip.open(os.path.join(GOLDEN, "duplicate_remover_cases.json.gz"), "rb") as f:
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

HDR = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS0\tS1\tS2\n"
BASES = (b"A", b"C", b"G", b"T", b"AC", b"GT", b"ACGT", b"<DEL>", b"<INS:ME>", b"*")


def record(chrom, pos, id_, ref, alt, rest=b".\tPASS\t.\tGT\t0/1\t1/1\t0|0"):
    return b"\t".join([chrom, pos, id_, ref, alt, rest])


def gen_vcf(seed, n, mix=False, crlf=False, final_newline=True, header=True):
    """n data lines of which roughly half repeat the key of an earlier one: as it stands under a new
    ID, with other sample columns, with the ALT tokens in another order; the rest are new keys, many
    one field away from an earlier key (CHROM, POS, REF, one ALT token, an ALT token twice).
    mix: '#' lines, empty lines and lines of fewer than four tabs in between."""
    rnd = random.Random(seed)
    keys, lines = [], []
    eol = b"\r\n" if crlf else b"\n"

    def new_key():
        k = rnd.choice((1, 1, 2, 3, 4, 8))
        return [rnd.choice((b"1", b"2", b"chr10", b"X")), b"%d" % rnd.randrange(1, 400), rnd.choice(BASES[:7]),
                [rnd.choice(BASES) for _ in range(k)]]

    def tail():
        return b".\tPASS\tDP=%d\tGT\t%s" % (rnd.randrange(99), b"\t".join(rnd.choice((b"0/0", b"0/1", b"1|1", b"./."))
                                                                           for _ in range(3)))

    while len(lines) < n:
        r = rnd.random()
        if keys and r < 0.5:
            c, p, ref, alts = rnd.choice(keys)
            alts = list(alts)
            how = rnd.randrange(3)
            if how == 1 or len(alts) == 1:
                pass
            else:
                rnd.shuffle(alts)
            rest = b".\tPASS\t.\tGT\t0/1\t1/1\t0|0" if how == 0 else tail()
            lines.append(record(c, p, b"rs%d" % rnd.randrange(10 ** 6), ref, b",".join(alts), rest))
            continue
        if keys and r < 0.7:  # a neighbour of an earlier key
            c, p, ref, alts = rnd.choice(keys)
            alts = list(alts)
            what = rnd.randrange(5)
            if what == 0:
                c = c + b"_alt"
            elif what == 1:
                p = b"%d" % (int(p) + 1)
            elif what == 2:
                ref = ref + b"A"
            elif what == 3:
                alts[rnd.randrange(len(alts))] += b"T"
            else:
                alts.append(alts[0])
            k = [c, p, ref, alts]
        else:
            k = new_key()
        keys.append(k)
        lines.append(record(k[0], k[1], b".", k[2], b",".join(k[3]), tail()))
    out = []
    for ln in lines:
        if mix:
            r = rnd.random()
            if r < 0.05:
                out.append(b"")
            elif r < 0.10:
                out.append(b"#comment %d" % len(out))
            elif r < 0.14:
                out.append(rnd.choice((b"1\t5\t.\tA", b"1\t5", b"x", b"1\t5\t.\t")))
        out.append(ln)
    body = eol.join(out) + (eol if final_newline else b"")
    return (HDR.replace(b"\n", eol) if header else b"") + body


def nontrivial(buf, stdin):
    """(data lines, dropped lines, dropped lines whose ALT bytes differ from their first occurrence's,
    dropped lines equal to it in CHROM..ALT bytes but for ID)"""
    st, first = statuses(buf, stdin)
    spans = line_spans(buf)
    data = sum(s in (KEPT, DUP) for s in st)
    alt_order = same_but_id = 0

    def fields(i):
        return buf[spans[i][0]:spans[i][1]].split(b"\t")

    for i, s in enumerate(st):
        if s == DUP:
            a, b = fields(i), fields(first[i])
            alt_order += a[4] != b[4]
            same_but_id += (a[0], a[1], a[3], a[4]) == (b[0], b[1], b[3], b[4]) and (a[2] != b[2] or a[5:] != b[5:])
    return data, st.count(DUP), alt_order, same_but_id


# the generated inputs the GPU tests use: name -> gen_vcf arguments
GENERATED = {
    "g600": dict(seed=600, n=600),
    "n255": dict(seed=255, n=255, header=False),
    "n256": dict(seed=256, n=256, header=False),
    "n257": dict(seed=257, n=257, header=False),
    "n4097": dict(seed=4097, n=4097),
    "mix": dict(seed=7, n=500, mix=True),
    "mix_crlf": dict(seed=8, n=300, mix=True, crlf=True),
    "mix_no_final_newline": dict(seed=9, n=300, mix=True, final_newline=False),
    "routes": dict(seed=10, n=2000, mix=True),
}


def generated(name):
    return gen_vcf(**GENERATED[name])
