"""Exact-arithmetic references for the engine's number and text edges.

Everything here is Python `int` and `fractions.Fraction` (plus, where the operation under test
IS an fp64 sequence, Python floats: IEEE doubles, one correctly rounded operation at a time, no
fused multiply-add).  Nothing calls into the project's code.

  parse / to_double / relation / passes   strtod(field) OP threshold (VCFX_record_filter's
                                           parseDouble + compareDouble; the grammar is the one
                                           vcfxg_num.h states)
  af_text                                  VCFX_allele_freq_calc's frequency text, both modes
  hwe_text                                 VCFX_hwe_tester's p-value text, both modes
  dyadic_decimal / bounds                  n * 2^k as a normalised decimal; the two rounding
                                           boundaries of a double (what threshold_bounds makes)
  near_tie_pairs                           the (alt, total) pairs near a fifth-decimal tie
  *_vcf                                    small writers: count tuples -> VCF bytes
"""
import functools
import math
import struct
from fractions import Fraction

MODE_FILE, MODE_STDIN = 0, 1
OPS = (">", ">=", "<", "<=", "==", "!=")  # in the order of the engine's GT, GE, LT, LE, EQ, NE

_SPACE = b" \t\n\v\f\r"
_DIGITS = b"0123456789"
_HEX = b"0123456789abcdefABCDEF"
_NCHAR = b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ_"
# a decimal exponent beyond this is cut to it: such a value is far outside the doubles' range
# (10^+-5000 against 2^+-1075), so it rounds to inf or to zero either way
_EXP_CLAMP = 5000


def _exp_digits(s, p):
    """an optional exponent's "[sign]digits" at s[p:]: (value, end), or None if no digit follows"""
    q = p
    neg = False
    if q < len(s) and s[q] in b"+-":
        neg = s[q] == 0x2D
        q += 1
    d0 = q
    while q < len(s) and s[q] in _DIGITS:
        q += 1
    if q == d0:
        return None
    v = int(s[d0:q])
    return (-v if neg else v), q


def parse(text):
    """strtod over the whole field: None (nothing parsed, or bytes left over), ("nan",),
    ("inf", sign) or the exact rational the text denotes"""
    s = bytes(text)
    p = 0
    while p < len(s) and s[p] in _SPACE:
        p += 1
    sign = 1
    if p < len(s) and s[p] in b"+-":
        sign = -1 if s[p] == 0x2D else 1
        p += 1
    rest = s[p:]
    low = rest.lower()
    if low[:1] == b"i":
        return ("inf", sign) if low in (b"inf", b"infinity") else None
    if low[:1] == b"n":
        if low == b"nan":
            return ("nan",)
        # nan(n-char-sequence): without the closing parenthesis strtod stops after "nan"
        if low[:4] == b"nan(" and low[-1:] == b")" and all(c in _NCHAR for c in rest[4:-1]):
            return ("nan",)
        return None
    if low[:2] == b"0x":
        q = 2
        while q < len(rest) and rest[q] in _HEX:
            q += 1
        ip = rest[2:q]
        fp = b""
        if q < len(rest) and rest[q] == 0x2E:
            q += 1
            f0 = q
            while q < len(rest) and rest[q] in _HEX:
                q += 1
            fp = rest[f0:q]
        if not ip and not fp:
            return None  # strtod reads the "0" and stops at the 'x'
        bexp = 0
        if q < len(rest) and rest[q] in b"pP":
            e = _exp_digits(rest, q + 1)
            if e is not None:
                bexp, q = e
        if q != len(rest):
            return None
        m = int(ip + fp, 16)
        if m == 0:
            return Fraction(0)
        bexp = max(-_EXP_CLAMP * 4, min(_EXP_CLAMP * 4, bexp - 4 * len(fp) + m.bit_length())) - m.bit_length()
        return sign * (Fraction(m) * (Fraction(2) ** bexp))
    q = 0
    while q < len(rest) and rest[q] in _DIGITS:
        q += 1
    ip = rest[:q]
    fp = b""
    if q < len(rest) and rest[q] == 0x2E:
        q += 1
        f0 = q
        while q < len(rest) and rest[q] in _DIGITS:
            q += 1
        fp = rest[f0:q]
    if not ip and not fp:
        return None
    dexp = 0
    if q < len(rest) and rest[q] in b"eE":
        e = _exp_digits(rest, q + 1)
        if e is not None:
            dexp, q = e
    if q != len(rest):
        return None
    m = int(ip + fp)
    if m == 0:
        return Fraction(0)
    nd = len(str(m))
    dexp = max(-_EXP_CLAMP, min(_EXP_CLAMP, dexp - len(fp) + nd)) - nd
    return sign * (Fraction(m) * (Fraction(10) ** dexp))


_INF_BITS = 0x7FF << 52
_NAN_BITS = 0x7FF8 << 48
_SIGN_BIT = 1 << 63


def to_bits(q):
    """the IEEE-754 binary64 pattern of the rational q rounded to nearest, ties to even:
    overflow gives +-inf, small values subnormals or zero"""
    q = Fraction(q)
    if q == 0:
        return 0
    sb = _SIGN_BIT if q < 0 else 0
    n, d = abs(q.numerator), q.denominator
    # e with 2^52 <= q / 2^e < 2^53, but no smaller than the subnormals' -1074
    e = n.bit_length() - d.bit_length() - 53
    for _ in range(3):
        lo = (n << -e) if e < 0 else n
        dd = d if e < 0 else (d << e)
        if lo < (dd << 52):
            e -= 1
        elif lo >= (dd << 53):
            e += 1
        else:
            break
    e = max(e, -1074)
    num = (n << -e) if e < 0 else n
    den = d if e < 0 else (d << e)
    m, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (m & 1)):
        m += 1
    if m >> 53:  # (2^53 exactly: the carry of an all-ones significand)
        m >>= 1
        e += 1
    if m >> 52:
        if e > 971:
            return sb | _INF_BITS
        return sb | ((e + 1075) << 52) | (m & ((1 << 52) - 1))
    return sb | m  # subnormal (e == -1074), or zero


def bits_to_float(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def float_to_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def to_double(q):
    """the correctly rounded (half to even) double of the rational q, as a Python float"""
    return bits_to_float(to_bits(q))


def bits_value(b):
    """a binary64 pattern as ("nan",), ("inf", sign) or its exact rational"""
    sign = -1 if b >> 63 else 1
    ex = (b >> 52) & 0x7FF
    m = b & ((1 << 52) - 1)
    if ex == 0x7FF:
        return ("nan",) if m else ("inf", sign)
    if ex == 0:
        return sign * Fraction(m, 1 << 1074)
    return sign * (Fraction((1 << 52) | m) * Fraction(2) ** (ex - 1075))


@functools.lru_cache(maxsize=None)
def _strtod(text):
    """strtod's result for the field, as bits_value gives it; None when the parse fails"""
    v = parse(text)
    if v is None or isinstance(v, tuple):
        return v
    return bits_value(to_bits(v))


def _order(x, y):
    """-1 / 0 / +1 of two bits_value results, None if either is NaN"""
    if x == ("nan",) or y == ("nan",):
        return None

    def key(v):
        return (v[1], Fraction(0)) if isinstance(v, tuple) else (0, v)
    kx, ky = key(x), key(y)
    return (kx > ky) - (kx < ky)


@functools.lru_cache(maxsize=None)
def _relation(text, tb):
    v = _strtod(text)
    if v is None:
        return None
    r = _order(v, bits_value(tb))
    return "unordered" if r is None else r


def relation(text, t):
    """strtod(text) against the double t (a float or a bit pattern given as int): None when
    the parse fails, "unordered" when either side is NaN, else -1 / 0 / +1"""
    return _relation(bytes(text), t if isinstance(t, int) else float_to_bits(float(t)))


def _apply(op, rel):
    if rel == "unordered":
        return op == "!="
    return {">": rel > 0, ">=": rel >= 0, "<": rel < 0, "<=": rel <= 0, "==": rel == 0, "!=": rel != 0}[op]


def passes(text, op, t):
    """parseDouble(text) && compareDouble(x, op, t)"""
    rel = relation(text, t)
    return False if rel is None else _apply(op, rel)


def qual_passes(text, op, t):
    """evaluateCriterion on QUAL: an empty field and "." compare as 0.0"""
    return passes(b"0" if text in (b"", b".") else text, op, t)


# ---------------------------------------------------------------------------------------------
# allele frequency text
# ---------------------------------------------------------------------------------------------
def _half_even(num, den):
    k, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (k & 1)):
        k += 1
    return k


def af_scaled(a, t, mode):
    """the frequency a / t in units of 1e-4, as the mode's rule rounds it"""
    if t <= 0:
        return 0
    if mode == MODE_FILE:
        # writeDouble4: (unsigned long long)(v * 10000.0 + 0.5) in fp64
        return int(float(a) / float(t) * 10000.0 + 0.5)
    # printf("%.4f"): the exact binary value of fl(a / t), rounded half to even
    v = bits_value(to_bits(Fraction(a, t)))
    return _half_even(v.numerator * 10000, v.denominator)


def af_text(a, t, mode):
    k = af_scaled(a, t, mode)
    return b"%d.%04d" % (k // 10000, k % 10000)


def af_half_up(a, t):
    """a / t in units of 1e-4 by exact half-up rounding"""
    return (20000 * a + t) // (2 * t) if t > 0 else 0


def near_tie_pairs(T):
    """every (a, t), 1 <= t <= T, 0 <= a <= t, whose 10000 * a / t lies within 1/4000 of a tie
    k + 1/2 (r = 10000 a mod t, |2 r - t| * 2000 <= t): an (n, 2) int64 array ordered by t, a"""
    import numpy as np
    out = []
    a_all = np.arange(T + 1, dtype=np.int64)
    for t in range(1, T + 1):
        a = a_all[:t + 1]
        r = (10000 * a) % t
        sel = a[np.abs(2 * r - t) * 2000 <= t]
        if len(sel):
            out.append(np.stack([sel, np.full(len(sel), t, np.int64)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def af_classes(T):
    """Over every (a, t), 1 <= t <= T, 0 <= a <= t: the pairs whose two mode texts differ, the
    exact ties at the fifth decimal, and the pairs whose file-mode digits differ from exact
    half-up rounding -- three sets of (a, t).

    Vectorised.  The file rule is evaluated as it stands, in numpy float64 (one IEEE operation
    per step, as the reference's).  The stdin rule needs the exact binary value of fl(a / t)
    times 10000, rounded half to even: y = fl(fl(a / t) * 10000.0) is within one ulp(y) <= 2^-39
    of that product, so wherever y is further than 1e-9 from k + 1/2 the rounding is decided
    by y; the few other pairs are done in exact integers (af_scaled)."""
    import numpy as np
    differ, ties, off_half_up = set(), set(), set()
    a_all = np.arange(T + 1, dtype=np.int64)
    for t in range(1, T + 1):
        a = a_all[:t + 1]
        r = (10000 * a) % t
        f = a.astype(np.float64) / float(t)
        y = f * 10000.0
        k_file = (y + 0.5).astype(np.int64)
        k_up = (20000 * a + t) // (2 * t)
        fl = np.floor(y)
        k_stdin = np.floor(y + 0.5).astype(np.int64)
        unsure = np.nonzero(np.abs(y - fl - 0.5) <= 1e-9)[0]
        for i in unsure.tolist():
            k_stdin[i] = af_scaled(int(a[i]), t, MODE_STDIN)
        for i in np.nonzero(k_file != k_stdin)[0].tolist():
            differ.add((int(a[i]), t))
        for i in np.nonzero(2 * r == t)[0].tolist():
            ties.add((int(a[i]), t))
        for i in np.nonzero(k_file != k_up)[0].tolist():
            off_half_up.add((int(a[i]), t))
    return differ, ties, off_half_up


def af_fma_sensitive(ties):
    """the ties where a fused multiply-add in the file rule -- fl(v * 10000 + 0.5) in one
    rounding instead of two -- would print another digit"""
    out = set()
    for a, t in ties:
        v = bits_value(to_bits(Fraction(a, t)))
        fused = bits_value(to_bits(v * 10000 + Fraction(1, 2)))
        if fused.numerator // fused.denominator != af_scaled(a, t, MODE_FILE):
            out.add((a, t))
    return out


# ---------------------------------------------------------------------------------------------
# Hardy-Weinberg p-value text
# ---------------------------------------------------------------------------------------------
def hwe_pvalue(h0, h1, h2):
    """calculateHWE_chisq + chi2_pvalue_1df in the reference's operation order (Python floats,
    math.sqrt / math.exp): (value, went through exp())"""
    n = h0 + h1 + h2
    if n < 1:
        return 1.0, False
    dn = float(n)
    p = (2.0 * float(h0) + float(h1)) / (2.0 * dn)
    q = 1.0 - p
    if p <= 0.0 or p >= 1.0:
        return 1.0, False
    ex = (dn * p * p, dn * 2.0 * p * q, dn * q * q)
    ob = (float(h0), float(h1), float(h2))
    chi2 = 0.0
    for k in range(3):
        y = 0.0
        if ex[k] > 0.0:
            diff = abs(ob[k] - ex[k]) - 0.5
            if diff < 0.0:
                diff = 0.0
            y = (diff * diff) / ex[k]
        chi2 = y if k == 0 else chi2 + y
    if chi2 <= 0.0:
        return 1.0, False
    if chi2 > 700.0:
        return 0.0, False
    x = math.sqrt(chi2 * 0.5)
    t = 1.0 / (1.0 + 0.3275911 * x)
    y = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    return y * math.exp(-x * x), True


def fmt6(v, mode):
    """a p-value 0 <= v < 10 in the mode's six-digit format"""
    if mode == MODE_FILE:
        # appendDouble: the integer digit, then six times *10 and truncate, in fp64
        ip = int(v)
        fr = v - float(ip)
        out = b"%d." % ip
        for _ in range(6):
            fr = fr * 10.0
            d = int(fr)
            out += b"%d" % d
            fr = fr - float(d)
        return out
    # printf("%.6f"): the exact binary value, rounded half to even
    n, d = float(v).as_integer_ratio()
    k = _half_even(n * 1000000, d)
    return b"%d.%06d" % (k // 1000000, k % 1000000)


def hwe_text(h0, h1, h2, mode):
    return fmt6(hwe_pvalue(h0, h1, h2)[0], mode)


def hwe_boundary_ulps(v, mode):
    """how many representable doubles lie between v (0 < v < 1) and the nearest value that
    prints differently in the mode's format, rounded down: v's distance to a print boundary"""
    # the boundaries are k * 1e-6 (file: truncation; the repeated *10 is exact enough that the
    # estimate holds to a few ulps) and (k + 1/2) * 1e-6 (stdin)
    x = Fraction(v) * 1000000
    if mode == MODE_STDIN:
        x -= Fraction(1, 2)
    k = math.floor(x)
    dist = min(x - k, k + 1 - x) / 1000000
    ulp = Fraction(math.ulp(v))
    return int(dist / ulp)


# ---------------------------------------------------------------------------------------------
# decimal expansions of dyadic rationals
# ---------------------------------------------------------------------------------------------
def dyadic_decimal(n, k):
    """n * 2^k as (sign, exp, digits): value = sign * 0.<digits> * 10^exp, first and last digit
    nonzero; zero is (0, 0, "")"""
    if n == 0:
        return 0, 0, ""
    sign = -1 if n < 0 else 1
    n = abs(n)
    if k >= 0:
        s, scale = str(n << k), 0
    else:
        s, scale = str(n * 5 ** -k), -k
    return sign, len(s) - scale, s.rstrip("0")


def decimal_text(n, k):
    """n * 2^k written out in full as a plain decimal, e.g. b"-0.00123" """
    sign, exp, digits = dyadic_decimal(n, k)
    if sign == 0:
        return b"0"
    if exp <= 0:
        body = "0." + "0" * -exp + digits
    elif exp >= len(digits):
        body = digits + "0" * (exp - len(digits))
    else:
        body = digits[:exp] + "." + digits[exp:]
    return (("-" if sign < 0 else "") + body).encode()


def neighbours(b):
    """the bit patterns of the doubles just below and above the finite, positive or zero double
    with pattern b (a magnitude: the caller handles signs); above DBL_MAX comes inf"""
    return (b - 1 if b else None), b + 1


def _mag_dyadic(b):
    """magnitude pattern b (finite) as (M, e): value M * 2^e"""
    ex, m = (b >> 52) & 0x7FF, b & ((1 << 52) - 1)
    return (m, -1074) if ex == 0 else ((1 << 52) | m, ex - 1075)


def bounds(bits):
    """The interval of reals that strtod rounds to the double with this pattern, from the
    midpoints with its two neighbours: dict(kind, lo, hi, lo_to_t, hi_to_t) where lo / hi are
    (n, k) dyadics n * 2^k or ("inf", sign), and *_to_t says whether a value exactly on that
    end rounds to t (ties go to the even significand; the tie above DBL_MAX goes to inf).
    kind 1 = NaN (no interval)."""
    v = bits_value(bits)
    if v == ("nan",):
        return {"kind": 1}
    sign = -1 if bits >> 63 else 1
    mag = bits & ~_SIGN_BIT
    dbl_max = _INF_BITS - 1
    if mag == _INF_BITS:
        M, e = _mag_dyadic(dbl_max)
        near, far = (2 * M + 1, e - 1), ("inf", 1)
        near_to_t, far_to_t = 1, 0
    elif mag == 0:
        # both signs of zero: the interval is symmetric about 0, and half the smallest subnormal
        # is a tie between 0 (even) and it
        return {"kind": 0, "lo": (-1, -1075), "hi": (1, -1075), "lo_to_t": 1, "hi_to_t": 1}
    else:
        M, e = _mag_dyadic(mag)
        even = int(M % 2 == 0)
        # the midpoint with the successor (for DBL_MAX: with 2^1024, where inf would be)
        far = (2 * M + 1, e - 1)
        # the predecessor of a power of two (above the subnormals) is half as far away
        pM, pe = _mag_dyadic(mag - 1)
        # midpoint = (M 2^e + pM 2^pe) / 2 with pe <= e
        near = ((M << (e - pe)) + pM, pe - 1)
        near_to_t = far_to_t = even
    if sign > 0:
        return {"kind": 0, "lo": near, "hi": far, "lo_to_t": near_to_t, "hi_to_t": far_to_t}

    def neg(d):
        return ("inf", -d[1]) if d[0] == "inf" else (-d[0], d[1])
    return {"kind": 0, "lo": neg(far), "hi": neg(near), "lo_to_t": far_to_t, "hi_to_t": near_to_t}


# ---------------------------------------------------------------------------------------------
# VCF writers
# ---------------------------------------------------------------------------------------------
def _header(ncols):
    return (b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t"
            + b"\t".join(b"S%d" % i for i in range(ncols)) + b"\n")


_GT = [b"0|0", b"0|1", b"1|0", b"1|1", b".|.", b".|1", b".|0"]
_G00, _G01, _G10, _G11, _GMISS, _GX1, _GX0 = range(7)


def _record(i, fmt, samples):
    return b"21\t%d\trs%d\tA\tC\t50\tPASS\t.\t%s\t%s\n" % (1000 + i, i, fmt, samples)


def _write(code_rows, ncols, layout, seed):
    """records from per-record genotype codes (indices into _GT; padded with '.|.' to ncols and
    shuffled with the seed).  layout "gt": FORMAT GT, every sample 3 bytes (fixed stride);
    "gtadp": FORMAT GT:AD:DP, samples of varying width (the exact per-sample path)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    table = np.frombuffer(b"".join(g + b"\t" for g in _GT), np.uint8).reshape(len(_GT), 4)
    out = [_header(ncols)]
    for i, codes in enumerate(code_rows):
        row = np.full(ncols, _GMISS, np.int64)
        assert len(codes) <= ncols
        row[:len(codes)] = codes
        row = row[rng.permutation(ncols)]
        if layout == "gt":
            out.append(_record(i, b"GT", table[row].tobytes()[:-1]))
        else:
            out.append(_record(i, b"GT:AD:DP", b"\t".join(
                _GT[g] + b":%d,%d:%d" % (j % 13, (j * 7) % 11, j % 13 + (j * 7) % 11) for j, g in enumerate(row.tolist()))))
    return b"".join(out)


def af_rows(pairs, mode):
    """the rows VCFX_allele_freq_calc prints for af_vcf(pairs, ...), without the header line"""
    return b"".join(b"21\t%d\trs%d\tA\tC\t%s\n" % (1000 + i, i, af_text(int(a), int(t), mode))
                    for i, (a, t) in enumerate(pairs))


def hwe_rows(triples, mode):
    """the rows VCFX_hwe_tester prints for hwe_vcf(triples, ...), without the header line"""
    return b"".join(b"21\t%d\trs%d\tA\tC\t%s\n" % (1000 + i, i, hwe_text(*h, mode)) for i, h in enumerate(triples))


def af_vcf(pairs, ncols, layout, seed=0):
    """One record per (alt, total): `ncols` diploid samples holding `alt` 1-alleles among `total`
    called alleles: '.|.' pads the total, one '.|1' or '.|0' makes an odd total."""
    import numpy as np
    rows = []
    for a, t in pairs:
        a, t = int(a), int(t)
        assert 0 <= a <= t <= 2 * ncols
        odd = []
        if t & 1:
            odd = [_GX1 if a & 1 else _GX0]
            a -= a & 1
            t -= 1
        n11, n01 = a // 2, a & 1  # (a odd here only with an even t: one heterozygote)
        n00 = t // 2 - n11 - n01
        assert n00 >= 0
        rows.append(np.concatenate([np.array(odd, np.int64), np.full(n11, _G11), np.full(n01, _G01), np.full(n00, _G00)]))
    return _write(rows, ncols, layout, seed)


def hwe_vcf(triples, ncols, layout, seed=0):
    """One record per (hom-ref, het, hom-alt): that many 0|0, 0|1 / 1|0 and 1|1 samples"""
    import numpy as np
    rows = []
    for h0, h1, h2 in triples:
        het = np.where(np.arange(h1) & 1, _G01, _G10)
        rows.append(np.concatenate([np.full(h0, _G00), het, np.full(h2, _G11)]).astype(np.int64))
    return _write(rows, ncols, layout, seed)


def rf_vcf(texts, ncols=40, seed=0):
    """Every text once as QUAL and once as X= in INFO (the key at the front, in the middle and at
    the end of the field, by turns), each record with `ncols` genotype columns.  Returns (bytes,
    [(kind, text)] per data line), kind "QUAL" or "INFO"."""
    import numpy as np
    rng = np.random.default_rng(seed)
    gts = [b"0|0", b"0|1", b"1|0", b"1|1"]
    out, what = [_header(ncols)], []
    for i, x in enumerate(texts):
        g = b"\t".join(gts[int(k)] for k in rng.integers(0, 4, ncols))
        out.append(b"21\t%d\trs%d\tA\tC\t%s\tPASS\tDP=7;XX=1\tGT\t%s\n" % (2000 + 2 * i, i, x, g))
        what.append(("QUAL", x))
        info = (b"X=%s;DP=7;XX=1", b"DP=7;X=%s;XX=1", b"XX=1;DP=7;X=%s")[i % 3] % x
        out.append(b"21\t%d\trs%d\tA\tC\t50\tPASS\t%s\tGT\t%s\n" % (2001 + 2 * i, i, info, g))
        what.append(("INFO", x))
    return b"".join(out), what


# ---------------------------------------------------------------------------------------------
# generated edges of the numeric compare
# ---------------------------------------------------------------------------------------------
DBL_MAX_BITS = _INF_BITS - 1


def edge_thresholds():
    """about two dozen threshold bit patterns: everyday values, random normals, powers of two
    (quarter-ulp low boundary), an odd / even significand pair, subnormals, the range's ends,
    zero, a negative, the infinities and NaN"""
    import random
    rng = random.Random(20240611)
    f = float_to_bits
    out = [f(0.1), f(30.0)]
    for ex in (1, 700, 1023, 1100, 2046):  # random significands over the exponent range
        out.append((ex << 52) | rng.getrandbits(52))
    out.append(_SIGN_BIT | (1000 << 52) | rng.getrandbits(52))
    out += [1 << 52, 1023 << 52, (1023 + 60) << 52]       # 2^-1022, 1.0, 2^60
    out += [0x3FF123456789ABCD, 0x3FF123456789ABCE]          # odd, even significand
    out += [0x000123456789ABCD, (1 << 52) - 1, 1]            # subnormals: some, the largest, the smallest
    out += [DBL_MAX_BITS, 0, f(-0.1), _INF_BITS, _SIGN_BIT | _INF_BITS, _NAN_BITS]
    return out


def _plain(sign, exp, digits):
    """sign * 0.<digits> * 10^exp written without an exponent"""
    if exp <= 0:
        body = "0." + "0" * -exp + digits
    elif exp >= len(digits):
        body = digits + "0" * (exp - len(digits))
    else:
        body = digits[:exp] + "." + digits[exp:]
    return (("-" if sign < 0 else "") + body).encode()


def _hex_forms(n, k):
    """n * 2^k (n > 0) as hex floats: all digits before the point, and the point after the first"""
    h = "%x" % n
    out = [("0x%sp%d" % (h, k)).encode()]
    if len(h) > 1:
        out.append(("0X%s.%sP%+d" % (h[0], h[1:].upper(), k + 4 * (len(h) - 1))).encode())
    return out


def threshold_texts(bits):
    """Field texts around the finite threshold with this pattern, from the exact expansions: the
    threshold and its two neighbours, both rounding boundaries in full, nudged, cut short and
    extended, with the point moved and an exponent, decorated, and as hex floats."""
    v = bits_value(bits)
    if isinstance(v, tuple):
        return []
    b = bounds(bits)
    sgn = b"-" if bits >> 63 else b""
    mag = bits & ~_SIGN_BIT
    out = []
    # t, pred(t), succ(t) (by magnitude; succ(DBL_MAX) is 2^1024, which no double holds)
    for m in (mag, mag - 1, mag + 1):
        if m < 0:
            continue
        M, e = _mag_dyadic(m) if m <= DBL_MAX_BITS else (1, 1024)
        out.append(sgn + decimal_text(M, e))
    for key in ("lo", "hi"):
        n, k = b[key]
        sign, exp, digits = dyadic_decimal(n, k)
        full = _plain(sign, exp, digits)
        out.append(full)
        last = int(digits[-1])  # (5: the boundaries are odd multiples of a power of two)
        out.append(_plain(sign, exp, digits[:-1] + str(last - 1)))
        out.append(_plain(sign, exp, digits[:-1] + str(last + 1)))
        for cut in (1, 3, 9):
            if len(digits) > cut:
                out.append(_plain(sign, exp, digits[:-cut]))
        out.append(_plain(sign, exp, digits + "000"))
        out.append(_plain(sign, exp, digits + "0" * 40 + "1"))
        # the point moved, with an exponent
        s = "-" if sign < 0 else ""
        out.append(("%s%s.%se%d" % (s, digits[0], digits[1:], exp - 1)).encode())
        out.append(("%s%sE%+d" % (s, digits, exp - len(digits))).encode())
        out.append(("%s0.000%se%d" % (s, digits, exp + 3)).encode())
        # decorated
        mag_text = full.lstrip(b"-")
        out.append((b"-" if sign < 0 else b"") + b"000" + mag_text)
        out.append((b"-" if sign < 0 else b"+") + mag_text)
        out.append(b" " + full)
        out.append(b"\v \r" + full)
        out.append((b"" if sign < 0 else b"-") + mag_text)
        # hex: the boundary in 14 hex digits (n has 54 bits for a normal t) and in 20, where the
        # device keeps 16 digits and the rest decides tie or sticky
        hs = b"-" if n < 0 else b""
        for form in _hex_forms(abs(n), k):
            out.append(hs + form)
        wide = abs(n) << 24
        for w in (wide, wide + 1, wide - 1):
            for form in _hex_forms(w, k - 24):
                out.append(hs + form)
    if mag:
        M, e = _mag_dyadic(mag)
        for form in _hex_forms(M, e):
            out.append(sgn + form)
    return out


HEX_EDGES = [b"0x0.0000000000001p-1022", b"0x1p-1074", b"0x1p-1075", b"0x1.8p-1075", b"0x1.0000000000000001p-1075",
             b"0x1p-1076", b"0x0.8p-1073", b"0x123456789abcdp-1074", b"0x1p1024", b"0x1.fffffffffffff8p1023",
             b"0x1.fffffffffffff7fffp1023", b"0x1.fffffffffffffp1023", b"0x1p99999999999999999999",
             b"0x1p-99999999999999999999", b"0x0p99999999999999999999", b"-0x1p1024", b"0X1P3", b"0x.8", b"0x8.",
             b"0x.p1", b"0x1p", b"0x1.p+", b"0x1p-", b"0xg", b"0x1.2.3", b"0x00000000000000000000001p0",
             b"0x1000000000000000000000p-84", b"1e99999999999999999999", b"1e-99999999999999999999",
             b"0e99999999999999999999", b"1e+", b"1e-", b"1E5", b"1.e1", b".e1", b"1..2", b"1e5.0", b"infinit",
             b"infinityx", b"INF", b"+inf", b"nan(", b"nan()", b"nan(a_1)", b"nan(a-1)", b"nan(1)x", b"-nan",
             b"1 ", b"\x0c1", b"+-1", b"--1", b"+", b"-", b"1,5", b"1_0"]


def edge_texts(junk=()):
    """every generated field text once, in a fixed order: threshold_texts of every edge
    threshold, the hex and grammar edges, and the caller's junk list"""
    seen, out = set(), []
    for x in [t for b in edge_thresholds() for t in threshold_texts(b)] + HEX_EDGES + \
            [j.encode() if isinstance(j, str) else j for j in junk]:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def rf_expected(what, field, op, bits):
    """per data line of rf_vcf (its second result): does `field OP threshold` keep the line, for
    field "QUAL" or the INFO key "X"?  The lines that carry the text in the other place hold
    QUAL 50 and no X (an absent key fails every operator)."""
    q50 = qual_passes(b"50", op, bits)
    out = []
    for kind, text in what:
        if field == "QUAL":
            out.append(qual_passes(text, op, bits) if kind == "QUAL" else q50)
        else:
            out.append(passes(text, op, bits) if kind == "INFO" else False)
    return out


def threshold_arg(bits):
    """a threshold as the text of a --filter argument: strtod reads back exactly this double"""
    v = bits_value(bits)
    if v == ("nan",):
        return "nan"
    if isinstance(v, tuple):
        return "inf" if v[1] > 0 else "-inf"
    return repr(bits_to_float(bits))


# ---------------------------------------------------------------------------------------------
# Hardy-Weinberg count triples
# ---------------------------------------------------------------------------------------------
def small_triples(n_max=40):
    """every (hom-ref, het, hom-alt) with 0 <= N <= n_max"""
    return [(a, b, n - a - b) for n in range(0, n_max + 1) for a in range(n + 1) for b in range(n + 1 - a)]


def _hwe_pvalue_np(h0, h1, h2):
    """hwe_pvalue over int arrays in numpy float64 -- for ranking only: numpy's exp need not be
    the C library's in the last place.  NaN where the value does not go through exp()."""
    import numpy as np
    with np.errstate(all="ignore"):
        o = [h0.astype(np.float64), h1.astype(np.float64), h2.astype(np.float64)]
        dn = o[0] + o[1] + o[2]
        p = (2.0 * o[0] + o[1]) / (2.0 * dn)
        q = 1.0 - p
        ex = [dn * p * p, dn * 2.0 * p * q, dn * q * q]
        chi2 = None
        for k in range(3):
            diff = np.maximum(np.abs(o[k] - ex[k]) - 0.5, 0.0)
            y = np.where(ex[k] > 0.0, diff * diff / ex[k], 0.0)
            chi2 = y if chi2 is None else chi2 + y
        x = np.sqrt(chi2 * 0.5)
        t = 1.0 / (1.0 + 0.3275911 * x)
        y = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
        v = y * np.exp(-x * x)
        return np.where((p > 0.0) & (p < 1.0) & (chi2 > 0.0) & (chi2 <= 700.0), v, np.nan)


def hwe_nearest_boundary(n, mode, keep=50):
    """the `keep` triples with h0 + h1 + h2 == n whose p-value lies nearest, in units of its own
    last place, to a value where the mode's six-digit text changes: [(ulps, triple)], nearest
    first, the distance recomputed with math.exp (hwe_boundary_ulps)"""
    import numpy as np
    a = np.repeat(np.arange(n + 1, dtype=np.int64), n + 1)
    b = np.tile(np.arange(n + 1, dtype=np.int64), n + 1)
    ok = a + b <= n
    a, b = a[ok], b[ok]
    c = n - a - b
    v = _hwe_pvalue_np(a, b, c)
    with np.errstate(all="ignore"):
        x = v * 1e6 - (0.5 if mode == MODE_STDIN else 0.0)
        d = np.abs(x - np.round(x)) / (np.spacing(v) * 1e6)
    d = np.where(np.isnan(d), np.inf, d)
    idx = np.argsort(d, kind="stable")[:4 * keep]  # (ranked roughly; the exact distance sorts the short list)
    out = []
    for i in idx.tolist():
        h = (int(a[i]), int(b[i]), int(c[i]))
        pv, through_exp = hwe_pvalue(*h)
        if through_exp and 0.0 < pv < 1.0:
            out.append((hwe_boundary_ulps(pv, mode), h))
    out.sort()
    return out[:keep]


LARGE_HEAD = [(2504, 0, 0), (0, 2504, 0), (1252, 0, 1252), (1, 0, 2503), (1000, 1504, 0), (626, 1252, 626), (350, 0, 1),
              (351, 0, 1), (175, 0, 175), (2000, 4, 500)]
_large = {}


def large_triples(with_distance=False):
    """the large-N list: extreme disequilibrium and equilibrium by hand, their mirrors, and per
    N in (97, 301, 2504) and per mode the 50 triples nearest to a print boundary.  With
    with_distance: also the smallest distance found, in ulps, per (N, mode)."""
    if not _large:
        out = list(LARGE_HEAD)
        out += [h[::-1] for h in LARGE_HEAD if h[::-1] not in out]
        nearest = {}
        for n in (97, 301, 2504):
            for mode in (MODE_FILE, MODE_STDIN):
                found = hwe_nearest_boundary(n, mode)
                nearest[(n, mode)] = found[0][0]
                out += [h for _, h in found if h not in out]
        _large["list"], _large["nearest"] = out, nearest
    return (_large["list"], _large["nearest"]) if with_distance else _large["list"]
