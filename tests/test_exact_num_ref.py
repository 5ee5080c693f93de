"""The exact-arithmetic references of tests/_exact_num.py held to the C oracle and to Python's own
float conversions, and the allele-frequency pair selector pinned -- without a device.

The GPU tests (test_gpu_num_edges.py, test_gpu_count_edges.py) compare the engine with these
references; here the references are compared with independent implementations of the same
operations: glibc's strtod through the oracle's VCFX_record_filter, its printf, the oracle's
restated formatters, and float() / float.fromhex."""
import ctypes
import itertools
from fractions import Fraction

import numpy as np
import pytest

from tests import _exact_num as X
from tests._golden import Oracle

# the fixed junk list of the record filter's hand-picked edges (strings only: no device use)
from tests.test_gpu_rf import EDGE_VALUES

T_MAX = 5008  # 2,504 diploid samples


@pytest.fixture(scope="module")
def oracle():
    o = Oracle()
    L = o.lib
    for name in ("oracle_fmt_fixed4", "oracle_fmt_double4", "oracle_hwe_fmt_mmap"):
        getattr(L, name).restype = ctypes.c_size_t
        getattr(L, name).argtypes = [ctypes.c_double, ctypes.c_char_p]
    L.oracle_hwe_pvalue.restype = ctypes.c_double
    L.oracle_hwe_pvalue.argtypes = [ctypes.c_int] * 3
    return o


def _fmt(lib, name, v):
    b = ctypes.create_string_buffer(64)
    n = getattr(lib, name)(v, b)
    return b.raw[:n]


@pytest.fixture(scope="module")
def selected():
    return X.near_tie_pairs(T_MAX)


# ---------------------------------------------------------------------------------------------
# strtod
# ---------------------------------------------------------------------------------------------
def test_to_double_against_python_floats():
    """to_double (integers only) against float() and float.fromhex on every generated text that
    Python's grammar also accepts, on random rationals, and at the range's ends"""
    import random
    n = 0
    for t in X.edge_texts(EDGE_VALUES):
        v = X.parse(t)
        if v is None or isinstance(v, tuple):
            continue
        s = t.decode("latin1")
        try:
            f = float.fromhex(s) if "x" in s.lower() else float(s)
        except (ValueError, OverflowError):  # (float.fromhex raises on overflow, where strtod gives inf)
            assert X.to_bits(v) & ~(1 << 63) == 0x7FF << 52, t[:80]
            continue
        assert X.to_double(v) == f and (v == 0 or X.to_bits(v) == X.float_to_bits(f)), t[:80]
        n += 1
    assert n > 700
    rng = random.Random(7)
    for _ in range(3000):
        q = Fraction(rng.getrandbits(rng.randrange(1, 200)) + 1, rng.getrandbits(rng.randrange(1, 200)) + 1)
        q *= Fraction(2) ** rng.randrange(-1100, 1000)
        try:
            f = q.numerator / q.denominator  # (int / int is correctly rounded in CPython)
        except OverflowError:
            f = float("inf")
        assert X.to_bits(q) == X.float_to_bits(f)
        assert X.to_bits(-q) == X.float_to_bits(-f)
    top = Fraction(2) ** 1024 - Fraction(2) ** 970  # DBL_MAX + half an ulp: the tie goes to inf
    assert X.to_bits(top) == 0x7FF << 52 and X.to_bits(top - Fraction(1, 10 ** 400)) == X.DBL_MAX_BITS
    assert X.to_bits(Fraction(1, 2 ** 1075)) == 0 and X.to_bits(Fraction(3, 2 ** 1076)) == 1
    assert X.to_bits(Fraction(1, 2 ** 1075) + Fraction(1, 10 ** 2000)) == 1
    # every bit pattern's value rounds back to the pattern
    for _ in range(2000):
        b = rng.getrandbits(64)
        if (b >> 52) & 0x7FF != 0x7FF:
            assert X.to_bits(X.bits_value(b)) == b or b == 1 << 63


def test_edge_texts_straddle_every_boundary():
    """for every finite threshold the generated texts lie strictly between the neighbouring
    double and the boundary, exactly on it, and strictly between it and the threshold"""
    vals = [v for v in (X.parse(t) for t in X.edge_texts(EDGE_VALUES)) if isinstance(v, Fraction)]
    n = 0
    for bits in X.edge_thresholds():
        t = X.bits_value(bits)
        if isinstance(t, tuple):
            continue
        b = X.bounds(bits)
        for key in ("lo", "hi"):
            m = Fraction(b[key][0]) * Fraction(2) ** b[key][1]
            other = 2 * m - t  # the neighbouring double (2^1024 beyond DBL_MAX)
            lo, hi = min(other, t), max(other, t)
            assert any(lo < v < m for v in vals), (hex(bits), key, "below")
            assert any(v == m for v in vals), (hex(bits), key, "on")
            assert any(m < v < hi for v in vals), (hex(bits), key, "above")
            n += 1
    assert n >= 2 * 19


def _rf_cases():
    texts = X.edge_texts(EDGE_VALUES)
    buf, what = X.rf_vcf(texts)
    return texts, buf, what


def test_passes_against_the_oracle_record_filter(oracle):
    """every threshold x operator x QUAL / INFO: the lines the oracle's VCFX_record_filter (glibc
    strtod on both sides) keeps are the lines `passes` keeps"""
    texts, buf, what = _rf_cases()
    lines = buf.split(b"\n")
    first = next(i for i, l in enumerate(lines) if l.startswith(b"#CHROM")) + 1
    head, data = lines[:first], lines[first:-1]
    assert len(data) == len(what) == 2 * len(texts)
    for bits in X.edge_thresholds():
        arg = X.threshold_arg(bits)
        for op, field in itertools.product(X.OPS, ("QUAL", "X")):
            want = X.rf_expected(what, field, op, bits)
            out, _, rc = oracle.run(["VCFX_record_filter", "--filter", field + op + arg], buf)
            assert rc == 0
            assert out == b"".join(l + b"\n" for l in head + [d for d, w in zip(data, want) if w]), (field, op, arg)


# ---------------------------------------------------------------------------------------------
# allele frequency text
# ---------------------------------------------------------------------------------------------
def test_af_text_against_the_oracle_formats(oracle, selected):
    """file mode prints through writeDouble4 (oracle_fmt_double4), stdin mode through printf
    "%.4f" (oracle_fmt_fixed4), each on the fp64 quotient a / t"""
    assert len(selected) == 11214
    for a, t in selected.tolist():
        f = a / t
        assert X.af_text(a, t, X.MODE_FILE) == _fmt(oracle.lib, "oracle_fmt_double4", f), (a, t)
        assert X.af_text(a, t, X.MODE_STDIN) == _fmt(oracle.lib, "oracle_fmt_fixed4", f) == b"%.4f" % f, (a, t)
    assert X.af_text(0, 0, X.MODE_FILE) == X.af_text(0, 0, X.MODE_STDIN) == b"0.0000"


@pytest.fixture(scope="module")
def classes():
    return X.af_classes(T_MAX)


def test_selector_and_its_classes(selected, classes):
    """counted over all 12,547,544 pairs (af_classes), not over the selection only"""
    differ, ties, off_half_up = classes
    sel = set(map(tuple, selected.tolist()))
    assert len(sel) == len(selected) == 11214
    tt = selected[:, 1]
    assert (int((tt <= 64).sum()), int(((tt > 64) & (tt <= 1024)).sum()), int((tt > 1024).sum())) == (32, 1184, 9998)
    assert (len(differ), len(ties), len(off_half_up)) == (3778, 8000, 222)
    assert differ <= sel and ties <= sel and off_half_up <= sel
    # A fused multiply-add in the file rule changes no digit at these totals: the product k + 1/2 -
    # eps and the sum k + 1 - eps lie in one binade, so rounding once or twice decides alike.  (A
    # reordered product, a * 10000 / t, does show: on the 222.)  So no input up to 5,008 alleles can
    # tell the two apart; the device keeps the unfused sequence because that is the reference's.
    assert X.af_fma_sensitive(ties) == set()
    # the vectorised classes against the scalar reference on the selection, and on pairs outside it
    for a, t in selected.tolist():
        kf, ks = X.af_scaled(a, t, X.MODE_FILE), X.af_scaled(a, t, X.MODE_STDIN)
        assert (kf != ks) == ((a, t) in differ) and (kf != X.af_half_up(a, t)) == ((a, t) in off_half_up)
    rng = np.random.default_rng(5)
    for t in rng.integers(1, T_MAX + 1, 3000).tolist():
        a = int(rng.integers(0, t + 1))
        if (a, t) not in sel:
            assert X.af_scaled(a, t, X.MODE_FILE) == X.af_scaled(a, t, X.MODE_STDIN) == X.af_half_up(a, t)


# ---------------------------------------------------------------------------------------------
# Hardy-Weinberg text
# ---------------------------------------------------------------------------------------------
def test_hwe_text_against_the_oracle(oracle):
    small = X.small_triples()
    assert len(small) == 12341
    exact1 = 0
    for h in small + X.large_triples():
        v = oracle.lib.oracle_hwe_pvalue(*h)
        mine, through_exp = X.hwe_pvalue(*h)
        assert X.float_to_bits(mine) == X.float_to_bits(v), h
        exact1 += (not through_exp) and sum(h) <= 40
        assert X.hwe_text(*h, X.MODE_FILE) == _fmt(oracle.lib, "oracle_hwe_fmt_mmap", v), h
        assert X.hwe_text(*h, X.MODE_STDIN) == b"%.6f" % v, h
    assert exact1 == 986
    # distinct six-digit texts over the small triples: truncated (file mode) and rounded (stdin)
    assert len({X.hwe_text(*h, X.MODE_FILE) for h in small}) == 4514
    assert len({X.hwe_text(*h, X.MODE_STDIN) for h in small}) == 4521
    assert sum(X.hwe_pvalue(*h)[1] for h in small) == 11355
    assert X.hwe_text(2504, 0, 0, X.MODE_FILE) == b"1.000000" and X.hwe_text(1252, 0, 1252, X.MODE_STDIN) == b"0.000000"


def test_dyadic_decimal():
    assert X.dyadic_decimal(0, 5) == (0, 0, "")
    assert X.dyadic_decimal(1, -1) == (1, 0, "5")
    assert X.dyadic_decimal(-3, 2) == (-1, 2, "12")
    assert X.dyadic_decimal(5, 3) == (1, 2, "4")
    assert X.dyadic_decimal(1, -1074)[1] == -323 and len(X.dyadic_decimal(1, -1074)[2]) == 751
    for n, k in ((12345, -20), (2 ** 53 - 1, 971), (7, -1075)):
        s, e, d = X.dyadic_decimal(n, k)
        assert s * Fraction(int(d), 10 ** len(d)) * Fraction(10) ** e == Fraction(n) * Fraction(2) ** k
        assert X.parse(X.decimal_text(n, k)) == Fraction(n) * Fraction(2) ** k
