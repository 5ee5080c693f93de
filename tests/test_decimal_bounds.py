"""threshold_bounds (vcfxg_decimal.cpp, the host half of the device's exact numeric compare) against
fractions, without a device: tests/decimal_bounds_test.cpp is a program of its own, built with
vcfxg_decimal.cpp under ASan + UBSan; it reads doubles as bit patterns and prints the two decimal
rounding boundaries threshold_bounds makes for each.  Expected: the midpoints of the double and its
two neighbours as exact `Fraction`s, written out in full; a value exactly on a midpoint rounds to
the neighbour with the even significand (and the midpoint above DBL_MAX to inf)."""
import os
import random
import subprocess
from fractions import Fraction

from tests import _exact_num as X
from vcfx_amd import BUILD, REPO

SIGN = 1 << 63
INF = 0x7FF << 52


def patterns():
    out = [0, 1, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, INF - 1, INF, 0x7FF8 << 48,
           X.float_to_bits(1.0), X.float_to_bits(0.1), X.float_to_bits(2.0 ** 52), X.float_to_bits(2.0 ** 53)]
    for ex in range(1, 2047, 37):  # a power of two and its two neighbours (quarter-ulp low boundary)
        out += [(ex << 52) - 1, ex << 52, (ex << 52) + 1]
    out += [(2046 << 52) - 1, 2046 << 52, (2046 << 52) + 1, (2 << 52) - 1, 2 << 52]
    rng = random.Random(1160)
    out += [rng.getrandbits(63) for _ in range(300)]
    out += [rng.getrandbits(52) for _ in range(60)]          # subnormals
    out = [b for b in out if (b & ~SIGN) <= INF or b == 0x7FF8 << 48]
    seen, uniq = set(), []
    for b in out + [b | SIGN for b in out]:
        if b not in seen:
            seen.add(b)
            uniq.append(b)
    return uniq


def _decimal(q):
    """a dyadic Fraction as "sign,exp,inf,digits" the way the program prints a DecHost"""
    if q == 0:
        return "0,0,0,-"
    n, d = abs(q.numerator), q.denominator
    k = d.bit_length() - 1
    assert d == 1 << k
    s = str(n * 5 ** k)              # q = s / 10^k
    return "%d,%d,0,%s" % (-1 if q < 0 else 1, len(s) - k, s.rstrip("0"))


def expected(bits):
    t = X.bits_value(bits)
    if t == ("nan",):
        return "%016x 1" % bits
    mag = bits & ~SIGN
    sign = -1 if bits >> 63 else 1
    if mag == INF:
        # everything from DBL_MAX + half an ulp on rounds to inf: that midpoint itself too
        near = (X.bits_value(INF - 1) + Fraction(2) ** 1024) / 2
        lo, hi = (_decimal(near), "1,0,1,-") if sign > 0 else ("-1,0,1,-", _decimal(-near))
        return "%016x 0 %s %s %d %d" % (bits, lo, hi, int(sign > 0), int(sign < 0))
    if mag == 0:
        half = Fraction(1, 2 ** 1075)  # between 0 and the smallest subnormal: the tie goes to (even) 0
        return "%016x 0 %s %s 1 1" % (bits, _decimal(-half), _decimal(half))
    below = X.bits_value(mag - 1)
    above = X.bits_value(mag + 1) if mag + 1 < INF else Fraction(2) ** 1024
    a = abs(t)
    near, far = (a + below) / 2, (a + above) / 2
    even = int(mag & 1 == 0)  # the significand's last bit is the pattern's
    lo, hi = (near, far) if sign > 0 else (-far, -near)
    return "%016x 0 %s %s %d %d" % (bits, _decimal(lo), _decimal(hi), even, even)


def test_threshold_bounds_under_asan_and_ubsan():
    exe = os.path.join("build", "san", "decimal_bounds_asan")
    subprocess.check_call(["make", "-s", "-C", REPO, exe])
    assert os.path.dirname(os.path.join(REPO, exe)) == os.path.join(BUILD, "san")
    pats = patterns()
    assert len(pats) > 1000
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, exe)], input="".join("%016x\n" % b for b in pats).encode(),
                       capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    got = r.stdout.decode().splitlines()
    assert len(got) == len(pats)
    for b, line in zip(pats, got):
        assert line == expected(b), "%016x" % b


def test_the_reference_bounds_are_the_same_midpoints():
    """_exact_num.bounds (integers; the GPU test's texts are generated from it) against the
    midpoints as fractions"""
    for b in patterns():
        want = expected(b).split()
        got = X.bounds(b)
        assert got["kind"] == int(want[1])
        if got["kind"]:
            continue
        for key, w in (("lo", want[2]), ("hi", want[3])):
            if got[key][0] == "inf":
                assert w == "%d,0,1,-" % got[key][1]
            else:
                s, e, d = X.dyadic_decimal(*got[key])
                assert "%d,%d,0,%s" % (s, e, d or "-") == w, "%016x" % b
        assert (got["lo_to_t"], got["hi_to_t"]) == (int(want[4]), int(want[5])), "%016x" % b
