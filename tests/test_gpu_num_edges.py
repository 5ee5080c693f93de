"""The device's exact numeric compare (vcfxg_num.h: strtod(field) OP threshold decided from the
field's digits against the two decimal boundaries vcfxg_decimal.cpp makes) on generated edges,
against exact arithmetic (tests/_exact_num.py -- held to glibc's strtod by
tests/test_exact_num_ref.py).

Thresholds: everyday values, random normals, powers of two, an odd / even significand pair,
subnormals, DBL_MAX, zero, a negative, the infinities, NaN.  Field texts, per threshold, from the
exact expansions: the threshold and its neighbours, both rounding boundaries in full (about 1,100
digits for the subnormals: heads that leave the walk's window and take k_fq_finish's own scan),
nudged by one in the last digit, cut short, extended with zeros and with a digit after 40 zeros,
with the point moved and an exponent, with leading zeros / '+' / white space / the other sign, and
as hex floats of 14 and 20 digits (the device keeps 16: tie and sticky); the hex and grammar
edges; and the hand-picked junk of test_gpu_rf.py.  Every text stands once as QUAL and once as
X= in INFO (front, middle, end), in records of 40 genotype columns.

Checked line by line, for every threshold x operator x place: index + the per-tool kernel, and
the filter / query walk on chunks of 128 KiB, 4 KiB and 1 KiB; and the drop-in tool against the
oracle's bytes for thresholds written as text."""
import itertools
import os

import numpy as np
import pytest

from tests import _exact_num as X
from tests._golden import Oracle
from tests.test_gpu_rf import EDGE_VALUES
from vcfx_amd import engine, tools

pytestmark = pytest.mark.gpu

OPCODE = {">": engine.GT, ">=": engine.GE, "<": engine.LT, "<=": engine.LE, "==": engine.EQ, "!=": engine.NE}


@pytest.fixture(scope="module")
def cases():
    """the input, and the expected status bytes per (threshold, operator, place) -- computed once,
    before any device call"""
    texts = X.edge_texts(EDGE_VALUES)
    buf, what = X.rf_vcf(texts)
    # the set holds texts on each side of, and on, both boundaries of every finite threshold
    vals = [v for v in (X.parse(t) for t in texts) if not isinstance(v, tuple) and v is not None]
    for bits in X.edge_thresholds():
        t = X.bits_value(bits)
        if isinstance(t, tuple):
            continue
        b = X.bounds(bits)
        for key in ("lo", "hi"):
            m = X.Fraction(b[key][0]) * X.Fraction(2) ** b[key][1]
            other = 2 * m - t
            assert any(min(other, t) < v < m for v in vals) and any(v == m for v in vals) \
                and any(m < v < max(other, t) for v in vals), (hex(bits), key)
    want = {}
    for bits in X.edge_thresholds():
        for op, field in itertools.product(X.OPS, ("QUAL", "X")):
            keep = np.array(X.rf_expected(what, field, op, bits))
            want[(bits, op, field)] = np.where(keep, 1, 2).astype(np.uint8)
    return buf, what, want


def _crit(bits, op, field):
    t = X.bits_to_float(bits)
    if field == "QUAL":
        return [(engine.QUAL, OPCODE[op], 1, t, "", "")]
    return [(engine.INFO, OPCODE[op], 1, t, "X", "")]


def _open(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return engine.Engine(0)  # the context reads the VCFXG_* knobs when it opens
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _compare(got, want, what, key):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (hex(key[0]), X.threshold_arg(key[0]), key[1], key[2], len(bad),
                           [(what[i][0], what[i][1][:60], int(got[i]), int(want[i])) for i in bad[:5]])


def test_per_tool_kernel_on_generated_edges(cases):
    """(a) vcfxg_index + vcfxg_record_filter"""
    buf, what, want = cases
    eng = _open({"VCFXG_FQ_WALK": "0"})
    ds = engine.data_start_of(buf)
    eng.load(buf)
    assert eng.index(ds) == len(what)
    for key, w in want.items():
        s = eng.record_filter(_crit(*key))
        _compare(eng.statuses(s.n_lines), w, what, key)
        assert s.rows == int((w == 1).sum())
    eng.close()


@pytest.mark.parametrize("chunk", [131072, 4096, 1024])
def test_walk_on_generated_edges(cases, chunk):
    """(b) vcfxg_record_filter_region with the walk forced: the compare on a wave's register copy
    of the head, and k_fq_finish's own scan for the heads that leave the window"""
    buf, what, want = cases
    eng = _open({"VCFXG_FQ_WALK": "1", "VCFXG_WALK_CHUNK": str(chunk)})
    ds = engine.data_start_of(buf)
    for key, w in want.items():
        eng.load(buf)
        s = eng.record_filter_region(ds, _crit(*key))
        assert s.n_lines == len(what)
        _compare(eng.statuses(s.n_lines), w, what, key)
        assert s.rows == int((w == 1).sum())
    eng.close()


# thresholds as the text of a --filter argument (the tool's own strtod, then threshold_bounds)
ARG_THRESHOLDS = ["0.1", "30", "2.2250738585072014e-308", "5e-324", "1.7976931348623157e308", "-0.1",
                  "0x1.123456789abcdp+0", "0X1.123456789ABCEP0", "1152921504606846976", "-inf", "nan"]


def test_tool_on_generated_edges(cases):
    buf, what, _ = cases
    oracle = Oracle()
    head = buf[:engine.data_start_of(buf)]
    lines = buf[len(head):].split(b"\n")[:-1]
    for thr in ARG_THRESHOLDS:
        tb = X.to_bits(X.parse(thr.encode())) if isinstance(X.parse(thr.encode()), X.Fraction) else \
            X.float_to_bits(float(thr))
        for op, field in itertools.product(X.OPS, ("QUAL", "X")):
            argv = ["VCFX_record_filter", "--filter", field + op + thr]
            got = tools.run(argv, buf)
            assert got == oracle.run(argv, buf), (field, op, thr)
            keep = X.rf_expected(what, field, op, tb)
            assert got[0] == head + b"".join(l + b"\n" for l, k in zip(lines, keep) if k), (field, op, thr)
