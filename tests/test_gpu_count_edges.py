"""Allele frequency and Hardy-Weinberg text over the count space, against exact arithmetic
(tests/_exact_num.py -- held to the C oracle by tests/test_exact_num_ref.py).

AF: the (alt, total) pairs with total <= 5,008 whose frequency lies within 1/4000 of a tie at the
fifth decimal (near_tie_pairs: 11,214 of the 12,547,544 pairs).  They hold every pair on which
the two input modes' rounding rules print different digits (3,778), every exact tie (8,000) and
every pair on which the file mode's fp64 sequence differs from exact half-up rounding (222).  One
file per bin of sample columns (32, 512, 1,536, 2,504).  The two lower bins hold their whole
selection.  All 6,784 ties of the two upper bins would take 58 MB as fixed-stride records alone,
so those bins hold every pair of the two classes on which a wrong rule or a reordered product
must show (the 3,778 and the 222: both are subsets of the ties) and a fixed every-k-th subset of the
rest; the GT:AD:DP layout, three times as wide, holds every k-th pair of each bin's list.  The inputs
total under 40 MB (asserted).

HWE: every (hom-ref, het, hom-alt) with N <= 40 in 40 columns (12,341 triples: all-het, no-het,
monomorphic and single-sample cases among them), and at 2,504 columns the extremes of
disequilibrium, their mirrors, and per N in (97, 301, 2504) and mode the 50 triples whose p-value
lies nearest to a value where the six-digit text changes.

Every check is byte-exact: the engine's rows (the walk and the two-sweep schedule), the drop-in
tools' output, the oracle's, and the reference's are the same bytes, and the counts are the counts
that were written."""
import os

import numpy as np
import pytest

from tests import _exact_num as X
from tests._golden import Oracle
from tests.test_gpu_hwe import _engine_text
from vcfx_amd import engine, tools

pytestmark = pytest.mark.gpu

T_MAX = 5008
BINS = (32, 512, 1536, 2504)  # sample columns; a bin takes the totals above the bin before it
AF_HEAD = b"CHROM\tPOS\tID\tREF\tALT\tAllele_Frequency\n"
HWE_HEAD = b"CHROM\tPOS\tID\tREF\tALT\tHWE_pvalue\n"
# of the pairs outside the two kept classes, every k-th stays (upper bins); of a bin's list,
# every k-th is also written as GT:AD:DP
REST_STRIDE = {32: 1, 512: 1, 1536: 8, 2504: 20}
GTADP_STRIDE = {32: 1, 512: 8, 1536: 25, 2504: 60}


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def eng():
    return engine.Engine(0)


@pytest.fixture(scope="module")
def af_bins():
    """{(columns, layout): (pairs, file bytes)}"""
    sel = X.near_tie_pairs(T_MAX)
    differ, ties, off_half_up = X.af_classes(T_MAX)
    keep = differ | off_half_up
    assert (len(sel), len(differ), len(ties), len(off_half_up)) == (11214, 3778, 8000, 222)
    out, lo = {}, 0
    for ncols in BINS:
        inbin = [(a, t) for a, t in sel.tolist() if lo < t <= 2 * ncols]
        lo = 2 * ncols
        kept = [p for p in inbin if p in keep]
        rest = [p for p in inbin if p not in keep][::REST_STRIDE[ncols]]
        pairs = sorted(kept + rest, key=lambda p: (p[1], p[0]))
        assert set(kept) <= set(pairs) and any(p in differ for p in pairs)
        out[(ncols, "gt")] = (pairs, X.af_vcf(pairs, ncols, "gt", seed=ncols))
        sub = pairs[::GTADP_STRIDE[ncols]]
        out[(ncols, "gtadp")] = (sub, X.af_vcf(sub, ncols, "gtadp", seed=ncols + 1))
    assert sum(len(b) for _, b in out.values()) <= 40 * 10 ** 6
    assert set(p for (n, l), (ps, _) in out.items() if l == "gt" for p in ps) >= keep
    return out


@pytest.mark.parametrize("layout", ["gt", "gtadp"])
@pytest.mark.parametrize("ncols", BINS)
def test_af_pairs(eng, oracle, af_bins, ncols, layout, tmp_path):
    pairs, buf = af_bins[(ncols, layout)]
    want_alt = np.array([p[0] for p in pairs], np.int32)
    want_tot = np.array([p[1] for p in pairs], np.int32)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    print("af %d columns, %s: %d pairs, %d bytes" % (ncols, layout, len(pairs), len(buf)))
    for mode in (engine.MODE_FILE, engine.MODE_STDIN):
        want = X.af_rows(pairs, mode)
        argv = ["VCFX_allele_freq_calc", "-q"] + (["-i", str(path)] if mode == engine.MODE_FILE else [])
        stdin = b"" if mode == engine.MODE_FILE else buf
        ref = oracle.run(argv, stdin)
        assert ref[0] == AF_HEAD + want
        ralt, rtot = oracle.af_counts(buf, stdin_mode=(mode == engine.MODE_STDIN))
        assert np.array_equal(ralt, want_alt) and np.array_equal(rtot, want_tot)
        ds = engine.data_start_of(buf, strip_cr=(mode == engine.MODE_FILE))
        for name in ("region", "index + allele_freq"):
            eng.load(buf)
            if name == "region":
                s = eng.allele_freq_region(ds, mode)
            else:
                eng.index(ds)
                s = eng.allele_freq(mode)
            alt, tot, st = eng.lines(s.n_lines)
            rows = st == 1
            assert s.rows == len(pairs) == int(rows.sum()), (name, mode)
            bad = np.nonzero((alt[rows] != want_alt) | (tot[rows] != want_tot))[0]
            assert len(bad) == 0, (name, mode, [(pairs[i], int(alt[rows][i]), int(tot[rows][i])) for i in bad[:5]])
            got = eng.text(s.text_bytes)
            if got != want:
                g, w = got.split(b"\n"), want.split(b"\n")
                diff = [(pairs[i], g[i], w[i]) for i in range(min(len(g), len(w)) - 1) if g[i] != w[i]]
                assert False, (name, mode, len(diff), diff[:5])
            if layout == "gt":
                assert s.general_records == 0, (name, mode)
        assert tools.run(argv, stdin) == ref, mode


def _hwe_cases(which, layout):
    if which == "small":
        return X.small_triples(), 40
    large = X.large_triples()
    # (GT:AD:DP records of 2,504 samples are 30 KB each: the hand-picked head and every 4th of the rest)
    return (large if layout == "gt" else large[:20] + large[20::4]), 2504


@pytest.mark.parametrize("layout", ["gt", "gtadp"])
@pytest.mark.parametrize("which", ["small", "large"])
def test_hwe_triples(oracle, which, layout, tmp_path):
    """The engine's rows after patching the rows hwe_rechecks() lists (the p-values within the
    safety margin of a print boundary, which the host recomputes): every unlisted row must be
    right as the device wrote it.  With the C library's exp no p-value of these lists comes
    within 4,000 units in the last place of a boundary, so the list is expected to be empty; it
    is printed, not asserted."""
    triples, ncols = _hwe_cases(which, layout)
    buf = X.hwe_vcf(triples, ncols, layout, seed=7 + ncols)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    print("hwe %s, %s: %d triples, %d bytes" % (which, layout, len(triples), len(buf)))
    for mode in (engine.MODE_FILE, engine.MODE_STDIN):
        want = X.hwe_rows(triples, mode)
        argv = ["VCFX_hwe_tester"] + (["-q", str(path)] if mode == engine.MODE_FILE else [])
        stdin = b"" if mode == engine.MODE_FILE else buf
        ref = oracle.run(argv, stdin)
        assert ref[0] == HWE_HEAD + want
        offs = np.cumsum([0] + [len(r) + 1 for r in want.split(b"\n")[:-1]])  # row starts
        for fused in ("7", "8"):  # the walk; the two-sweep schedule
            s, text, rc = _engine_text(buf, mode, {"VCFXG_AF_FUSED": fused})
            assert s.rows == len(triples) and len(text) == len(want), (mode, fused)
            print("hwe %s, %s, mode %d, schedule %s: %d rows left to the host" % (which, layout, mode, fused, len(rc)))
            t = bytearray(text)
            for off, a, b, c in rc:
                i = int(np.searchsorted(offs, off, side="right")) - 1
                assert (a, b, c) == tuple(triples[i]) and t[off + 8:off + 9] == b"\n" and t[off - 1:off] == b"\t"
                t[off:off + 8] = want[off:off + 8]
            if bytes(t) != want:
                g, w = bytes(t).split(b"\n"), want.split(b"\n")
                diff = [(triples[i], g[i], w[i]) for i in range(len(w) - 1) if g[i] != w[i]]
                assert False, (mode, fused, len(diff), diff[:5])
        assert tools.run(argv, stdin) == ref, mode
