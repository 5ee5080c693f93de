"""The AF GT-only walk's sweep depths (k_af_walk<AfOp, false, depth, rolling>, depth 6 / 8 / 10 /
12 wave-steps of 1 KiB): every compiled depth, forced with VCFXG_AF_DEPTH through a fresh Engine,
must give the two-sweep schedule's lines, text and call summary on the same bytes, and the
oracle's VCFX_allele_freq_calc text -- byte for byte.

A record's sweep covers [b0, E): b0 = its sample start rounded down to 16, E its end (before a
'\\r').  Er = E - b0 is 4 * samples - 1 plus 0..15, so it varies with the head length (POS).  A
record of Er <= depth KiB is one batch; a longer one continues rolling, batch after batch.  The
sample counts put Er just below, at and just above every wave-step edge that is a batch edge of
some depth (6, 8, 10, 12 KiB and their multiples), and give rolling records of one to five
batches; the cases assert from the record offsets which side of its edge each input reaches."""
import functools
import tempfile

import numpy as np
import pytest

from tests._golden import Oracle
from vcfx_amd import engine, synth

pytestmark = pytest.mark.gpu

DEPTHS = (6, 8, 10, 12)
STEP = 1024
RECORDS = 240
SAMPLES = (128, 255, 256, 257, 1535, 1536, 1537, 2047, 2049, 2504, 2559, 2560, 2561, 3071, 3072, 3073, 4000, 5000, 6200)
# (5000: the three-batch record of depth 8; the others give one to five batches at the other depths)
# (name, missing_rate, irregular_rate, crlf, cut the final newline, mode)
VARIANTS = {
    "missing": (0.01, 0.0, 0, False, engine.MODE_FILE),     # the per-allele path inside a batch
    "irregular": (0.0, 0.05, 0, False, engine.MODE_FILE),   # rejected predictions, re-sweeps, pending lines
    "crlf": (0.0, 0.0, 1, False, engine.MODE_FILE),
    "nofinalnl": (0.0, 0.0, 0, True, engine.MODE_FILE),
    "stdin": (0.0, 0.0, 0, False, engine.MODE_STDIN),
}
CASES = [("plain", n) for n in SAMPLES] + [(v, n) for v in VARIANTS for n in (2504, 3073)] + [("nofinalnl", 6200)]


def _engine(env):
    mp = pytest.MonkeyPatch()
    for k in ("VCFXG_AF_FUSED", "VCFXG_AF_DEPTH", "VCFXG_WALK_CHUNK"):
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    try:
        return engine.Engine(0)  # (the knobs are read when the context opens)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def engines():
    e = {d: _engine({"VCFXG_AF_FUSED": "7", "VCFXG_AF_DEPTH": str(d)}) for d in DEPTHS}
    e["two_sweep"] = _engine({"VCFXG_AF_FUSED": "8"})
    e["plan"] = _engine({})
    yield e
    for x in e.values():
        x.close()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def _input(variant, samples):
    miss, irr, crlf, cut, mode = VARIANTS.get(variant, (0.0, 0.0, 0, False, engine.MODE_FILE))
    buf = synth.generate(RECORDS, samples, 1000 + samples, 0, miss, 0, irr, crlf)
    return (buf[:-1] if cut else buf), mode


def sweep_ends(buf):
    """Er of every GT-only data record: its end (before a '\\r') relative to its sample start
    rounded down to 16"""
    out = []
    pos = 0
    for line in buf.split(b"\n"):
        start, pos = pos, pos + len(line) + 1
        if not line or line[:1] == b"#":
            continue
        f = line.split(b"\t", 9)
        if len(f) < 10 or f[8] != b"GT":
            continue
        s = start + len(line) - len(f[9])
        e = start + len(line) - (1 if line.endswith(b"\r") else 0)
        out.append(e - (s & ~15))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _reference(variant, samples):
    """(input, mode, data start) -- the expected results are added by the first test that needs them"""
    buf, mode = _input(variant, samples)
    return {"buf": buf, "mode": mode, "ds": engine.data_start_of(buf, strip_cr=(mode == engine.MODE_FILE))}


def _run(eng, ref):
    eng.load(ref["buf"])
    s = eng.allele_freq_region(ref["ds"], ref["mode"])
    alt, tot, st = eng.lines(s.n_lines)
    rows = st == 1  # (the counts of a line without a row are not part of the result)
    return {"status": st.tobytes(), "alt": alt[rows].tobytes(), "tot": tot[rows].tobytes(),
            "text": eng.text(s.text_bytes),
            "summary": (s.n_lines, s.rows, s.data_lines, s.warn_lines, s.general_records, s.text_bytes)}


def _expected(engines, oracle, variant, samples):
    ref = _reference(variant, samples)
    if "want" not in ref:
        ref["want"] = _run(engines["two_sweep"], ref)
        assert engines["two_sweep"].L.vcfxg_last_schedule(engines["two_sweep"].h) == b"af_two_sweep"
        with tempfile.NamedTemporaryFile(suffix=".vcf") as f:
            f.write(ref["buf"])
            f.flush()
            out, _, rc = oracle.run(["VCFX_allele_freq_calc", "-q", "-i", f.name])
        assert rc == 0
        ref["oracle_text"] = out
    return ref


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("variant,samples", CASES, ids=["%s-%d" % c for c in CASES])
def test_depth_matches_two_sweep_and_oracle(engines, oracle, variant, samples, depth):
    ref = _expected(engines, oracle, variant, samples)
    eng = engines[depth]
    got = _run(eng, ref)
    assert eng.L.vcfxg_last_schedule(eng.h) == b"af_walk"
    assert eng.last_af_depth() == (depth, True)
    for k in ("summary", "status", "alt", "tot", "text"):
        assert got[k] == ref["want"][k], k
    assert b"CHROM\tPOS\tID\tREF\tALT\tAllele_Frequency\n" + got["text"] == ref["oracle_text"]


@pytest.mark.parametrize("samples", SAMPLES)
def test_shapes_reach_both_sides_of_their_edge(samples):
    """4 * samples - 1 + (0..15) against the wave-step edges: an input whose range holds an edge
    has records on both sides of it; the others lie where their name says (just above an edge, or
    between edges)"""
    er = sweep_ends(_reference("plain", samples)["buf"])
    assert len(er) == RECORDS
    lo, hi = 4 * samples - 1, 4 * samples + 14
    assert er.min() >= lo and er.max() <= hi
    edge = hi // STEP * STEP
    if lo <= edge:  # (Er <= edge: the steps up to the edge hold the record)
        assert (er <= edge).any() and (er > edge).any(), (samples, edge)
    else:
        assert (lo - 1) // STEP == hi // STEP


def test_shapes_cover_every_batch_edge_and_rolling_depth():
    """both sides of every depth's first batch edge, and rolling records of one, two and three
    batches at every depth (up to five at depth 6)"""
    er = {n: sweep_ends(_reference("plain", n)["buf"]) for n in SAMPLES}
    for d in DEPTHS:
        edge = d * STEP
        assert any((e <= edge).any() and (e > edge).any() for e in er.values()), d
        batches = set()
        for e in er.values():
            batches.update(int(b) for b in np.unique((e + edge - 1) // edge))
        assert {1, 2, 3} <= batches, (d, batches)


def test_rolling_record_at_the_buffer_end():
    """the last record of the 6,200-sample input without a final newline rolls at every depth and
    ends on the buffer's last byte"""
    ref = _reference("nofinalnl", 6200)
    buf = ref["buf"]
    assert not buf.endswith(b"\n")
    last = sweep_ends(buf)[-1]
    assert last > max(DEPTHS) * STEP and buf.rfind(b"\t") + 4 == len(buf)


@pytest.mark.parametrize("samples,want", [(256, (6, False)), (2504, (10, True)), (6200, (6, False))])
def test_plan_chooses_depth(engines, samples, want):
    """knob unset: depth 10 for records of 10 wave-steps (the measured size), the batches of 6 for
    every other size"""
    ref = _reference("plain", samples)
    eng = engines["plan"]
    eng.load(ref["buf"])
    eng.allele_freq_region(ref["ds"], ref["mode"])
    assert eng.L.vcfxg_last_schedule(eng.h) == b"af_walk"
    assert eng.last_af_depth() == want


def test_uncompiled_depth_is_the_plans_choice():
    eng = _engine({"VCFXG_AF_DEPTH": "7"})
    try:
        ref = _reference("plain", 2504)
        eng.load(ref["buf"])
        eng.allele_freq_region(ref["ds"], ref["mode"])
        assert eng.last_af_depth() == (10, True)
    finally:
        eng.close()
