"""The AF walk's chunk layouts (VCFXG_WALK_LAYOUT: uniform, fit, taper:<div>:<g>, and split:<div>:<K1>
for a switch at a chosen dispatch round) compute what the uniform layout computes: for every
layout the output text and the per-line arrays are byte-identical to the uniform run's, and the
text is the oracle's; the layout the engine reports is the one asked for.

The knobs are read when a context opens, so each (chunk, layout) has a context of its own.
VCFXG_WALK_RESIDENT stands in for the device's resident walkers (4,096 on an MI355X: no input of
a test's size would make one generation), so that 100 walkers are six generations of 16.

Inputs (vcfx_amd.synth):
  a   600 records x 160 samples, chunk 4096: about 100 walkers, a grid not divisible by 8
  b   40 records x 2,504 samples, chunk 32 KiB: 10 KB records; its tapers come to short chunks
      under a record, so some walkers own no line
  b4  the same at chunk 4096: records straddle several full and short chunks, most walkers own no line
  cm  a with missing_rate 0.01, ci: a with irregular_rate 0.05: leftover lines and dirty walkers
      in short chunks"""
import tempfile

import numpy as np
import pytest

from tests._golden import Oracle
from vcfx_amd import engine, synth

pytestmark = pytest.mark.gpu

WAVES = 4
HEADER = b"CHROM\tPOS\tID\tREF\tALT\tAllele_Frequency\n"
# name -> (synth arguments, VCFXG_WALK_CHUNK, VCFXG_WALK_RESIDENT)
INPUTS = {
    "a": ((600, 160, 4245, 0, 0.0, 0, 0.0, 0), 4096, 16),
    "b": ((40, 2504, 4246, 0, 0.0, 0, 0.0, 0), 32768, 4),
    "b4": ((40, 2504, 4246, 0, 0.0, 0, 0.0, 0), 4096, 16),
    "cm": ((600, 160, 4247, 0, 0.01, 0, 0.0, 0), 4096, 16),
    "ci": ((600, 160, 4248, 0, 0.0, 0, 0.05, 0), 4096, 16),
}
# "default": VCFXG_WALK_LAYOUT unset, the plan's choice: taper:2:1 from one generation of the main chunk on
LAYOUTS = ["fit", "taper:2:1", "taper:4:1", "taper:4:2", "split:2:1", "split:4:last", "default"]


class Case:
    def __init__(self, name):
        args, self.chunk, self.resident = INPUTS[name]
        self.buf = synth.generate(*args)
        self.ds = engine.data_start_of(self.buf)
        with tempfile.NamedTemporaryFile(suffix=".vcf") as f:
            f.write(self.buf)
            f.flush()
            self.want_text, _, _ = Oracle().run(["VCFX_allele_freq_calc", "-q", "-i", f.name])
        self.uniform = self.run("uniform")

    def run(self, layout, resident=True):
        mp = pytest.MonkeyPatch()
        mp.setenv("VCFXG_WALK_CHUNK", str(self.chunk))
        if resident:
            mp.setenv("VCFXG_WALK_RESIDENT", str(self.resident))
        else:
            mp.delenv("VCFXG_WALK_RESIDENT", raising=False)
        if layout == "default":
            mp.delenv("VCFXG_WALK_LAYOUT", raising=False)
        else:
            mp.setenv("VCFXG_WALK_LAYOUT", layout)
        mp.delenv("VCFXG_AF_FUSED", raising=False)
        try:
            eng = engine.Engine(0)
            try:
                eng.load(self.buf)
                s = eng.allele_freq_region(self.ds, engine.MODE_FILE)
                assert eng.L.vcfxg_last_schedule(eng.h).decode() == "af_walk"
                alt, tot, st = eng.lines(s.n_lines)
                return dict(text=eng.text(s.text_bytes), alt=alt.copy(), tot=tot.copy(), st=st.copy(), rows=s.rows,
                            general=s.general_records, layout=eng.last_walk_layout())
            finally:
                eng.close()
        finally:
            mp.undo()


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(name)
        return cache[name]

    return get


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_uniform_layout_is_the_chunks_of_before_and_matches_the_oracle(cases, name):
    c = cases(name)
    u = c.uniform
    R = len(c.buf) - c.ds
    nw = -(-R // c.chunk)
    assert u["layout"] == dict(kind="uniform", C=c.chunk, Cs=c.chunk, K1=-1, grid=-(-nw // WAVES), walkers=nw,
                               resident=0, div=1, g=0)
    assert HEADER + u["text"] == c.want_text
    if name == "a":
        assert 90 <= nw <= 110 and u["layout"]["grid"] % 8 != 0
    if name == "cm":  # missing calls (still fixed-stride records)
        assert (u["tot"][u["st"] == 1] < 2 * 160).any()
    if name == "ci":
        assert u["general"] > 0  # lines left to the exact per-line path


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_layout_computes_what_uniform_computes(cases, name, layout):
    c = cases(name)
    u = c.uniform
    nw0, S = u["layout"]["walkers"], c.resident
    rounds0 = -(-u["layout"]["grid"] // 8)
    asked = layout
    if layout == "default":
        layout = "taper:2:1"
    kind, _, rest = layout.partition(":")
    if rest.endswith("last"):  # the switch at the uniform grid's last round
        layout = "%s:%s:%d" % (kind, rest.split(":")[0], rounds0 - 1)
    got = c.run("default" if asked == "default" else layout)
    assert got["text"] == u["text"]
    for k in ("alt", "tot", "st"):
        assert np.array_equal(got[k], u[k]), k
    assert (got["rows"], got["general"]) == (u["rows"], u["general"])
    assert HEADER + got["text"] == c.want_text
    # the layout that ran is the one asked for
    lay = got["layout"]
    R = len(c.buf) - c.ds
    G = nw0 // S
    assert G >= 1  # (every input here is at least one generation of its resident walkers)
    assert lay["kind"] == kind
    if kind == "split":
        div, K1 = (int(x) for x in layout.split(":")[1:])
        assert (lay["C"], lay["Cs"], lay["K1"], lay["div"], lay["g"]) == (c.chunk, c.chunk // div, K1, div, K1)
        full = min(8 * K1 * WAVES * c.chunk, R)
        if R > full:  # short walkers ran
            assert lay["walkers"] > -(-full // c.chunk) and lay["grid"] > 8 * K1
        return
    div, g = (int(x) for x in layout.split(":")[1:]) if kind == "taper" else (1, 0)
    unit = 16 * div
    C = lay["C"]
    assert lay["resident"] == S and C >= c.chunk and C % unit == 0 and G * S * C >= R
    assert C - unit < c.chunk or G * S * (C - unit) < R
    if kind == "fit":
        assert lay["K1"] == -1 and (G - 1) * S < lay["walkers"] <= G * S
    else:
        assert (lay["Cs"], lay["K1"], lay["div"], lay["g"]) == (C // div, (G - min(g, G)) * (S // WAVES) // 8, div, g)
        assert lay["walkers"] > nw0  # more, shorter walkers


def test_under_one_generation_of_the_device_the_default_is_uniform(cases):
    """without VCFXG_WALK_RESIDENT the resident walkers are the device's (thousands): 100 walkers are under
    one generation, so the default and `fit` both come to the uniform layout"""
    c = cases("a")
    for layout in ("default", "fit"):
        got = c.run(layout, resident=False)
        assert got["text"] == c.uniform["text"]
        lay = got["layout"]
        assert (lay["kind"], lay["C"], lay["K1"], lay["walkers"]) == ("uniform", c.chunk, -1, c.uniform["layout"]["walkers"])
        if layout == "fit":
            assert lay["resident"] >= 1024 and lay["resident"] % WAVES == 0  # (the occupancy query's answer)


def test_some_short_walkers_own_no_line(cases):
    """b's tapers: chunks of 8 and 16 KiB under its 10 KB records (nothing to check but that they ran:
    the parity above is the test); b4: 100 walkers for 40 lines"""
    c = cases("b4")
    assert c.uniform["layout"]["walkers"] > 2 * 40
    b = cases("b")
    lay = b.run("taper:4:2")["layout"]
    assert lay["Cs"] < 10016 and lay["walkers"] > 40
