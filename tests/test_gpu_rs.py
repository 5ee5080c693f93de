"""GPU parity of VCFX_region_subsampler, byte for byte: every golden case of the compiled reference
(tests/golden/region_subsampler_cases.json.gz) through the in-process drop-in and the executable;
constructed and generated inputs in both modes against the plain-Python restatement
(tests/_region_subsampler_ref.py, itself held to the goldens by tests/test_region_subsampler_ref.py):
the device's merged table at the scan's tile edges, names that differ in one byte and names longer
than the head window, hash collisions forced through the raw ABI, the edges of the lane path's head
window, line counts around the kernels' tiles, line mixes, wide records, BGZF input, VCFX_NGPU=2 and
a vcfx_pipe chain."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _region_subsampler_ref as R
from tests._golden import REPO
from vcfx_amd import engine, synth, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
PIPE = os.path.join(REPO, "build", "bin", "vcfx_pipe")
CASES = R.load_cases()
W = R.WINDOW
MODES = ((engine.MODE_FILE, False), (engine.MODE_STDIN, True))
REST = b".\tA\tC\t.\tPASS\t.\tGT\t0/1"
CHROM_LINE = R.HDR.split(b"\n")[1] + b"\n"


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_in_process(case):
    out, err, rc = tools.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_golden_binary():
    """the executable on every golden case (a process each, twelve at a time; argv[0] is the
    tool's name, as recorded, so that getopt's messages match)"""
    assert os.access(BIN, os.X_OK)

    def one(case):
        r = subprocess.run(case["argv"], executable=BIN, input=R.case_stdin(case), capture_output=True, cwd=R.GOLDEN,
                           timeout=120)
        return (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])

    with ThreadPoolExecutor(12) as ex:
        ok = list(ex.map(one, CASES))
    assert all(ok), [c["name"] for c, v in zip(CASES, ok) if not v]


def both_modes(buf, bed, tmp_path, tag="", extra=()):
    """the drop-in in file mode and stdin mode against the restatement"""
    path, bpath = tmp_path / ("in%s.vcf" % tag), tmp_path / ("in%s.bed" % tag)
    path.write_bytes(buf)
    bpath.write_bytes(bed)
    for argv, stdin in (([TOOL, "-b", str(bpath), "-i", str(path)] + list(extra), b""),
                        ([TOOL, "-b", str(bpath)] + list(extra), buf)):
        got, want = tools.run(argv, stdin), R.run(argv, stdin)
        assert got[2] == want[2] and got[1] == want[1], (argv[3:4], tag)
        assert got[0] == want[0], (argv[3:4], tag, len(got[0]), len(want[0]))


def check_engine(eng, buf, table, hash_bits=0):
    """statuses, summary and counts of the raw ABI in both modes; returns the wave-path lines per mode"""
    spans = R.line_spans(buf)
    eng.load(buf)
    assert eng.index(0) == len(spans)
    eng.regions_load(*table.arrays(), hash_bits=hash_bits)
    assert eng.regions_merged() == table.rows
    waves = []
    for mode, stdin in MODES:
        wave = sum(not R.lane_path(buf[a:b], stdin) for a, b in spans)
        want = R.statuses(buf, stdin, table)
        s, st, cnt = eng.region_filter(mode)
        assert st.tolist() == want, (stdin, hash_bits, [(i, a, b) for i, (a, b) in enumerate(zip(st.tolist(), want)) if a != b][:10])
        assert cnt[:7] == tuple(want.count(k) for k in range(7))
        assert cnt[7] == s.general_records == wave
        warn = want.count(R.EARLY) + want.count(R.SHORT) + want.count(R.BADPOS)
        assert (s.n_lines, s.rows, s.warn_lines, s.data_lines) == \
            (len(want), want.count(R.IN), warn, want.count(R.IN) + want.count(R.OUT) + warn)
        waves.append(wave)
    return waves


def test_golden_fixtures_per_line(eng):
    """every VCF fixture with its BED through the raw ABI: per-line statuses, counts and summary"""
    pairs = [(c["argv"][4], c["argv"][2]) for c in CASES if c["name"].endswith("__file")]
    assert len(pairs) >= 20
    for vcf, bed in pairs:
        with open(os.path.join(R.GOLDEN, vcf), "rb") as f, open(os.path.join(R.GOLDEN, bed), "rb") as g:
            buf, table = f.read(), R.Table(g.read())
        if buf:
            assert check_engine(eng, buf, table) == [0, 0], vcf


# ---- the table -----------------------------------------------------------------------------------

def merged_of(eng, names, ivs):
    eng.regions_load(names, [x[0] for x in ivs], [x[1] for x in ivs], [x[2] for x in ivs])
    got = eng.regions_merged()
    assert got == R.merged(ivs), (len(got), len(R.merged(ivs)))
    return got


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097])
def test_merged_table_on_one_name(eng, n):
    """n shuffled intervals on one name: runs that overlap, touch and stand apart, across the scan's
    tiles"""
    rnd = random.Random(n)
    ivs, p = [], 1
    for _ in range(n):
        ln = rnd.randrange(1, 50)
        ivs.append((0, p, p + ln))
        p += rnd.choice((ln // 2, ln + 1, ln + 2, ln + 30))  # overlapping, touching, one base apart, apart
    rnd.shuffle(ivs)
    got = merged_of(eng, [b"chr1"], ivs)
    assert n < 255 or 0.1 * n < len(got) < 0.9 * n


def test_merged_table_on_300_names(eng):
    names = [b"n%d" % i for i in range(300)]
    ivs = [(i, 10 + i, 20 + i) for i in range(300)]
    random.Random(1).shuffle(ivs)
    assert len(merged_of(eng, names, ivs)) == 300


def test_first_interval_contains_all_others(eng):
    """the running maximum set by the table's first element must cross every tile; the next name
    starts below it and must not inherit it"""
    ivs = [(0, 1, 1000000)] + [(0, 10 + 7 * i, 12 + 7 * i) for i in range(4096)] + [(1, 5, 6), (1, 9, 9)]
    random.Random(2).shuffle(ivs)
    assert merged_of(eng, [b"a", b"b"], ivs) == [(0, 1, 1000000), (1, 5, 6), (1, 9, 9)]


def test_equal_starts_duplicates_and_touching_pairs(eng):
    ivs = [(0, 10, 20), (0, 10, 40), (0, 10, 15), (0, 50, 60), (0, 50, 60), (0, 50, 60), (0, 70, 80), (0, 81, 90),
           (0, 100, 110), (0, 112, 120), (1, 1, 1), (1, 2, 2), (1, 4, 4), (1, 2147483000, 2147483646)]
    assert merged_of(eng, [b"x", b"y"], ivs) == [(0, 10, 40), (0, 50, 60), (0, 70, 90), (0, 100, 110), (0, 112, 120),
                                                (1, 1, 2), (1, 4, 4), (1, 2147483000, 2147483646)]


def test_a_table_of_zero_intervals(eng):
    assert merged_of(eng, [], []) == []
    buf = CHROM_LINE + R.record(b"1", b"5", REST) + b"\n\n"
    check_engine(eng, buf, R.Table(b""))
    eng.regions_load([b"1"], [], [], [])  # a name without intervals
    eng.load(buf)
    eng.index(0)
    assert eng.region_filter(engine.MODE_FILE)[1].tolist() == [R.HEADER, R.OUT, R.EMPTY]


# ---- names ---------------------------------------------------------------------------------------

def names_input():
    long70 = b"L" * 70
    names = [b"chr1", b"chr10", b"chr1\r", b"CHR1", long70, long70[:69]]
    ivs = [(0, 10, 20), (1, 30, 40), (2, 50, 60), (3, 70, 80), (4, 90, 100), (5, 110, 120)]
    lines = []
    for c in names + [b"chr", b"chr11", b"absent", long70 + b"L", long70[:68], b""]:
        for p in (15, 35, 55, 75, 95, 115):
            lines.append(R.record(c, b"%d" % p, REST))
    return R.HDR + b"\n".join(lines) + b"\n", R.Table(names=names, ivs=ivs), len(lines)


@pytest.mark.parametrize("hash_bits", [1, 2, 4, 0])
def test_names_and_forced_collisions(eng, hash_bits):
    """chr1 / chr10 / "chr1\\r" / CHR1, a 70-byte name and its 69-byte prefix (the wave path), a CHROM
    absent from the BED; the hash cut to 1, 2 and 4 bits puts the names into 2, 4 and 16 probe chains:
    the statuses do not depend on the hash"""
    buf, table, n = names_input()
    want = R.statuses(buf, False, table)
    assert want.count(R.IN) == 6 and want.count(R.SHORT) == 6 and want.count(R.OUT) == n - 12  # (an empty CHROM is short)
    waves = check_engine(eng, buf, table, hash_bits)
    assert waves[0] == 4 * 6  # CHROM of 68 bytes and more: the second tab is past the window
    vcf, bed = R.generated("collide")
    check_engine(eng, vcf, R.Table(bed), hash_bits)


# ---- the head window -----------------------------------------------------------------------------

def test_head_window_edges(eng, tmp_path):
    """the second tab (file) and the seventh tab (stdin) at byte W - 1, W and W + 1 of the line; a POS
    field that straddles W; a short line of exactly W bytes and of W + 1"""
    lines, names, ivs = [], [], []
    for at in (W - 1, W, W + 1):
        # the second tab at `at`: CHROM padded
        c = b"c" * (at - 1 - 3)
        lines.append(R.record(c, b"150", REST))
        assert lines[-1].index(b"\t", len(c) + 1) == at
        names.append(c)
        ivs.append((len(names) - 1, 100, 200))
        lines.append(R.record(c, b"250", REST))
        # the seventh tab at `at`: ID padded
        bare = b"\t".join([b"s", b"150", b"", b"A", b"C", b".", b"PASS", b".", b"GT", b"0/1"])
        k = [i for i, ch in enumerate(bare) if ch == 9][6]
        lines.append(bare.replace(b"\t\t", b"\t" + b"i" * (at - k) + b"\t"))
        assert [i for i, ch in enumerate(lines[-1]) if ch == 9][6] == at
    names.append(b"s")
    ivs.append((len(names) - 1, 100, 200))
    # POS straddles W: bytes W - 2 .. W + 2
    c = b"p" * (W - 3)
    names.append(c)
    ivs.append((len(names) - 1, 12340, 12350))
    lines += [R.record(c, b"12345", REST), R.record(c, b"12399", REST), c + b"\t12345", c + b"\t1234", c + b"\t123",
              b"q" * W, b"q" * (W + 1), b"q" * (W - 1) + b"\t", b"q" * W + b"\t", b"q" * W + b"\t5", b"\t" * W, b"\t" * (W + 1)]
    buf = R.HDR + b"\n".join(lines) + b"\n"
    table = R.Table(names=names, ivs=ivs)
    waves = check_engine(eng, buf, table)
    assert waves[0] >= 6 and waves[1] >= 8 and max(waves) <= len(lines) - 4
    bed = b"".join(b"%s\t%d\t%d\n" % (names[i], s - 1, e) for i, s, e in ivs)
    both_modes(buf, bed, tmp_path)


@pytest.mark.parametrize("name", ["n255", "n256", "n257", "n4097", "g600"])
def test_line_counts_at_the_tile_edges(eng, name, tmp_path):
    buf, bed = R.generated(name)
    assert name == "g600" or len(R.line_spans(buf)) == int(name[1:])
    check_engine(eng, buf, R.Table(bed))
    both_modes(buf, bed, tmp_path, name)


@pytest.mark.parametrize("name", ["mix", "mix_crlf", "mix_no_final_newline"])
def test_line_mixes(eng, name, tmp_path):
    """'#' and empty lines between the data lines, data before the header, a second "#CHROM" line,
    short lines and bad POS fields, with and without -q in both modes; the three warning kinds
    interleave on stderr as their lines do"""
    buf, bed = R.generated(name)
    table = R.Table(bed)
    st = R.statuses(buf, True, table)
    # (with CRLF an empty line is "\\r": a short data line)
    assert min(st.count(k) for k in (R.HEADER, R.SHORT, R.IN, R.OUT, R.BADPOS) + ((R.EMPTY,) if name != "mix_crlf" else ())) >= 5
    assert st.count(R.EARLY) >= 2
    check_engine(eng, buf, table)
    both_modes(buf, bed, tmp_path, name)
    both_modes(buf, bed, tmp_path, name, extra=("-q",))
    bpath = tmp_path / "order.bed"
    bpath.write_bytes(bed)
    out, err, rc = tools.run([TOOL, "-b", str(bpath)], buf)
    kinds = [{R.WARN_EARLY: "e", R.WARN_SHORT_STDIN: "s", R.WARN_POS: "p"}[w + b"\n"] for w in err.split(b"\n")[:-1]]
    assert "".join(kinds) == "".join({R.EARLY: "e", R.SHORT: "s", R.BADPOS: "p"}.get(s, "") for s in st)
    assert len(set(kinds)) == 3 and kinds != sorted(kinds) and kinds != sorted(kinds, reverse=True)  # not grouped by kind
    assert tools.run([TOOL, "--quiet", "-b", str(bpath)], buf) == (out, err, 0)  # -q silences nothing on stdin


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_data_lines(eng, n, tmp_path):
    bed = b"1\t0\t10\n"
    for tail in (b"\n", b""):
        for second in (R.record(b"1", b"10", REST), R.record(b"1", b"11", REST), b"1\t3"):
            buf = CHROM_LINE + R.record(b"1", b"5", REST) + (b"\n" + second if n == 2 else b"") + tail
            check_engine(eng, buf, R.Table(bed))
            both_modes(buf, bed, tmp_path)


def test_wide_records(eng, tmp_path):
    """300 lines x 2,504 samples; the BED keeps about half of them, in runs of five: the sample bytes do
    not matter and are not read"""
    buf = synth.generate(300, 2504, 11)
    k = buf.index(b"\n#CHROM") + 1
    k = buf.index(b"\n", k) + 1
    recs = buf[k:].split(b"\n")[:-1]
    assert len(recs) == 300 and min(len(r) for r in recs) > 5000
    pos = [int(r.split(b"\t", 2)[1]) for r in recs]
    chrom = recs[0].split(b"\t", 1)[0]
    bed = b"".join(b"%s\t%d\t%d\n" % (chrom, pos[i] - 1, pos[i + 4]) for i in range(0, 300, 10))
    table = R.Table(bed)
    st = R.statuses(buf, False, table)
    assert 140 <= st.count(R.IN) <= 160 and st.count(R.OUT) == 300 - st.count(R.IN)
    assert check_engine(eng, buf, table) == [0, 0]
    both_modes(buf, bed, tmp_path)


def _run_bin(argv, stdin=b"", env=None):
    r = subprocess.run(argv, executable=BIN, input=stdin, capture_output=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    return r.stdout, r.stderr, r.returncode


def test_bgzf_input_gives_the_plain_output(tmp_path):
    from tests import _bgzf
    buf, bed = R.generated("routes")
    plain, comp, bpath = tmp_path / "in.vcf", tmp_path / "in.vcf.gz", tmp_path / "in.bed"
    plain.write_bytes(buf)
    comp.write_bytes(_bgzf.bgzf(buf))
    bpath.write_bytes(bed)
    want = R.run([TOOL, "-b", str(bpath), "-i", str(plain)])
    assert want[0].count(b"\n") > 500 and want[1]
    assert tools.run([TOOL, "-b", str(bpath), "-i", str(plain)]) == want
    assert tools.run([TOOL, "-b", str(bpath), "-i", str(comp)]) == want
    # inflated on the device (the host then fetches the written lines from there)
    assert _run_bin([TOOL, "-b", str(bpath), "-i", str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1"}) == want
    # ... through a read-back window that moves many times
    assert _run_bin([TOOL, "-b", str(bpath), "-i", str(comp)],
                    env={"VCFX_BGZF_DEVICE_MIN": "1", "VCFX_WINDOW_BYTES": "1024"}) == want


def test_ngpu_gives_the_unsharded_bytes(tmp_path):
    buf, bed = R.generated("routes")
    path, bpath = tmp_path / "in.vcf", tmp_path / "in.bed"
    path.write_bytes(buf)
    bpath.write_bytes(bed)
    argv = [TOOL, "-b", str(bpath), "-i", str(path)]
    assert tools.shard_plan(argv, 2)[0] == 1
    want = R.run(argv)
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": "2"}) == want


def test_pipe_chain_starting_with_the_tool(tmp_path):
    """vcfx_pipe 'VCFX_region_subsampler -b X | VCFX_variant_counter' against the counter on the
    restatement's output"""
    buf, bed = R.generated("routes")
    bpath = tmp_path / "in.bed"
    bpath.write_bytes(bed)
    kept = R.run([TOOL, "-b", str(bpath)], buf)[0]
    want = tools.run(["VCFX_variant_counter"], kept)
    assert want[2] == 0 and want[0]
    r = subprocess.run([PIPE, "%s -b %s | VCFX_variant_counter" % (TOOL, bpath)], input=buf, capture_output=True, timeout=120)
    assert (r.stdout, r.returncode) == (want[0], 0)


def test_state_and_argument_errors():
    e = engine.Engine(0)
    try:
        e.load(CHROM_LINE + b"1\t5\n")
        e.index(0)
        s = engine.Summary()
        st = np.zeros(4, np.uint8)
        n = engine._U64(0)
        import ctypes
        assert e.L.vcfxg_region_filter(e.h, engine.MODE_FILE, ctypes.byref(s)) == -5  # VCFXG_E_STATE: no table
        assert e.L.vcfxg_regions_merged(e.h, None, None, None, 0, ctypes.byref(n)) == -5
        e.regions_load([b"1"], [0], [1], [10])
        assert e.L.vcfxg_region_status(e.h, 0, 2, st.ctypes.data) == -5  # no filter on this index
        assert e.L.vcfxg_region_filter(e.h, 7, ctypes.byref(s)) == -3  # VCFXG_E_ARG: no such mode
        assert e.region_filter(engine.MODE_FILE)[1].tolist() == [R.HEADER, R.IN]
        assert e.L.vcfxg_region_status(e.h, 0, 2, st.ctypes.data) == 0 and st[:2].tolist() == [R.HEADER, R.IN]
        assert e.L.vcfxg_region_status(e.h, 2, 1, st.ctypes.data) == -3  # a range past the lines
        assert e.L.vcfxg_region_status(e.h, 1, 2, st.ctypes.data) == -3
        e.index(0)
        assert e.L.vcfxg_region_status(e.h, 0, 2, st.ctypes.data) == -5  # a new index: no filter on it
        e.region_filter(engine.MODE_STDIN)
        e.regions_load([b"1"], [0], [6], [10])
        assert e.L.vcfxg_region_status(e.h, 0, 2, st.ctypes.data) == -5  # a new table: no filter with it
        assert e.region_filter(engine.MODE_FILE)[1].tolist() == [R.HEADER, R.OUT]
        # intervals outside the ABI's domain
        one = np.array([0], np.uint32)
        for a, b, cid in ((0, 5, 0), (6, 5, 0), (1, 5, 1)):
            s1, en = np.array([a], np.int32), np.array([b], np.int32)
            one[0] = cid
            p = ctypes.c_uint32(0)
            off = np.array([0, 1], np.uint64)
            assert e.L.vcfxg_regions_load(e.h, b"1", off.ctypes.data, 1, one.ctypes.data, s1.ctypes.data, en.ctypes.data, 1,
                                          ctypes.byref(p)) == -3
    finally:
        e.close()
