"""GPU parity of VCFX_fasta_converter, byte for byte: every golden case of the compiled reference
(tests/golden/fasta_converter_cases.json.gz) through the in-process drop-in and the executable;
generated inputs in both modes against the plain-Python restatement (tests/_fasta_converter_ref.py,
itself held to the goldens by tests/test_fasta_converter_ref.py) through the tool and through the
raw ABI (statuses, column numbers, general_records, every sample's row of the text): sample counts
around the wave width and the transpose tile's height, column counts around the FASTA line and the
tile's width, blocks that end in the middle of a FASTA line, records longer than a sweep step,
FORMATs with GT first, alone and late, alleles past the scan's table, ragged, empty and '#' lines,
repeated "#CHROM" lines, CRLF, BGZF input, VCFX_NGPU=2, a vcfx_pipe chain."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _fasta_converter_ref as R
from tests._golden import REPO
from vcfx_amd import engine, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
PIPE = os.path.join(REPO, "build", "bin", "vcfx_pipe")
CASES = R.load_cases()
MODES = ((engine.MODE_FILE, False), (engine.MODE_STDIN, True))
TS, TC = R.TILE_SAMPLES, R.TILE_COLUMNS


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def test_golden_in_process():
    bad = []
    for case in CASES:
        got = tools.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
        if got != (case["stdout"], case["stderr"], case["rc"]):
            bad.append(case["name"])
    assert not bad, bad


def test_golden_binary():
    """the executable on every golden case (a process each, sixteen at a time)"""
    assert os.access(BIN, os.X_OK)

    def one(case):
        r = subprocess.run(case["argv"], executable=BIN, input=R.case_stdin(case), capture_output=True, cwd=R.GOLDEN,
                           timeout=120)
        return (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])

    with ThreadPoolExecutor(12) as ex:  # (with this process, under the 16 that may have the device open)
        ok = list(ex.map(one, CASES))
    assert all(ok), [c["name"] for c, v in zip(CASES, ok) if not v]


def both_modes(buf, tmp_path, tag=""):
    """the drop-in in file mode and stdin mode against the restatement"""
    path = tmp_path / ("in%s.vcf" % tag)
    path.write_bytes(buf)
    for argv, stdin in (([TOOL, "-i", str(path)], b""), ([TOOL], buf)):
        got, want = tools.run(argv, stdin), R.run(argv, stdin)
        assert got[2] == want[2] and got[1] == want[1], (argv[1:2], tag)
        assert got[0] == want[0], (argv[1:2], tag, len(got[0]), len(want[0]))


def check_engine(e, buf, block=65536, want_general=None):
    """the raw ABI in both modes as the drop-in drives it: the statuses and column numbers of every
    block, the runs between "#CHROM" lines, then every block's bases transposed into the text;
    every sample's row and the general_records against the restatement.  Returns the fasta calls of
    the stdin mode."""
    calls = 0
    for mode, stdin in MODES:
        start, names, seen, per = R.device_view(buf, stdin)
        assert start is not None and per
        if stdin and not seen:
            continue
        lines = R.raw_lines(buf[start:])
        e.load(buf)
        n = e.index(start)
        assert n == len(per)
        ns, total, run_start, runs, skipped = len(names), 0, 0, [], [0] * len(names)
        l = 0
        while l < n:
            s, st, col = e.fasta_scan(l, n, ns, mode)
            k = int(s.n_lines)
            assert k == min(block, n - l)
            want = [R.line_status(ln, stdin, ns) for ln in lines[l:l + k]]
            assert st.tolist() == want, (stdin, l)
            flags = [w == R.COLUMN for w in want]
            assert col.tolist() == [sum(flags[:j]) for j in range(k)], (stdin, l)
            assert s.rows == sum(flags) and s.warn_lines == want.count(R.CHROM)
            step = k
            for j, w in enumerate(want):
                total += w == R.COLUMN
                if w == R.CHROM:
                    more = len(R.header_names(lines[l + j]))
                    if stdin:
                        runs.append((run_start, l + j, ns))
                        run_start, step = l + j + 1, j + 1
                    skipped += [total if stdin else 0] * more
                    ns += more
                    if stdin:
                        break
            l += step
        runs = runs + [(run_start, n, ns)] if stdin else [(0, n, ns)]
        q = R.sequences(buf, stdin)
        if q is None:
            assert not ns or not total or skipped[0] >= total
            continue
        assert [len(x) for x in q[1]] == [total - sk for sk in skipped] and len(q[0]) == ns
        rows = [R.wrap(x) for x in q[1]]
        row_off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
        e.fasta_begin(int(row_off[-1]))
        first, general = 0, 0
        for l0, l1, rns in runs:
            l = l0
            while l < l1:
                skip = skipped[:rns] if any(skipped[:rns]) else None
                s = e.fasta(l, l1, rns, first, total, row_off[:max(rns, 1)], skip, mode)
                assert int(s.n_lines) == min(block, l1 - l) and s.text_bytes == int(row_off[-1])
                first += int(s.rows)
                general += int(s.general_records)
                l += int(s.n_lines)
                calls += stdin
        assert first == total
        text = e.text_range(0, int(row_off[-1]))
        for k, r in enumerate(rows):
            got = text[int(row_off[k]):int(row_off[k + 1])]
            assert got == r, (stdin, k, got[:130], r[:130])
        assert general == q[2], (stdin, general, q[2])
        if want_general is not None:
            assert general == want_general, (stdin, general)
    return calls


def check(e, buf, tmp_path, tag="", **kw):
    check_engine(e, buf, **kw)
    both_modes(buf, tmp_path, tag)


def test_golden_fixtures_through_the_abi(eng):
    d = os.path.join(R.GOLDEN, "fasta_converter")
    seen = 0
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            buf = f.read()
        if R.device_view(buf, True)[0] is not None and R.device_view(buf, False)[0] is not None:
            check_engine(eng, buf)
            seen += 1
    assert seen >= 25


@pytest.mark.parametrize("ns", (1, 63, 64, 65, 2 * TS + 1))
def test_sample_counts_around_the_tile_height(eng, tmp_path, ns):
    """one below, at and above the wave width = the tile's height, and three sample tiles; GT-only
    fixed-stride records leave the fast path for no line, the malformed ones for the counted lines"""
    check(eng, R.gen_vcf(200 + ns, 70, ns, clean=True), tmp_path, "c%d" % ns, want_general=0)
    check(eng, R.gen_vcf(300 + ns, 25, ns, fmt=b"GT:AD:DP", odd=0.2), tmp_path, "o%d" % ns)


@pytest.mark.parametrize("cols", (1, 59, 60, 61, 119, 120, 121, TC - 1, TC, TC + 1))
def test_column_counts_around_the_line_and_the_tile_width(eng, tmp_path, cols):
    buf = R.gen_vcf(400 + cols, cols, 3, clean=True)
    assert R.sequences(buf, False)[1][0].__len__() == cols
    check(eng, buf, tmp_path, str(cols), want_general=0)


@pytest.mark.parametrize("block", (1, 7))
def test_blocks_that_end_inside_a_fasta_line(monkeypatch, tmp_path, block):
    """calls of one line and of seven: every block but the first starts off a multiple of 60 (the
    byte path of the transpose), blocks hold '#' and empty lines only, and a second "#CHROM" line
    cuts a block; the executable with the same setting"""
    monkeypatch.setenv("VCFXG_FA_BLOCK", str(block))
    e = engine.Engine(0)
    try:
        buf = R.gen_vcf(500 + block, 130, 5, fmt=b"GT:DP", odd=0.2, mix=True, second_header=(70, [b"X1", b"X2"]))
        n = len(R.device_view(buf, True)[3])
        assert check_engine(e, buf, block=block) >= (n - 1) // block  # (the "#CHROM" line is in no run)
        check_engine(e, R.gen_vcf(510 + block, 125, 66, clean=True), block=block, want_general=0)
    finally:
        e.close()
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    env = {"VCFXG_FA_BLOCK": str(block)}
    assert _run_bin([TOOL, "-i", str(path)], env=env) == R.run([TOOL, "-i", str(path)])
    assert _run_bin([TOOL], buf, env=env) == R.run([TOOL], buf)


def test_records_longer_than_a_sweep_step(eng, tmp_path):
    """1,100 samples: 4.4 KB of fixed-stride samples (more than the fast path's batch of 4 KiB), and
    GT:AD:DP records of 11 KB on the general path"""
    buf = R.gen_vcf(600, 9, 1100, clean=True)
    assert max(len(ln) for ln in buf.split(b"\n")) > 4400
    check(eng, buf, tmp_path, "a", want_general=0)
    check(eng, R.gen_vcf(601, 5, 1100, fmt=b"GT:AD:DP", odd=0.05), tmp_path, "b")


def test_a_sample_field_over_a_kibibyte(eng, tmp_path):
    body = []
    for i, big in enumerate((b"0/1:" + b"9," * 700 + b"9", b"7" * 1500 + b":1/1", b"x" * 1100, b"1|0:" + b"z" * 3000)):
        samples = [b"0/0:1", big, b"1/1:2", big, b"0/1:3"]
        body.append(b"\t".join([b"1", b"%d" % i, b".", b"A", b"G", b".", b".", b".", b"GT:XX" if i != 1 else b"XX:GT"] + samples))
    buf = b"##x\n" + R.chrom_line([b"S%d" % i for i in range(5)]) + b"\n" + b"\n".join(body) + b"\n"
    assert R.sequences(buf, False)[1][1] == b"RGNR"
    check(eng, buf, tmp_path)


@pytest.mark.parametrize("fmt", (b"GT", b"GT:AD:DP", b"DP:GT"))
def test_formats(eng, tmp_path, fmt):
    check(eng, R.gen_vcf(700 + len(fmt), 65, 9, fmt=fmt, odd=0.25, mix=True), tmp_path)


def test_seventeen_alt_alleles(eng, tmp_path):
    """alleles 15, 16 and 17 straddle the scan's table of 16: the later ones walk the ALT text"""
    alt = b",".join([b"C", b"G", b"T", b"A"] * 4 + [b"G"])
    gts = [b"%d/%d" % (a, b) for a in (0, 1, 15, 16, 17, 18) for b in (0, 15, 16, 17)] + [b"16|16", b"17|17", b"18/18", b"16/16:9"]
    body = [b"\t".join([b"1", b"%d" % i, b".", b"A", alt + extra, b".", b".", b".", fmt] + gts)
            for i, (fmt, extra) in enumerate(((b"GT", b""), (b"GT:DP", b""), (b"GT", b",AT,c"), (b"GT", b",")))]
    buf = b"##x\n" + R.chrom_line([b"S%d" % i for i in range(len(gts))]) + b"\n" + b"\n".join(body) + b"\n"
    seqs = R.sequences(buf, False)[1]
    assert seqs[gts.index(b"16/16")][:1] == b"A" and seqs[gts.index(b"17/17")] == b"GGGG" and \
        seqs[gts.index(b"18/18")] == b"NNNN" and seqs[gts.index(b"0/16")][:1] == b"A"
    check(eng, buf, tmp_path)


def test_ragged_empty_and_hash_lines(eng, tmp_path):
    """file mode writes a NUL for every sample a line lacks (short, empty and nine-field lines are
    columns); stdin mode skips those lines"""
    buf = R.gen_vcf(800, 150, 6, fmt=b"GT:DP", odd=0.3, mix=True)
    f, s = R.sequences(buf, False), R.sequences(buf, True)
    assert b"\0" in f[1][5] and b"\0" not in b"".join(s[1]) and len(f[1][0]) > len(s[1][0]) + 10
    assert f[2] > 20 and s[2] > 20
    check(eng, buf, tmp_path)
    check(eng, R.gen_vcf(801, 100, 4, clean=True, extra=2), tmp_path, "extra", want_general=0)


def test_two_chrom_lines(eng, tmp_path):
    buf = R.gen_vcf(900, 150, 3, odd=0.1, mix=True, second_header=(61, [b"L1", b"L2", b"L3"]))
    f, s = R.sequences(buf, False), R.sequences(buf, True)
    assert len(f[0]) == len(s[0]) == 6 and len(s[1][0]) > len(s[1][3]) > 60 and len(f[1][0]) == len(f[1][5])
    check(eng, buf, tmp_path)
    third = buf + R.chrom_line([b"Z"]) + b"\n" + R.gen_record(__import__("random").Random(1), 1, 7, 1)
    check(eng, third, tmp_path, "third")


@pytest.mark.parametrize("final", (True, False))
def test_crlf(eng, tmp_path, final):
    buf = R.gen_vcf(950 + final, 70, 4, odd=0.2, mix=True, crlf=True, final_newline=final)
    assert R.run([TOOL], buf)[0].count(b"\r") == 1  # (the last name's)
    check(eng, buf, tmp_path)
    check(eng, R.gen_vcf(960 + final, 70, 4, clean=True, crlf=True, final_newline=final), tmp_path, "clean")


def _run_bin(argv, stdin=b"", env=None):
    r = subprocess.run(argv, executable=BIN, input=stdin, capture_output=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    return r.stdout, r.stderr, r.returncode


def test_bgzf_input_gives_the_plain_output(tmp_path):
    from tests import _bgzf
    buf = R.gen_vcf(41, 200, 20, odd=0.1, mix=True, second_header=(150, [b"Q"]))
    plain, comp = tmp_path / "in.vcf", tmp_path / "in.vcf.gz"
    plain.write_bytes(buf)
    comp.write_bytes(_bgzf.bgzf(buf))
    want = R.run([TOOL, "-i", str(plain)])
    assert want[0].count(b"\n") > 80
    assert tools.run([TOOL, "-i", str(plain)]) == want
    assert tools.run([TOOL, "-i", str(comp)]) == want
    # inflated on the device (the host then fetches the "#CHROM" lines from there)
    assert _run_bin([TOOL, str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1"}) == want
    # ... and the text through a read-back window that moves many times
    assert _run_bin([TOOL, str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1", "VCFX_WINDOW_BYTES": "4096"}) == want


def test_ngpu_gives_the_unsharded_bytes(tmp_path):
    buf = R.gen_vcf(42, 100, 10, odd=0.1, mix=True)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    argv = [TOOL, "-i", str(path)]
    assert tools.shard_plan(argv, 2)[0] == 1
    want = R.run(argv)
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": "2"}) == want


def test_pipe_chain_ending_in_the_tool():
    """vcfx_pipe 'VCFX_nonref_filter | VCFX_fasta_converter' against the converter on the filter's
    own output"""
    lines = R.gen_vcf(43, 120, 10, clean=True).split(b"\n")
    homref = b"\t".join(lines[2].split(b"\t")[:9] + [b"0/0"] * 10)
    buf = b"\n".join(lines[:2] + [x for ln in lines[2:-1] for x in (ln, homref)]) + b"\n"
    kept = tools.run(["VCFX_nonref_filter"], buf)
    assert kept[2] == 0 and 20 < kept[0].count(b"\n") < buf.count(b"\n")
    want = R.run([TOOL], kept[0])
    assert want[0].startswith(b">S0\n")
    r = subprocess.run([PIPE, "VCFX_nonref_filter | %s" % TOOL], input=buf, capture_output=True, timeout=120)
    assert (r.stdout, r.returncode) == (want[0], 0)


def test_calls_out_of_order(eng):
    eng.load(b"#CHROM\tP\tI\tR\tA\tQ\tF\tI\tF\tS\n1\t5\t.\tA\tC\t.\t.\t.\tGT\t0/1\n")
    n = eng.index(0)
    st = np.zeros(2, np.uint8)
    assert eng.L.vcfxg_fasta_status(eng.h, 0, 2, st.ctypes.data, None) == -5  # VCFXG_E_STATE: no scan on this index
    s, st, col = eng.fasta_scan(0, n, 1)
    assert st.tolist() == [R.CHROM, R.COLUMN] and col.tolist() == [0, 0] and (s.rows, s.warn_lines) == (1, 1)
    off = np.zeros(1, np.uint64)
    p = engine.FaParams(engine.MODE_FILE, 1, 0, 1, off.ctypes.data, None)
    import ctypes
    eng.fasta_begin(1)
    assert eng.L.vcfxg_fasta(eng.h, 0, n, ctypes.byref(p), None) == -3  # VCFXG_E_ARG: the row does not fit the text
    eng.fasta_begin(2)
    assert eng.fasta(0, n, 1, 0, 1, off).rows == 1 and eng.text_range(0, 2) == b"M\n"
