"""GPU parity of VCFX_field_extractor, byte for byte in both modes: every golden case of the compiled
reference (tests/golden/field_extractor_cases.json.gz) through the in-process drop-in and the
executable; the device's cell matrix, statuses, row numbers and row offsets through the raw ABI against
the plain-Python restatement (tests/_field_extractor_ref.py, itself held to the goldens by
tests/test_field_extractor_ref.py): the edges of the sweep's 16 B blocks and 1 KiB steps, fields that
span three steps, the early stop, the first, the last and one past the last column of wide records,
field lists on both sides of the LDS table size, row counts around the kernels' tiles, rows shorter
than a flushed piece and longer than the LDS stage, generated line mixes, BGZF input, VCFX_NGPU=2 and
a vcfx_pipe chain."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _field_extractor_ref as R
from tests._golden import REPO
from vcfx_amd import engine, synth, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
PIPE = os.path.join(REPO, "build", "bin", "vcfx_pipe")
CASES = R.load_cases()
MODES = ((engine.MODE_FILE, False), (engine.MODE_STDIN, True))
CHROM_LINE = R.HDR.split(b"\n")[1] + b"\n"
RICH = "CHROM,POS,ID,FILTER,INFO,DP,AF,DB,NA1:GT,NA2:DP,S3:GT,S5:DP,S6:GT,dup:DP,NA1:GT"


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
    """the executable on every golden case (a process each, twelve at a time; argv[0] is the tool's
    name, as recorded, so that getopt's messages match)"""
    assert os.access(BIN, os.X_OK)

    def one(case):
        r = subprocess.run(case["argv"], executable=BIN, input=R.case_stdin(case), capture_output=True, cwd=R.GOLDEN,
                           timeout=120)
        return (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])

    with ThreadPoolExecutor(12) as ex:
        ok = list(ex.map(one, CASES))
    assert all(ok), [c["name"] for c, v in zip(CASES, ok) if not v]


def check_engine(eng, buf, fields, table_global=None):
    """statuses, row numbers, row offsets, the matrix entry for entry and the text of the raw ABI in both
    modes; returns the text per mode"""
    fields = fields.split(",") if isinstance(fields, str) else fields
    texts = []
    eng.load(buf)
    for mode, stdin in MODES:
        names, names_from = R.names_of(buf, stdin)
        cols, pool = R.table(fields, names, stdin)
        assert eng.index(0) == len(R.line_spans(buf))
        eng.fields_load(cols, pool, mode)
        s, st, row, off, cells = eng.fields_scan(names_from)
        want_st = R.statuses(buf, fields, stdin)
        want = R.cells(buf, fields, stdin)
        text = R.rows(buf, fields, stdin)
        assert st.tolist() == want_st, stdin
        got = cells.tolist()
        exp = [[list(c) for c in r] for r in want]
        assert got == exp, (stdin, [(i, j, g, w) for i, (a, b) in enumerate(zip(got, exp)) for j, (g, w) in enumerate(zip(a, b))
                                    if g != w][:8])
        assert (s.n_lines, s.rows, s.text_bytes) == (len(want_st), len(want), len(text))
        is_row = np.array([x == R.ROW for x in want_st], np.uint64)
        assert row.tolist() == (np.cumsum(is_row) - is_row).tolist()
        lens = [sum(1 if c[1] >= R.ONE else c[1] for c in r) + len(r) for r in want]
        it, acc, offs = iter(lens), 0, []
        for x in want_st:
            offs.append(acc)
            if x == R.ROW:
                acc += next(it)
        assert off.tolist() == offs
        if table_global is not None:
            assert s.general_records == int(table_global)
        got_text = eng.fields_text()
        assert got_text == text, (stdin, len(got_text), len(text))
        texts.append(text)
    return texts


def both_modes(buf, fields, tmp_path, tag=""):
    """the drop-in in file mode and stdin mode against the restatement"""
    path = tmp_path / ("in%s.vcf" % tag)
    path.write_bytes(buf)
    for argv, stdin in (([TOOL, "-f", fields, "-i", str(path)], b""), ([TOOL, "-f", fields], buf)):
        got, want = tools.run(argv, stdin), R.run(argv, stdin)
        assert got[2] == want[2] and got[1] == want[1], (argv[3:], tag)
        assert got[0] == want[0], (argv[3:], tag, len(got[0]), len(want[0]))


def test_golden_fixtures_per_line(eng):
    """every fixture through the raw ABI with the mixed field list"""
    d = os.path.join(R.GOLDEN, "field_extractor")
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            buf = f.read()
        if buf:
            check_engine(eng, buf, R.GEN_FIELDS, table_global=False)


# ---- the edges of the sweep ----------------------------------------------------------------------

def rec(info=b"DP=8;AF=2", fmt=b"GT:DP", samples=(b"0/1:3", b"1|1:4", b"0|0:5", b"./.:6", b"1/1:7"), id_=b"id"):
    return b"\t".join((b"1", b"5", id_, b"A", b"C", b"9", b"PASS", info, fmt) + tuple(samples))


def edge_line(feature, at):
    """a record with a short head whose `feature` byte stands at line offset `at`: the bytes before it in
    its own field are padded"""
    smp = (b"x:3", b"y:4", b"z:5", b"u:6", b"v:7")

    def build(pad):
        p = b"p" * pad
        if feature == "tab":          # the tab that ends POS
            line = b"\t".join((b"1", b"5" + p, b"id", b"", b"", b"", b"", b"DP=8;AF=2", b"G:D") + smp)
            return line, [i for i, c in enumerate(line) if c == 9][1]
        if feature in ("key", "eq"):  # the first byte of the key DP, its '='
            line = b"\t".join((b"1", b"5", b"", b"", b"", b"", b"", b"Q=" + p + b";DP=8;AF=2", b"G:D") + smp)
            return line, line.index(b";DP=8") + (1 if feature == "key" else 3)
        if feature == "colon":        # the ':' of FORMAT before D
            line = b"\t".join((b"1", b"5", b"", b"", b"", b"", b"", b".", b"G" + p + b":D") + smp)
            return line, line.index(b":D")
        line = b"\t".join((b"1", b"5", b"", b"", b"", b"", b"", b"", b"G:D", b"x" + p + b":3") + smp[1:])  # a token's end
        return line, line.index(b":3")
    line, k = build(0)
    assert k <= at, (feature, at, k)
    line, k = build(at - k)
    assert k == at, (feature, at, k)
    return line


@pytest.mark.parametrize("feature", ["tab", "key", "eq", "colon", "token"])
def test_block_and_step_edges(eng, feature):
    """a needed tab, a key's first byte, its '=', a FORMAT ':' and a sample token's end at line offsets
    15 / 16 / 17 and 1023 / 1024 / 1025, the line in the middle of a 3-line file whose neighbours hold
    other values for the same names, at three start alignments"""
    fields = "CHROM,POS,ID,INFO,DP,AF,Q,NA1:G,NA1:D,NA2:G,NA2:D,S1:D,S3:G,S5:D"
    for at in (15, 16, 17, 1023, 1024, 1025):
        for shift in (0, 5, 11):
            before = rec(info=b"DP=111;AF=7;Q=before", fmt=b"G:D", samples=(b"9/9:91", b"8/8:81", b"7/7:71", b"6/6:61", b"5/5:51"))
            after = rec(info=b"AF=after;DP=222", fmt=b"D:G", samples=(b"4/4:41", b"3/3:31", b"2/2:21", b"1/1:11", b"0/0:01"))
            buf = CHROM_LINE + before + b"x" * shift + b"\n" + edge_line(feature, at) + b"\n" + after + b"\n"
            check_engine(eng, buf, fields)


def test_every_start_alignment(eng):
    for shift in range(16):
        buf = CHROM_LINE + b"#" + b"x" * shift + b"\n" + rec() + b"\n" + rec(info=b"DB;AF=1") + b"\r\n" + rec(fmt=b"DP:GT")
        check_engine(eng, buf, RICH)


def test_fields_that_span_three_steps(eng, tmp_path):
    """an INFO and a FORMAT of more than 2 KiB each; a key only in the last pair of a 3 KiB INFO; the
    first and the last match of a key in different steps (file mode takes the minimum, stdin mode the
    maximum, both carried across the steps)"""
    filler = b";".join(b"K%d=%d" % (i, i) for i in range(330))
    assert 2100 < len(filler) < 3200
    long_fmt = b":".join(b"F%d" % i for i in range(500)) + b":GT:DP"
    long_smp = b":".join(b"%d" % i for i in range(500)) + b":0|1:77"
    assert len(long_fmt) > 2100
    lines = [rec(info=filler + b";LAST=z"),
             rec(info=b"AF=first;" + filler + b";AF=mid;" + filler + b";AF=last"),
             rec(info=b"AF=first;" + filler + b";DP=5;DB", fmt=long_fmt, samples=(long_smp,) * 5),
             rec(info=filler, fmt=long_fmt + b":LAST", samples=(long_smp + b":end",) * 5),
             rec(info=b"K0=" + b"v" * 3000 + b";AF=after_a_long_value;K7"),
             rec(info=b"K" * 3000 + b"=long_key;AF=after_a_long_key")]
    buf = CHROM_LINE + b"\n".join(lines) + b"\n"
    fields = "LAST,AF,DP,DB,K0,K7,K329,K33,NA1:GT,S5:DP,NA2:F499,S3:LAST,NA1:F0," + "K" * 3000
    texts = check_engine(eng, buf, fields)
    assert b"first" in texts[0] and b"\tlast\t" in texts[1] and texts[0] != texts[1]
    both_modes(buf, fields, tmp_path)


def test_early_stop_ignores_the_bytes_behind_the_last_field(eng):
    """tabs, ';', ':' and a look-alike key behind the last needed field do not change the row"""
    head = b"1\t5\tid\tA\tC\t9\tPASS\tDP=8;AF=2"
    tails = [b"", b"\tDP=99;AF=77:DP", b"\tGT:DP\tDP=1;AF=2\t;;::\t\t\tAF=9;DP=9" + b"\tDP=3:AF=4" * 300]
    for fields in ("CHROM,POS,DP,AF", "CHROM,FILTER", "INFO,DP"):
        rows = []
        for tail in tails:
            buf = CHROM_LINE + head + tail + b"\n" + head + tail + b"\n"
            rows.append(check_engine(eng, buf, fields))
        assert rows[0] == rows[1] == rows[2]


# ---- columns -------------------------------------------------------------------------------------

def test_first_last_and_one_past_the_last_column_of_wide_records(eng, tmp_path):
    buf = synth.generate(5, 2504, 11)
    names, _ = R.names_of(buf, False)
    assert len(names) == 2504
    by_col = {v: k for k, v in names.items()}
    first, last = by_col[9].decode(), by_col[2512].decode()
    fields = "CHROM,S1:GT,S2504:GT,S2505:GT,%s:GT,%s:GT,POS,S1252:GT,S2503:GT,nobody:GT" % (first, last)
    texts = check_engine(eng, buf, fields, table_global=False)
    assert all(r.split(b"\t")[3] == b"." and r.split(b"\t")[2] not in (b".", b"") for r in texts[0].split(b"\n")[:-1])
    both_modes(buf, fields, tmp_path)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1500])
def test_field_list_lengths(eng, n, tmp_path):
    """lists on both sides of the wave's 64 columns and of the LDS table size (the table of 1,500 fields
    is read from global memory: the summary says which)"""
    pool = ["CHROM", "DP", "NA1:GT", "S%d:DP", "AF", "dup:GT", "POS", "S%d:GT", "DB", "INFO"]
    fields = [pool[i % len(pool)] for i in range(n)]
    fields = [f % (1 + i % 7) if "%d" in f else f for i, f in enumerate(fields)]
    buf = R.gen_vcf(21, 40)
    check_engine(eng, buf, fields, table_global=n == 1500)
    both_modes(buf, ",".join(fields), tmp_path)


# ---- rows ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, R.TILE_ROWS - 1, R.TILE_ROWS, R.TILE_ROWS + 1, 4 * R.TILE_ROWS + 3])
def test_row_counts_at_the_tile_edges(eng, n, tmp_path):
    """n rows (the cell kernel takes 4 lines a block, the writer VCFXG_FX_TILE_ROWS)"""
    buf = R.gen_vcf(30 + n, n + 2, mix=False)
    assert R.statuses(buf, ["CHROM"], False).count(R.ROW) == n
    check_engine(eng, buf, RICH)
    both_modes(buf, RICH, tmp_path)


def test_all_lines_empty_and_all_lines_headers(eng, tmp_path):
    for buf in (b"\n" * 200, b"\r\n" * 70, b"##a\n" * 200, CHROM_LINE * 3, b"\n##x\n\n#y"):
        check_engine(eng, buf, RICH)
        both_modes(buf, RICH, tmp_path)


def test_short_rows_share_a_flushed_piece(eng):
    """rows of 2 to 5 bytes: eight and more of them in one 16 B piece"""
    buf = CHROM_LINE + b"".join(b"%d\t%d\n" % (i % 10, i) for i in range(1000))
    texts = check_engine(eng, buf, "CHROM")
    assert len(texts[0]) == 2000
    check_engine(eng, buf, "CHROM,POS")
    check_engine(eng, buf, "ID")


def test_a_row_longer_than_the_stage(eng, tmp_path):
    """one row of about 3.5 stages between short ones; its cells cross the windows"""
    info = b";".join(b"K%d=%d" % (i, i) for i in range(1000))
    assert len(info) > R.STAGE
    lines = [rec(), rec(), rec(info=info), rec(), rec(info=info + b";DP=1"), rec()]
    buf = CHROM_LINE + b"\n".join(lines)
    texts = check_engine(eng, buf, "CHROM,INFO,DP,INFO,NA1:GT,INFO,K999")
    assert max(len(r) for r in texts[0].split(b"\n")) > 3 * R.STAGE
    both_modes(buf, "INFO,INFO,K5", tmp_path)


@pytest.mark.parametrize("name", ["g300", "g300_crlf", "g300_no_final_newline", "g300_crlf_no_final_newline"])
def test_generated_line_mixes(eng, name, tmp_path):
    """300 lines from a fixed seed: every line kind, with CRLF or not, with a final newline or not"""
    buf = R.generated(name)
    st = R.statuses(buf, ["CHROM"], True)
    assert len(st) == 300 and min(st.count(k) for k in (R.EMPTY, R.HEADER, R.ROW)) >= (5 if "crlf" not in name else 0)
    nf = [r.count(b"\t") + 1 for r in buf.replace(b"\r", b"").split(b"\n") if r and r[:1] != b"#"]
    assert {1, 2, 8, 9, 10} <= set(nf)
    check_engine(eng, buf, R.GEN_FIELDS)
    both_modes(buf, R.GEN_FIELDS, tmp_path, name)


def test_names_hold_only_after_the_chrom_line(eng, tmp_path):
    buf = rec() + b"\n" + rec(info=b"NA1:GT=zz") + b"\n" + CHROM_LINE + rec() + b"\n" + \
        b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA2\tNA1\n" + rec() + b"\n"
    texts = check_engine(eng, buf, "NA1:GT,S1:GT,NA2:DP")
    assert texts[0] == b".\t0/1\t.\n.\t0/1\t.\n0/1\t0/1\t4\n0/1\t0/1\t4\n"
    assert texts[1] == b".\t0/1\t.\nzz\t0/1\t.\n0/1\t0/1\t4\n0/1\t0/1\t4\n"
    both_modes(buf, "NA1:GT,S1:GT,NA2:DP", tmp_path)


# ---- the routes ----------------------------------------------------------------------------------

def _run_bin(argv, stdin=b"", env=None):
    r = subprocess.run(argv, executable=BIN, input=stdin, capture_output=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    return r.stdout, r.stderr, r.returncode


def test_bgzf_input_gives_the_plain_output(tmp_path):
    from tests import _bgzf
    buf = R.generated("routes")
    plain, comp = tmp_path / "in.vcf", tmp_path / "in.vcf.gz"
    plain.write_bytes(buf)
    comp.write_bytes(_bgzf.bgzf(buf))
    argv = [TOOL, "-f", R.GEN_FIELDS, "-i", str(plain)]
    want = R.run(argv)
    assert want[0].count(b"\n") > 1000
    assert tools.run(argv) == want
    argv[-1] = str(comp)
    assert tools.run(argv) == want
    # inflated on the device (the host then fetches the "#CHROM" line from there)
    assert _run_bin(argv, env={"VCFX_BGZF_DEVICE_MIN": "1"}) == want
    # ... the rows through a read-back window that moves many times
    assert _run_bin(argv, env={"VCFX_BGZF_DEVICE_MIN": "1", "VCFX_WINDOW_BYTES": "1024"}) == want


def test_ngpu_gives_the_unsharded_bytes(tmp_path):
    buf = R.generated("routes")
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    argv = [TOOL, "-f", R.GEN_FIELDS, "-i", str(path)]
    assert tools.shard_plan(argv, 2)[0] == 1
    want = R.run(argv)
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": "2"}) == want


def test_pipe_chain_ending_with_the_tool(tmp_path):
    """vcfx_pipe 'VCFX_duplicate_remover | VCFX_field_extractor -f X' against the restatement on the
    remover's output"""
    buf = R.gen_vcf(41, 400, mix=False)
    buf += b"\n".join(buf.split(b"\n")[5:60]) + b"\n"  # duplicates to remove
    kept = tools.run(["VCFX_duplicate_remover"], buf)
    assert kept[2] == 0 and 0 < kept[0].count(b"\n") < buf.count(b"\n")
    want = R.run([TOOL, "-f", R.GEN_FIELDS], kept[0])
    r = subprocess.run([PIPE, "VCFX_duplicate_remover | %s -f %s" % (TOOL, R.GEN_FIELDS)], input=buf, capture_output=True,
                       timeout=120)
    assert (r.stdout, r.returncode) == (want[0], 0)


def test_state_and_argument_errors():
    import ctypes
    e = engine.Engine(0)
    try:
        e.load(CHROM_LINE + rec() + b"\n")
        e.index(0)
        s = engine.Summary()
        st = np.zeros(4, np.uint8)
        assert e.L.vcfxg_fields_scan(e.h, 0, ctypes.byref(s)) == -5  # VCFXG_E_STATE: no table
        cols, pool = R.table(["CHROM", "DP", "NA1:GT"], R.names_of(CHROM_LINE, False)[0], False)
        e.fields_load(cols, pool, engine.MODE_FILE)
        assert e.L.vcfxg_fields_lines(e.h, 0, 2, st.ctypes.data, None, None) == -5  # no scan on this index
        assert e.L.vcfxg_fields_text(e.h, ctypes.byref(s)) == -5
        assert e.fields_scan(1)[1].tolist() == [R.HEADER, R.ROW]
        assert e.L.vcfxg_fields_lines(e.h, 1, 2, st.ctypes.data, None, None) == -3  # a range past the lines
        assert e.L.vcfxg_fields_cells(e.h, 0, 3, st.ctypes.data) == -3
        assert e.fields_text() == b"1\t8\t0/1\n"
        e.index(0)
        assert e.L.vcfxg_fields_lines(e.h, 0, 2, st.ctypes.data, None, None) == -5  # a new index: no scan on it
        e.fields_scan(1)
        e.fields_load(cols, pool, engine.MODE_STDIN)
        assert e.L.vcfxg_fields_cells(e.h, 0, 1, st.ctypes.data) == -5  # a new table: no scan with it
        # tables outside the ABI's domain
        for bad in ((R.STD, 8, 0, 0, R.NOKEY, 0, 0), (7, 0, 0, 0, R.NOKEY, 0, 0), (R.INFO, 0, 0, 2, 9, 0, 0),
                    (R.SAMPLE, 5, 0, 0, R.NOKEY, 0, 1), (R.SAMPLE, 9, 0, 0, R.NOKEY, 3, 9), (R.INFO, 0, 0, 0, R.NOKEY, 0, 0)):
            arr = (engine.FxCol * 1)(engine.FxCol(*bad, 0))
            assert e.L.vcfxg_fields_load(e.h, ctypes.cast(arr, ctypes.c_void_p), 1, b"abc", 3, 0) == -3, bad
        assert e.L.vcfxg_fields_load(e.h, ctypes.cast(arr, ctypes.c_void_p), 0, b"abc", 3, 0) == -3
        assert e.L.vcfxg_fields_load(e.h, ctypes.cast(arr, ctypes.c_void_p), 1, b"abc", 3, 7) == -3
    finally:
        e.close()
