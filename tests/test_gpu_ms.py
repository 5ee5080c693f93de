"""GPU parity of VCFX_multiallelic_splitter, byte for byte: every golden case of the compiled
reference (tests/golden/multiallelic_splitter_cases.json.gz) through the in-process drop-in and the
executable; generated inputs in both modes against the plain-Python restatement
(tests/_multiallelic_splitter_ref.py, itself held to the goldens by
tests/test_multiallelic_splitter_ref.py) through the tool and through the raw ABI (statuses, nAlts,
rows, every line's text range): sample counts around the wave width, allele counts up to 65 (a
sample field longer than a 1 KiB step), line lengths around the step and around 16 B, FORMAT key
counts and tables around the LDS caps, blocks of one line, BGZF input, VCFX_NGPU=2, a vcfx_pipe
chain."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import _multiallelic_splitter_ref as R
from tests._golden import REPO
from vcfx_amd import engine, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
PIPE = os.path.join(REPO, "build", "bin", "vcfx_pipe")
CASES = R.load_cases()
MODES = ((engine.MODE_FILE, False), (engine.MODE_STDIN, True))
K = R.KEYS_LDS


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def small_blocks(monkeypatch, lines, nbytes=None):
    """a context whose calls take at most `lines` lines and `nbytes` bytes of estimated text"""
    monkeypatch.setenv("VCFXG_MS_BLOCK", str(lines))
    if nbytes:
        monkeypatch.setenv("VCFXG_MS_BYTES", str(nbytes))
    return engine.Engine(0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_in_process(case):
    out, err, rc = tools.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_golden_binary():
    """the executable on every golden case (a process each, twelve at a time)"""
    assert os.access(BIN, os.X_OK)

    def one(case):
        r = subprocess.run(case["argv"], executable=BIN, input=R.case_stdin(case), capture_output=True, cwd=R.GOLDEN,
                           timeout=120)
        return (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])

    with ThreadPoolExecutor(12) as ex:
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


def check_engine(e, buf, table=None, want_general=None, limits=(65536, 512 << 20)):
    """the raw ABI in both modes, block by block: statuses, nAlts, the summary, every line's text
    range; table: another table than the header's (the restatement's meta follows it); limits: the
    context's lines and estimated text bytes per call, which decide the lines each call takes (a
    line counts as nAlts x (its bytes + 1), and one line is always taken).  Returns (calls,
    general_records) of the stdin mode."""
    res = None
    for mode, stdin in MODES:
        start, decls, per = R.device_view(buf, stdin)
        assert start is not None and per
        if table is not None:
            decls = table
            meta = {}
            for i, s, n in decls:
                meta[i] = (s, n)
            lines = R.raw_lines(buf[start:])
            per = []
            for ln in lines:
                f = R.fields_of(ln, stdin) if ln and ln[:1] != b"#" else []
                if len(f) >= 9 and b"," in f[4]:
                    rows = R.split_line(ln, stdin, meta)
                    per.append((R.SPLIT, len(rows), b"".join(r + b"\n" for r in rows)))
                else:
                    per.append((R.EMPTY if not ln else R.HEADER if ln[:1] == b"#" else R.COPY, 0, b""))
        e.load(buf)
        n = e.index(start)
        assert n == len(per)
        cost = [p[1] * (len(ln) + 1) for p, ln in zip(per, R.raw_lines(buf[start:]))]
        l = calls = general = 0
        while l < n:
            s, st, alt, off, text = e.multiallelic_split(l, n, R.table_entries(decls), mode)
            k = int(s.n_lines)
            fit = [j for j in range(1, min(limits[0], n - l) + 1) if sum(cost[l:l + j]) <= limits[1]]
            assert k == (fit[-1] if fit else 1), (stdin, l, k)
            blk = per[l:l + k]
            assert st.tolist() == [p[0] for p in blk], (stdin, l)
            assert alt.tolist() == [p[1] for p in blk], (stdin, l)
            assert s.rows == sum(p[1] for p in blk) and s.data_lines == sum(p[0] in (R.COPY, R.SPLIT) for p in blk)
            assert int(off[0]) == 0 and int(off[k]) == s.text_bytes == len(text)
            for i, p in enumerate(blk):
                got = text[int(off[i]):int(off[i + 1])]
                assert got == p[2], (stdin, l + i, got[:200], p[2][:200])
            general += s.general_records
            calls += 1
            l += k
        res = (calls, general)
        if want_general is not None:
            assert general == want_general[stdin], (stdin, general)
    return res


def check(e, buf, tmp_path, tag=""):
    check_engine(e, buf)
    both_modes(buf, tmp_path, tag)


def test_golden_fixtures_through_the_abi(eng):
    d = os.path.join(R.GOLDEN, "multiallelic_splitter")
    seen = 0
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            buf = f.read()
        if R.device_view(buf, True)[0] is not None and R.device_view(buf, False)[0] is not None:
            check_engine(eng, buf)
            seen += 1
    assert seen >= 15


@pytest.mark.parametrize("ns", (1, 2, 63, 64, 65, 130))
def test_sample_counts_and_allele_counts(eng, tmp_path, ns):
    """1..130 samples at nAlts 2, 3, 9, 10 and 11 (and unsplit lines), well-formed and malformed
    sub-fields; the 130-sample input has sample fields that straddle a lane's 16 B and a wave's
    1 KiB of the sweep, by the input's own offsets"""
    buf = R.gen_vcf(100 + ns, 12, ns, alts=(2, 3, 9, 10, 11, 1), keys=(b"GT", b"AD", b"DP", b"PL", b"XA"), odd=0.15)
    if ns == 130:
        lanes = steps = 0
        pos = buf.index(b"\n", buf.index(b"#CHROM")) + 1
        for ln in buf[pos:].split(b"\n")[:-1]:
            t, p = [], -1
            for _ in range(9):
                p = ln.index(b"\t", p + 1)
                t.append(p)
            a0 = (pos + t[8]) & ~15  # the sample sweep's first 16 B piece
            s = pos + t[8] + 1
            for f in ln[t[8] + 1:].split(b"\t"):
                lanes += (s - a0) // 16 != (s + len(f) - a0) // 16
                steps += (s - a0) // 1024 != (s + len(f) - a0) // 1024
                s += len(f) + 1
            pos += len(ln) + 1
        assert lanes >= 100 and steps >= 10
    check(eng, buf, tmp_path, str(ns))


def test_sixty_five_alleles_with_full_lists(eng, tmp_path):
    """nAlts above the wave width: a PL list of 2,211 values makes one sample field longer than a
    1 KiB step (and than any staging a wave could hold)"""
    buf = R.gen_vcf(65, 2, 3, alts=(65,), keys=(b"GT", b"AD", b"PL"), odd=0.0)
    fields = buf.split(b"\n")[-2].split(b"\t")
    assert fields[4].count(b",") == 64 and max(len(f) for f in fields[9:]) > 4096
    check(eng, buf, tmp_path)


def padded(length, tail=b"\tA\tC,G\t.\t.\tAF=1,2\tGT:AD\t1/2:1,2,3\t0/1:4,5,6"):
    ln = b"1\t5\t" + b"i" * (length - len(tail) - 4) + tail
    assert len(ln) == length
    return ln


def test_line_lengths_and_row_residues(eng, tmp_path):
    """lines of 1023, 1024 and 1025 bytes and around multiples of 16; by the restatement's own
    numbers the rows' offsets and lengths cover 0, 1 and 15 mod 16, and rows both shrink and grow
    against their line"""
    lens = (47, 48, 49, 63, 64, 65, 79, 80, 81, 1023, 1024, 1025, 2047, 2048, 2049)
    lines = [padded(n) for n in lens] + [padded(n, b"\tA\tC,G\t.\t.\t.\tGT\t1/2") for n in range(40, 72)]
    lines.append(b"1\t9\t.\tA\tC,G\t.\t.\t.\tGT:AD:DP:PL" + b"\t" * 50)                      # rows grow
    lines.append(b"1\t9\t.\tA\tC,G,T\t.\t.\t.\tGT:PL\t" + b"\t".join([b"1/2:0,1,2,3,4,5,6,7,8,9"] * 50))  # rows shrink
    buf = R.header(2) + b"\n".join(lines) + b"\n"
    per = R.device_view(buf, True)[2]
    offs, lens_, grow, shrink, o = set(), set(), 0, 0, 0
    for (st, n, rows), ln in zip(per, lines):
        for r in rows.split(b"\n")[:-1]:
            offs.add(o % 16)
            lens_.add((len(r) + 1) % 16)
            o += len(r) + 1
            grow += len(r) > len(ln)
            shrink += len(r) < len(ln)
    assert {0, 1, 15} <= offs and {0, 1, 15} <= lens_ and grow >= 2 and shrink >= 3
    check(eng, buf, tmp_path)


def keyed(nk, late):
    """a FORMAT of nk keys, the last one of class `late`, and samples with values for them"""
    keys = [b"GT", b"AD"] + [b"K%d" % i for i in range(2, nk - 1)] + [b"LAST"]
    assert len(keys) == nk
    sample = b":".join([b"1/2", b"1,2,3"] + [b"%d" % i for i in range(2, nk - 1)] + [b"7,8,9" if late == b"R" else b"7,8"])
    return b"\t".join([b"1", b"%d" % nk, b".", b"A", b"C,G", b".", b".", b"AF=1,2", b":".join(keys), sample, b"0/2", sample + b":x"])


def test_format_key_counts_around_the_lds_cap(eng, tmp_path):
    """K - 1, K and K + 1 FORMAT keys and 200: the keys past the cap get their class from the
    general look-up, and those lines are counted in general_records"""
    extra = [b"##FORMAT=<ID=LAST,Number=R,Type=Integer>"]
    counts = (K - 1, K, K + 1, 200, K - 1, 2 * K)
    buf = R.header(3, extra) + b"\n".join(keyed(nk, b"R") for nk in counts) + b"\n1\t1\t.\tA\tC\t.\t.\t.\tGT\t0/1\n"
    want = sum(nk > K for nk in counts)
    assert want == 3
    assert b":7,9" in R.split(buf, True) and b":7,8\t" in R.split(buf, True)
    check_engine(eng, buf, want_general={False: want, True: want})
    both_modes(buf, tmp_path)


@pytest.mark.parametrize("entries", (0, 1, 200, 900))
def test_header_tables(eng, tmp_path, entries):
    """a table of 0, 1 and 200 IDs in LDS, and one past the LDS cap (every split line then counts
    as general); the IDs the records use stand last, in the middle and first"""
    ids = [b"ID_%04d_%s" % (i, b"x" * (i % 23)) for i in range(entries)]
    rec = [b"XA", b"PL", b"AD"][:min(entries, 3)]
    for k, r in enumerate(rec):
        ids[(len(ids) - 1) * k // 2] = r
    cls = {b"XA": b"A", b"PL": b"G", b"AD": b"R"}
    hdr = [b"##FORMAT=<ID=%s,Number=%s,Type=Integer>" % (i, cls.get(i, b"AGR"[k % 3:k % 3 + 1])) for k, i in enumerate(ids)]
    hdr += [b"##INFO=<ID=%s_I,Number=A,Type=Integer>" % i for i in ids[:entries // 2]]
    body = R.gen_vcf(7, 9, 5, alts=(2, 3, 1), keys=(b"GT", b"AD", b"DP", b"PL", b"XA"), odd=0.1)
    body = body[body.index(b"#CHROM"):]
    buf = b"##fileformat=VCFv4.2\n" + b"".join(h + b"\n" for h in hdr) + body
    decls = R.device_view(buf, True)[1]
    past = R.table_bytes(decls) > R.TABLE_LDS
    assert past == (entries == 900) and len(decls) == len(hdr)
    split = sum(p[0] == R.SPLIT for p in R.device_view(buf, True)[2])
    assert split == 6
    check_engine(eng, buf, want_general={False: split * past, True: split * past})
    both_modes(buf, tmp_path)
    if entries == 200:  # the raw ABI with duplicates: the last entry of an ID wins, across the sections
        table = [(b"AD", R.FORMAT, b"R"), (b"PL", R.FORMAT, b"G"), (b"AD", R.INFO, b"G"), (b"XA", R.FORMAT, b"1"),
                 (b"XA", R.FORMAT, b"A"), (b"AF", R.INFO, b"A"), (b"AF", R.INFO, b"2"), (b"AC", R.FORMAT, b"R")]
        check_engine(eng, buf, table=table)


def test_blocks_of_one_line_and_cuts_between_lines(monkeypatch, tmp_path):
    """calls of one line, of two (a cut between a split line and a copied one), and calls cut by
    the byte budget; the executable with the same settings"""
    buf = R.gen_vcf(11, 14, 3, alts=(2, 1, 3, 1), odd=0.2, mix=True)
    per = R.device_view(buf, True)[2]
    n = len(per)
    assert any(per[i][0] == R.SPLIT and per[i + 1][0] == R.COPY for i in range(1, n - 1, 2))
    for lines, nbytes, calls in ((1, 512 << 20, n), (2, 512 << 20, (n + 1) // 2), (1 << 20, 1, None), (1 << 20, 700, None)):
        e = small_blocks(monkeypatch, lines, nbytes)
        try:
            got = check_engine(e, buf, limits=(lines, nbytes))[0]
            assert calls is None or got == calls
        finally:
            e.close()
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    for env in ({"VCFXG_MS_BLOCK": "1"}, {"VCFXG_MS_BLOCK": "3"}, {"VCFXG_MS_BYTES": "700"}):
        assert _run_bin([TOOL, "-i", str(path)], env=env) == R.run([TOOL, "-i", str(path)])
        assert _run_bin([TOOL], buf, env=env) == R.run([TOOL], buf)


def test_the_byte_budget_cuts_by_estimated_text(monkeypatch):
    """a line counts as nAlts x (its bytes + 1): three split lines of 100 bytes at two alleles fit a
    budget of 404 two at a time"""
    rec = padded(100)
    buf = R.header(2) + b"".join([rec + b"\n"] * 5)
    e = small_blocks(monkeypatch, 1 << 20, 404)
    try:
        assert check_engine(e, buf, limits=(1 << 20, 404))[0] == 3
    finally:
        e.close()


@pytest.mark.parametrize("which", ("none", "all", "last"))
def test_files_where_no_every_and_only_the_last_line_splits(eng, tmp_path, which):
    alts = {"none": (1,), "all": (2, 3), "last": (1,)}[which]
    buf = R.gen_vcf(21, 30, 4, alts=alts, odd=0.1)
    if which == "last":
        buf += R.gen_record(__import__("random").Random(1), 99, 4, 3)  # (and no final newline)
    st = [p[0] for p in R.device_view(buf, False)[2]]
    assert st.count(R.SPLIT) == {"none": 0, "all": 30, "last": 1}[which] and (which != "last" or st[-1] == R.SPLIT)
    check(eng, buf, tmp_path)


@pytest.mark.parametrize("crlf,final", ((True, True), (True, False), (False, False)))
def test_crlf_and_no_final_newline(eng, tmp_path, crlf, final):
    buf = R.gen_vcf(31 + crlf, 25, 3, odd=0.2, mix=True, crlf=crlf, final_newline=final)
    assert buf.endswith(b"\n") == final
    check(eng, buf, tmp_path)
    nine = R.header(0, eol=b"\r\n" if crlf else b"\n") + b"1\t5\t.\tA\tC,G\t.\t.\tAF=1,2\tGT" + (b"\r" if crlf else b"")
    check(eng, nine, tmp_path, "nine")


def test_lines_before_and_without_chrom(tmp_path):
    """stdin mode splits data lines that stand before a "#CHROM" line with the table read so far;
    file mode copies such an input as it is, without the device"""
    rec = b"1\t5\t.\tA\tC,G\t.\t.\tAF=1,2\tGT:AD\t1/2:1,2,3\n"
    buf = b"##INFO=<ID=AF,Number=A>\n" + rec + b"##FORMAT=<ID=AD,Number=R>\n\n#CHROM\tPOS\n" + rec + b"1\t6\t.\tA\tC"
    both_modes(buf, tmp_path)
    assert R.split(buf, True).count(b"1/.:1,2,3") == 2 and R.split(buf, False) == buf + b"\n"


def _run_bin(argv, stdin=b"", env=None):
    r = subprocess.run(argv, executable=BIN, input=stdin, capture_output=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    return r.stdout, r.stderr, r.returncode


def test_bgzf_input_gives_the_plain_output(tmp_path):
    from tests import _bgzf
    buf = R.gen_vcf(41, 200, 20, odd=0.1, mix=True)
    plain, comp = tmp_path / "in.vcf", tmp_path / "in.vcf.gz"
    plain.write_bytes(buf)
    comp.write_bytes(_bgzf.bgzf(buf))
    want = R.run([TOOL, "-i", str(plain)])
    assert want[0].count(b"\n") > 300
    assert tools.run([TOOL, "-i", str(plain)]) == want
    assert tools.run([TOOL, "-i", str(comp)]) == want
    # inflated on the device (the host then fetches the copied lines from there)
    assert _run_bin([TOOL, str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1"}) == want
    # ... through a read-back window that moves many times
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


def test_pipe_chain_starting_with_the_tool():
    """vcfx_pipe 'VCFX_multiallelic_splitter | VCFX_variant_counter' against the counter on the
    restatement's output"""
    buf = R.gen_vcf(43, 120, 10, odd=0.1)
    split = R.run([TOOL], buf)[0]
    want = tools.run(["VCFX_variant_counter"], split)
    assert want[2] == 0 and want[0] and split.count(b"\n") > buf.count(b"\n") + 100
    r = subprocess.run([PIPE, "%s | VCFX_variant_counter" % TOOL], input=buf, capture_output=True, timeout=120)
    assert (r.stdout, r.returncode) == (want[0], 0)


def test_range_call_needs_a_split(eng):
    import numpy as np
    eng.load(b"1\t5\t.\tA\tC,G\t.\t.\t.\tGT\t1/2\n")
    eng.index(0)
    off = np.zeros(2, np.uint64)
    assert eng.L.vcfxg_ms_line_ranges(eng.h, 0, 1, off.ctypes.data) == -5  # VCFXG_E_STATE: no split on this index
    s, st, alt, off, text = eng.multiallelic_split(0, 1, [], engine.MODE_FILE)
    assert (s.rows, st.tolist(), alt.tolist(), off.tolist()) == (2, [R.SPLIT], [2], [0, len(text)])
    assert text == b"1\t5\t.\tA\tC\t.\t.\t.\tGT\t1/.\n1\t5\t.\tA\tG\t.\t.\t.\tGT\t./1\n"
    assert eng.L.vcfxg_ms_line_ranges(eng.h, 1, 1, off.ctypes.data) == -3  # VCFXG_E_ARG
