"""GPU parity of VCFX_sorter: every recorded case of the compiled reference
(tests/golden/sorter_cases.json.gz) through the in-process drop-in and the executable, byte for byte
(the ties_* cases: byte for byte against the stable restatement, and against the reference's bytes
up to the order inside runs of equal keys); per-line statuses, the order and the gathered text of
the raw ABI against the plain-Python restatement (tests/_sorter_ref.py, itself held to the recorded
cases by tests/test_sorter_ref.py) in both modes and both orders: the fixtures, kept-line counts
around the kernels' and the sort's tiles, every pairing of source and destination alignment in the
gather, 70,000-byte lines, text blocks of 64 bytes and 4 KiB, sorted / reversed / all-equal inputs,
CHROM lengths that change the number of sort passes, BGZF input, VCFX_NGPU=2 and a vcfx_pipe chain."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _sorter_ref as R
from tests._golden import REPO
from vcfx_amd import engine, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
PIPE = os.path.join(REPO, "build", "bin", "vcfx_pipe")
CASES = R.load_cases()
W = R.WINDOW
COMBOS = tuple((mode, stdin, natural) for mode, stdin in ((engine.MODE_FILE, False), (engine.MODE_STDIN, True))
               for natural in (False, True))


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def expected_stdout(case):
    """what the drop-in must print: the recorded bytes, or for a ties_* case the stable order"""
    if not case["ties"]:
        return case["stdout"]
    want = R.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)[0]
    assert R.same_up_to_ties(want, case["stdout"], *R.case_mode(case))
    return want


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_in_process(case):
    out, err, rc = tools.run(case["argv"], R.case_stdin(case), cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert out == expected_stdout(case)
    assert err == case["stderr"]


def test_golden_binary():
    """the executable on every golden case (a process each, twelve at a time; argv[0] is the
    tool's name, as recorded, so that getopt's messages match)"""
    assert os.access(BIN, os.X_OK)

    def one(case):
        r = subprocess.run(case["argv"], executable=BIN, input=R.case_stdin(case), capture_output=True, cwd=R.GOLDEN,
                           timeout=120)
        return (r.returncode, r.stdout, r.stderr) == (case["rc"], expected_stdout(case), case["stderr"])

    with ThreadPoolExecutor(12) as ex:
        ok = list(ex.map(one, CASES))
    assert all(ok), [c["name"] for c, v in zip(CASES, ok) if not v]


def lane_path(line, stdin):
    """the line is settled by the key kernel's lane pass: its first tab (stdin mode: its first two)
    or its end lies inside the first W bytes"""
    if not line or line[:1] == b"#" or len(line) <= W:
        return True
    return line[:W].count(b"\t") >= (2 if stdin else 1)


def check_engine(e, buf, combos=COMBOS):
    """statuses, summary, counts, order and gathered text of the raw ABI against the restatement"""
    spans = R.line_spans(buf)
    e.load(buf)
    assert e.index(0) == len(spans)
    for mode, stdin, natural in combos:
        want, _ = R.statuses(buf, stdin, natural)
        order = R.order(buf, stdin, natural)
        s, st, cnt, got = e.sort(mode, natural)
        where = (stdin, natural)
        assert st.tolist() == want, (where, [i for i, (a, b) in enumerate(zip(st.tolist(), want)) if a != b][:10])
        assert cnt[:5] == tuple(want.count(k) for k in range(5)), where
        assert cnt[5] == s.general_records == sum(not lane_path(buf[a:b], stdin) for a, b in spans), where
        assert (s.n_lines, s.rows, s.data_lines, s.warn_lines) == \
            (len(want), len(order), want.count(R.KEPT), want.count(R.PRE) + want.count(R.BAD)), where
        assert got.tolist() == order, (where, [i for i, (a, b) in enumerate(zip(got.tolist(), order)) if a != b][:10])
        text = e.sorted_text(s.rows)
        exp = R.sort_bytes(buf, stdin, natural)[0]
        assert len(text) == len(exp), where
        assert text == exp, (where, next(i for i in range(len(exp)) if text[i] != exp[i]))


def both_modes(buf, tmp_path, tag="", extra=()):
    """the drop-in in file mode and stdin mode against the restatement"""
    path = tmp_path / ("in%s.vcf" % tag)
    path.write_bytes(buf)
    for argv, stdin in (([TOOL] + list(extra) + [str(path)], b""), ([TOOL] + list(extra), buf)):
        got, want = tools.run(argv, stdin), R.run(argv, stdin)
        assert got[2] == want[2] and got[1] == want[1], (argv[1:2], tag)
        assert got[0] == want[0], (argv[1:2], tag, len(got[0]), len(want[0]))


def test_golden_fixtures_per_line(eng):
    """every fixture through the raw ABI: per-line statuses, vcfxg_sort_order and the text"""
    d = os.path.join(R.GOLDEN, "sorter")
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            buf = f.read()
        if buf:
            check_engine(eng, buf)


@pytest.mark.parametrize("name", ["n1", "n2", "n16", "n17", "n255", "n256", "n257", "n4097"])
def test_kept_line_counts(eng, name, tmp_path):
    buf = R.generated(name)
    check_engine(eng, buf)
    both_modes(buf, tmp_path, name)
    both_modes(buf, tmp_path, name, extra=("-n",))


@pytest.mark.parametrize("name", ["mix", "mix_ties", "routes"])
def test_line_mixes(eng, name, tmp_path):
    """'#', empty and malformed lines between the data; mix_ties: most keys shared (the stable order)"""
    buf = R.generated(name)
    st = R.statuses(buf, False)[0]
    assert min(st.count(k) for k in (R.EMPTY, R.HEADER, R.BAD, R.KEPT)) >= 5
    check_engine(eng, buf)
    check_engine(eng, R.HDR.split(b"\n")[0] + b"\n" + buf[len(R.HDR):])  # no "#CHROM" line: all PRE in file mode
    both_modes(buf, tmp_path, name)
    both_modes(buf.replace(b"\n", b"\r\n"), tmp_path, name + "_crlf", extra=("-n",))
    both_modes(buf[:-1], tmp_path, name + "_no_final_newline")


def alignment_sweep():
    """Lines of 1..70 bytes, round after round in shuffled order, until every source offset mod 16
    has met every destination offset mod 16 in both modes (asserted).  A line shorter than 8 bytes
    is a '#' line, the others are data lines with keys of their own in random order."""
    rnd = random.Random(16)
    lines = [b"#CHROM"]
    pos = list(range(1, 20000))
    rnd.shuffle(pos)

    def pairs(buf, stdin):
        spans, got, o = R.line_spans(buf), set(), 0
        for i in R.order(buf, stdin):
            got.add((spans[i][0] % 16, o % 16))
            o += spans[i][1] - spans[i][0] + 1
        return got

    for _ in range(40):
        lens = list(range(1, 71))
        rnd.shuffle(lens)
        for n in lens:
            if n < 8:
                lines.append(b"#" + bytes(48 + (i * 7 + n) % 75 for i in range(n - 1)))
            else:
                head = b"%d\t%d\t" % (rnd.randrange(1, 4), pos.pop())
                lines.append(head + bytes(48 + (i * 7 + n) % 75 for i in range(n - len(head))))  # (no two runs alike)
            assert len(lines[-1]) == n
        buf = b"\n".join(lines) + b"\n"
        if len(pairs(buf, False)) == 256 and len(pairs(buf, True)) == 256:
            break
    assert len(pairs(buf, False)) == 256 and len(pairs(buf, True)) == 256
    assert {len(x) for x in lines} >= set(range(1, 71))
    return buf


def test_alignment_sweep(eng):
    """every pairing of a line's alignment in the input with its alignment in the output"""
    check_engine(eng, alignment_sweep(), COMBOS[::2])


def long_line(chrom, pos, n):
    head = R.record(chrom, pos, b"long") + b";L="
    return head + bytes(random.Random(n).choice(b"ACGT") for _ in range(n - len(head)))


def test_long_lines(eng, tmp_path):
    """one 70,000-byte line among short ones; a 70,000-byte line first and last in the output"""
    short = R.gen_vcf(70, 300, chroms=(b"2", b"3", b"chr5"))
    mid = long_line(b"3", b"500000", 70000)
    assert len(mid) == 70000
    lines = short.split(b"\n")[:-1]
    buf = b"\n".join(lines[:100] + [mid] + lines[100:]) + b"\n"
    check_engine(eng, buf)
    # "!" sorts before and "~" after every other CHROM as bytes; "1" / a hashed name by chromToId
    first, last = long_line(b"!", b"7", 70000), long_line(b"~", b"9", 70000)
    buf = b"\n".join(lines[:50] + [last] + lines[50:200] + [first] + lines[200:]) + b"\n"
    o = R.order(buf, False)
    spans = R.line_spans(buf)
    assert [spans[i][1] - spans[i][0] for i in (o[2], o[-1])] == [70000, 70000]
    check_engine(eng, buf)
    both_modes(buf, tmp_path)
    buf = b"\n".join(lines[:50] + [long_line(b"1", b"1", 70000)] + lines[50:] + [long_line(b"zz", b"1", 70000)])
    o = R.order(buf, True, True)
    spans = R.line_spans(buf)
    assert [spans[i][1] - spans[i][0] for i in (o[2], o[-1])] == [70000, 70000]
    check_engine(eng, buf)  # (and no final newline)


@pytest.mark.parametrize("block", [64, 4096])
def test_small_text_blocks(block, tmp_path, monkeypatch):
    """VCFXG_SRT_BLOCK = 64 bytes: a block holds one or two lines and most lines start one (the
    sweep's lines of 1..70 bytes: cuts between lines of every length, lines longer than a block);
    4 KiB: blocks of many lines; one line of 10,000 bytes exceeds either block and is taken alone"""
    monkeypatch.setenv("VCFXG_SRT_BLOCK", str(block))
    e = engine.Engine(0)
    try:
        buf = R.generated("mix")
        lines = buf.split(b"\n")
        buf = b"\n".join(lines[:200] + [long_line(b"2", b"77", 10000)] + lines[200:])
        check_engine(e, buf)
        check_engine(e, alignment_sweep(), COMBOS[1:2])
        # every call takes as many lines as fit the block, one at least
        e.load(buf)
        e.index(0)
        s = e.sort(engine.MODE_FILE)[0]
        spans = R.line_spans(buf)
        size = [spans[i][1] - spans[i][0] + 1 for i in R.order(buf, False)]
        calls, j, most = 0, 0, 0
        while j < s.rows:
            k, text = e.sort_text(j)
            assert k >= 1 and len(text) == sum(size[j:j + k]) and (len(text) <= block or k == 1)
            assert j + k == s.rows or len(text) + size[j + k] > block
            most = max(most, len(text))
            j += k
            calls += 1
        assert most > 10000 and max(size) > 10000
        assert s.rows / 3 < calls <= s.rows if block == 64 else 5 < calls < s.rows / 20
    finally:
        e.close()
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    assert _run_bin([TOOL, str(path)], env={"VCFXG_SRT_BLOCK": str(block)}) == R.run([TOOL, str(path)])


# POS fields at the edges of std::stoi's grammar and of int, which the stdin mode reads through the
# 64-bit C integer front end it shares with the merger and the duplicate remover (" \t7": the field
# is the blank before the tab)
POS_EDGES = [b"2147483647", b"2147483648", b"-2147483648", b"-2147483649", b"9223372036854775808",
             b"99999999999999999999", b"+5", b" \t7", b"", b"-"]


@pytest.mark.parametrize("pos", POS_EDGES, ids=[repr(p.decode()) for p in POS_EDGES])
def test_pos_edges_on_one_line(eng, pos):
    """a header and one data line (and the same line after a line that sorts on either side of any
    int): statuses, order and text of both modes against the restatement of std::stoi"""
    line = R.record(b"1", pos) + b"\n"
    for buf in (R.HDR + line, R.HDR + R.record(b"1", b"0") + b"\n" + line):
        check_engine(eng, buf)
    want = R.stoi(pos.split(b"\t")[0])
    assert R.statuses(R.HDR + line, True)[0][-1] == (R.BAD if want is None else R.KEPT)


def test_sorted_reversed_and_equal_inputs(eng, tmp_path):
    buf = R.gen_vcf(5, 1500, pad=60)
    lines = R.sort_bytes(buf, False)[0].split(b"\n")[2:-1]
    assert len(lines) == 1500
    ordered = R.HDR + b"\n".join(lines) + b"\n"
    assert R.sort_bytes(ordered, False)[0] == ordered
    check_engine(eng, ordered)
    rev = R.HDR + b"\n".join(lines[::-1]) + b"\n"
    assert R.sort_bytes(rev, False)[0] == ordered
    check_engine(eng, rev)
    # all keys equal: the output is the input
    same = R.HDR + b"\n".join(R.record(b"chr7", b"1234", b"id%d" % i, b"A\tC\t.\t.\tX=" + b"y" * (i % 90)) for i in range(1500)) + b"\n"
    for stdin in (False, True):
        for natural in (False, True):
            assert R.sort_bytes(same, stdin, natural)[0] == same
    check_engine(eng, same)
    both_modes(same, tmp_path)


@pytest.mark.parametrize("name", ["ties_a.vcf", "ties_b.vcf"])
def test_ties_fixtures_are_sorted_stably(eng, name, tmp_path):
    with open(os.path.join(R.GOLDEN, "sorter", name), "rb") as f:
        buf = f.read()
    check_engine(eng, buf)
    both_modes(buf, tmp_path)
    both_modes(buf, tmp_path, extra=("-n",))


def test_chrom_lengths_change_the_passes(eng, tmp_path):
    """2-byte names alone (one CHROM word), then with names of 9, 16, 17 and 40 bytes (up to five),
    names that differ only past byte 8, 16 and 32, a NUL byte inside a name, and stdin mode's empty
    CHROM behind a name of 0xFF bytes"""
    rnd = random.Random(40)
    two = [b"%c%c" % (rnd.choice(b"abcXYZ"), rnd.choice(b"0123456789")) for _ in range(12)]
    # (3,000 lines: past the one-block sort, where the trimmed last word must still order all lines)
    check_engine(eng, R.gen_vcf(40, 3000, chroms=tuple(two)))
    check_engine(eng, R.gen_vcf(41, 3000, chroms=(b"1", b"2", b"3", b"X")))
    b40 = b"contig_with_a_name_of_forty_bytes_abcdef"
    assert len(b40) == 40
    names = two + [b40, b40[:39] + b"g", b40[:33] + b"X" * 7, b40[:16], b40[:17], b40[:16] + b"~", b40[:8], b40[:9], b40[:8] + b"\x00",
                   b40[:8] + b"\x00\x00", b"a\x00b", b"a\x00", b"a", b"\xff" * 8, b"\xff" * 9, b"\xff", b""]
    for n in (len(two), len(names)):
        lines = [R.record(c, b"%d" % p, b"c%dp%d" % (i, p)) for i, c in enumerate(names[:n]) for p in (5, 3, 70000)]
        rnd.shuffle(lines)
        buf = R.HDR + b"\n".join(lines) + b"\n"
        check_engine(eng, buf)
        both_modes(buf, tmp_path, "w%d" % n)


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
    want = R.run([TOOL, str(plain)])
    assert want[0].count(b"\n") > 2000 and want[1]
    assert tools.run([TOOL, str(plain)]) == want
    assert tools.run([TOOL, str(comp)]) == want
    # inflated on the device (the lines are gathered from there)
    assert _run_bin([TOOL, "-n", str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1"}) == R.run([TOOL, "-n", str(plain)])
    assert _run_bin([TOOL], comp.read_bytes(), env={"VCFX_BGZF_DEVICE_MIN": "1"}) == R.run([TOOL], buf)


def test_ngpu_gives_the_unsharded_bytes(tmp_path):
    buf = R.generated("routes")
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    argv = [TOOL, str(path)]
    assert tools.shard_plan(argv, 2)[0] == 1
    want = R.run(argv)
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": "2"}) == want


def test_pipe_chain_starting_with_the_tool():
    """vcfx_pipe 'VCFX_sorter -n | VCFX_duplicate_remover -q' against the duplicate remover on the
    restatement's output"""
    buf = R.generated("mix_ties")
    ordered = R.run([TOOL, "-n"], buf)[0]
    want = tools.run(["VCFX_duplicate_remover", "-q"], ordered)
    assert want[2] == 0 and want[0].count(b"\n") > 50
    r = subprocess.run([PIPE, "%s -n | VCFX_duplicate_remover -q" % TOOL], input=buf, capture_output=True, timeout=120)
    assert (r.stdout, r.returncode) == (want[0], 0)


def test_calls_need_a_sort(eng):
    eng.load(b"#CHROM\n2\t5\t.\n1\t5\t.\n")
    eng.index(0)
    st, o = np.zeros(3, np.uint8), np.zeros(3, np.uint32)
    k, n = engine.ctypes.c_uint64(), engine.ctypes.c_uint64()
    assert eng.L.vcfxg_sort_status(eng.h, 0, 1, st.ctypes.data) == -5  # VCFXG_E_STATE: no sort on this index
    assert eng.L.vcfxg_sort_order(eng.h, 0, 1, o.ctypes.data) == -5
    assert eng.L.vcfxg_sort_text(eng.h, 0, engine.ctypes.byref(k), engine.ctypes.byref(n)) == -5
    s, got, cnt, order = eng.sort(engine.MODE_FILE)
    assert got.tolist() == [R.HEADER, R.KEPT, R.KEPT] and order.tolist() == [0, 2, 1]
    assert eng.L.vcfxg_sort_status(eng.h, 0, 3, st.ctypes.data) == 0 and st.tolist() == got.tolist()
    assert eng.L.vcfxg_sort_status(eng.h, 3, 1, st.ctypes.data) == -3  # VCFXG_E_ARG
    assert eng.L.vcfxg_sort_order(eng.h, 3, 1, o.ctypes.data) == -3
    assert eng.sort_text(3) == (0, b"") and eng.sort_text(1) == (2, b"1\t5\t.\n2\t5\t.\n")
    eng.index(0)  # a new index: the sort is gone
    assert eng.L.vcfxg_sort_order(eng.h, 0, 1, o.ctypes.data) == -5
