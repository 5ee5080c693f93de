"""GPU parity of VCFX_diff_tool: every recorded case of the compiled reference
(tests/golden/diff_tool_cases.json.gz) through the in-process drop-in and the executable (byte for
byte where the case is `ordered`: every -s case and every case whose sides hold at most one key;
else byte for byte against the restatement's input order AND by same_sections against the
reference's bytes); per-line statuses, counts, the path taken and both sides' text of the raw ABI
against the plain-Python restatement (tests/_diff_tool_ref.py, itself held to the recorded cases by
tests/test_diff_tool_ref.py): data-line counts around the kernels' and the sort's tiles, key fields
that end at the lane window's edge, a 70,000-byte REF, an ALT of 200 tokens, forced hash collisions,
text blocks of 64 bytes and 4 KiB, the serial walk seven steps a launch, sorted pairs whose equal
lines print different keys, empty files, gzip input and VCFX_NGPU=2."""
import gzip
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _diff_tool_ref as R
from tests._golden import REPO
from vcfx_amd import engine, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
CASES = R.load_cases()
W = R.WINDOW
MODES = ((False, False), (True, False), (True, True))  # (assume_sorted, natural)


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def case_env(case):
    return dict(os.environ, **case["env"])


def expected_stdout(case):
    """what the drop-in must print: the recorded bytes, or for an unordered case each side in input
    order of the key's first line (the same sections as the recorded bytes)"""
    if case["ordered"]:
        return case["stdout"]
    want = R.run(case["argv"], cwd=R.GOLDEN)[0]
    assert R.same_sections(want, case["stdout"])
    return want


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_in_process(case, monkeypatch):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    out, err, rc = tools.run(case["argv"], b"", cwd=R.GOLDEN)
    assert rc == case["rc"]
    assert out == expected_stdout(case)
    assert err == case["stderr"]


def test_golden_binary(monkeypatch):
    """the executable on every golden case (a process each, twelve at a time; argv[0] is the tool's
    name, as recorded, so that getopt's messages match)"""
    assert os.access(BIN, os.X_OK)

    def want(case):
        for k, v in case["env"].items():
            monkeypatch.setenv(k, v)
        w = expected_stdout(case)
        for k in case["env"]:
            monkeypatch.delenv(k)
        return w

    wants = [want(c) for c in CASES]

    def one(args):
        case, w = args
        r = subprocess.run(case["argv"], executable=BIN, input=b"", capture_output=True, cwd=R.GOLDEN, timeout=120,
                           env=case_env(case))
        return (r.returncode, r.stdout, r.stderr) == (case["rc"], w, case["stderr"])

    with ThreadPoolExecutor(12) as ex:
        ok = list(ex.map(one, zip(CASES, wants)))
    assert all(ok), [c["name"] for c, v in zip(CASES, ok) if not v]


def check_engine(e, f1, f2, modes=MODES, hash_bits=(0,)):
    """statuses, summary, counts, the path and both sides' text of the raw ABI against the restatement"""
    buf, second = R.join(f1, f2)
    e.load(buf)
    assert e.index(0) == len(R.line_spans(buf))
    for assume_sorted, natural in modes:
        want, s1, s2, path, cut, waves = R.diff(f1, f2, assume_sorted, natural)
        data = [sum(1 for i, v in enumerate(want) if v in (R.COMMON, R.UNIQUE, R.REPEAT) and (i >= cut) == side) for side in (False, True)]
        for bits in hash_bits if not assume_sorted else (0,):
            where = (assume_sorted, natural, bits)
            s, st, cnt = e.diff(second, assume_sorted, natural, bits)
            assert st.tolist() == want, (where, [(i, a, b) for i, (a, b) in enumerate(zip(st.tolist(), want)) if a != b][:10])
            assert cnt == (len(s1), len(s2), data[0], data[1], want.count(R.SKIPPED), waves, path, cut), where
            assert (s.n_lines, s.rows, s.data_lines, s.warn_lines, s.general_records) == \
                (len(want), len(s1) + len(s2), sum(data), want.count(R.SKIPPED), waves), where
            for side, keys in enumerate((s1, s2)):
                text, exp = e.diffed_text(side), b"".join(k + b"\n" for k in keys)
                assert len(text) == len(exp), (where, side)
                assert text == exp, (where, side, next(i for i in range(len(exp)) if text[i] != exp[i]))


def run_files(tmp_path, f1, f2, extra=(), tag=""):
    """the drop-in on two files against the restatement"""
    a, b = tmp_path / ("a%s.vcf" % tag), tmp_path / ("b%s.vcf" % tag)
    a.write_bytes(f1)
    b.write_bytes(f2)
    argv = [TOOL, "-a", str(a), "-b", str(b)] + list(extra)
    got, want = tools.run(argv, b""), R.run(argv)
    assert got == want, (extra, tag, len(got[0]), len(want[0]))
    return argv, want


def test_golden_fixtures_per_line(eng):
    """every pair of fixtures a recorded case compares, through the raw ABI"""
    pairs = set()
    for c in CASES:
        got = {k: v for k, v, _ in R.getopt_long(c["argv"])[0]}
        if c["rc"] == 0 and not c["env"] and got.get("a") and got.get("b") and "longpos" not in got["a"]:
            pairs.add((got["a"], got["b"]))
    assert len(pairs) >= 30
    for a, b in sorted(pairs):
        f1, f2 = R.read_input(a, R.GOLDEN), R.read_input(b, R.GOLDEN)
        if f1 is not None and f2 is not None:
            check_engine(eng, f1, f2)
    check_engine(eng, R.read_input("diff_tool/longpos_a.vcf", R.GOLDEN), R.read_input("diff_tool/longpos_b.vcf", R.GOLDEN), MODES[:1])


@pytest.mark.parametrize("n1,n2", [(0, 1), (1, 0), (1, 1), (63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255)])
def test_data_line_counts(eng, n1, n2, tmp_path):
    """data lines per side around the wave, the block and the sort's tiles; sorted and not"""
    for ordered in (False, True):
        f1 = R.gen_file(n1, n1, mix=True, ordered=ordered)
        f2 = R.gen_file(1000 + n2, n2, mix=True, ordered=ordered)
        check_engine(eng, f1, f2)
    run_files(tmp_path, f1, f2)
    run_files(tmp_path, f1, f2, ("-s",))


def edge_line(end, tabs5=True):
    """a data line whose fifth tab (or, without one, whose end) is byte `end` of the line"""
    head = b"c\t5\t.\t"
    alt = b"G,T"
    ref = b"A" * (end - len(head) - 1 - len(alt))
    line = head + ref + b"\t" + alt
    assert len(line) == end
    return line + (b"\tq\tf\tINFO=" + b"x" * 40 if tabs5 else b"")


@pytest.mark.parametrize("end", [63, 64, 65])
def test_key_fields_end_at_the_window_edge(eng, end):
    """the fifth tab at byte 63 (the lane's last), 64 and 65 (the wave's), and lines of exactly that
    length without a fifth tab; in both files, shared and not"""
    lines = [edge_line(end), edge_line(end, False), edge_line(end)[:-1] + b"\r", R.rec(b"1", b"5")]
    f1 = R.HDR + b"\n".join(lines) + b"\n"
    f2 = R.HDR + b"\n".join([lines[0], edge_line(end - 1), lines[1] + b"\r"]) + b"\n"
    # byte 63 is the window's last: a fifth tab there, and a line of 64 bytes, are the lane's
    assert R.lane_path(edge_line(63)) and not R.lane_path(edge_line(64)) and not R.lane_path(edge_line(65))
    assert R.lane_path(edge_line(64, False)) and not R.lane_path(edge_line(65, False))
    assert (R.diff(f1, f2)[5] == 0) == (end == 63)
    check_engine(eng, f1, f2)


def test_long_ref_and_many_alt_tokens(eng, tmp_path):
    """a 70,000-byte REF; an ALT of 200 tokens with empty and repeated ones, permuted in file 2"""
    rnd = random.Random(70)
    ref = bytes(rnd.choice(b"ACGT") for _ in range(70000))
    toks = [bytes(rnd.choice(b"ACGT") for _ in range(rnd.randrange(0, 6))) for _ in range(200)]
    toks[17], toks[90], toks[199] = b"", b"", toks[3]
    assert toks.count(b"") >= 2 and len(toks) == 200 and len(set(toks)) < 190
    perm = list(toks)
    rnd.shuffle(perm)
    f1 = R.HDR + b"\n".join([R.rec(b"1", b"5", ref, b"T"), R.rec(b"2", b"6", b"A", b",".join(toks)), R.rec(b"3", b"7", ref, b",".join(toks[:70])),
                             R.rec(b"4", b"8", b"A", b",".join(toks[:5]))]) + b"\n"
    f2 = R.HDR + b"\n".join([R.rec(b"2", b"6", b"A", b",".join(perm)), R.rec(b"1", b"5", ref[:-1] + b"N", b"T"),
                             R.rec(b"3", b"7", ref, b",".join(reversed(toks[:70]))), R.rec(b"4", b"8", b"A", b",".join(toks[4::-1])),
                             R.rec(b"1", b"5", ref, b"T")]) + b"\n"
    st = R.diff(f1, f2)
    assert (len(st[1]), len(st[2])) == (0, 1)  # only the REF that ends in N is unique
    check_engine(eng, f1, f2)
    run_files(tmp_path, f1, f2)


def test_forced_hash_collisions_give_the_same_answers(eng):
    """hash_bits 1, 2 and 3: two, four and eight runs hold every key; the statuses and the text are
    those of the full hash"""
    f1, f2 = R.gen_file(31, 300, mix=True, span=4), R.gen_file(32, 300, mix=True, span=4)
    st = R.diff(f1, f2)[0]
    assert min(st.count(k) for k in (R.COMMON, R.UNIQUE, R.REPEAT)) >= 20
    check_engine(eng, f1, f2, MODES[:1], hash_bits=(0, 1, 2, 3))
    for name in ("alts", "rules", "collide"):
        a, b = (R.read_input("diff_tool/%s_%s.vcf" % (name, x), R.GOLDEN) for x in "ab")
        check_engine(eng, a, b, MODES[:1], hash_bits=(1, 2, 3))


@pytest.mark.parametrize("block", [64, 4096])
def test_small_text_blocks(block, tmp_path, monkeypatch):
    """VCFXG_DF_BLOCK = 64 bytes: a block holds a few keys; 4 KiB: many; one key of 10,000 bytes exceeds
    either block and is taken alone"""
    monkeypatch.setenv("VCFXG_DF_BLOCK", str(block))
    f1 = R.gen_file(41, 300, span=4000)
    f1 += R.rec(b"9", b"1", b"A" * 10000) + b"\n" + b"".join(R.rec(b"9", b"%d" % i) + b"\n" for i in range(2, 40))
    f2 = R.gen_file(42, 300, span=4000)
    e = engine.Engine(0)
    try:
        check_engine(e, f1, f2)
        buf, second = R.join(f1, f2)
        e.load(buf)
        e.index(0)
        e.diff(second)
        for side, keys in enumerate(R.diff(f1, f2)[1:3]):
            size = [len(k) + 1 for k in keys]
            calls, j, most = 0, 0, 0
            while j < len(keys):
                k, text = e.diff_text(side, j)
                assert k >= 1 and len(text) == sum(size[j:j + k]) and (len(text) <= block or k == 1)
                assert j + k == len(keys) or len(text) + size[j + k] > block
                most = max(most, len(text))
                j += k
                calls += 1
            assert len(keys) > 100
            assert len(keys) / 8 < calls <= len(keys) if block == 64 else 1 <= calls < len(keys) / 20
            assert side == 1 or most > 10000
            assert e.diff_text(side, len(keys)) == (0, b"")
    finally:
        e.close()
    argv, want = run_files(tmp_path, f1, f2)
    r = subprocess.run(argv, executable=BIN, input=b"", capture_output=True, timeout=120, env=dict(os.environ))
    assert (r.stdout, r.stderr, r.returncode) == want


def test_serial_walk_seven_steps_a_launch(monkeypatch, tmp_path):
    """a 100-line pair, each file unsorted: the serial walk, seven steps a launch (fifteen launches and
    more carry the pointers in device memory); then unsorted on one side only"""
    monkeypatch.setenv("VCFXG_DF_WALK_STEPS", "7")
    f1, f2 = R.gen_file(51, 50), R.gen_file(52, 50)
    assert R.diff(f1, f2, True)[3] == R.PATH_WALK
    e = engine.Engine(0)
    try:
        check_engine(e, f1, f2, MODES[1:])
        check_engine(e, R.gen_file(51, 50, ordered=True), f2, MODES[1:2])
        check_engine(e, f1, R.gen_file(52, 50, ordered=True, natural=True), MODES[2:])
        check_engine(e, f1, R.HDR, MODES[1:2])
    finally:
        e.close()
    argv, want = run_files(tmp_path, f1, f2, ("-s",))
    r = subprocess.run(argv, executable=BIN, input=b"", capture_output=True, timeout=120, env=dict(os.environ))
    assert (r.stdout, r.stderr, r.returncode) == want


def test_sorted_pairs_whose_equal_lines_print_different_keys(eng, tmp_path):
    """runs of lines that compare equal (POS 7 / 07 / 007; with -n the names 1 / chr1 / 01 / CHR1; ALT
    compared unsorted) of different lengths in the two files: the bounds path reports the later
    occurrences, each with its own key text"""
    rnd = random.Random(61)
    rows = []
    for pos in range(1, 60):
        for name in (b"1", b"chr1", b"01", b"CHR1"):
            for z in range(rnd.randrange(0, 3)):
                rows.append(R.rec(name, b"0" * rnd.randrange(0, 3) + b"%d" % pos, b"A", rnd.choice((b"C,T", b"T,C"))))
    for natural in (False, True):
        def srt(lines):
            return sorted(lines, key=lambda l: R.sort_key(R.parse(l)[1], natural))
        f1 = R.HDR + b"\n".join(srt(rnd.sample(rows, len(rows) * 2 // 3))) + b"\n"
        f2 = R.HDR + b"\n".join(srt(rnd.sample(rows, len(rows) * 2 // 3))) + b"\n"
        st, s1, s2, path, _, _ = R.diff(f1, f2, True, natural)
        assert path == R.PATH_BOUNDS and len(s1) > 20 and len(s2) > 20
        check_engine(eng, f1, f2, ((True, natural),))
        run_files(tmp_path, f1, f2, ("-s", "-n") if natural else ("-s",), tag=str(natural))


def test_empty_files_and_missing_final_newline(eng, tmp_path):
    f = R.gen_file(71, 40, mix=True)
    for f1, f2 in ((b"", f), (f, b""), (f[:-1], f), (f[:-1], b""), (b"", f[:-1]), (R.rec(b"1", b"5"), R.rec(b"1", b"5")),
                   (R.rec(b"1", b"5"), R.rec(b"1", b"6") + b"\n"), (b"\n", b"\n\n"), (R.HDR, R.HDR[:-1])):
        check_engine(eng, f1, f2)
        run_files(tmp_path, f1, f2)
        run_files(tmp_path, f1, f2, ("-s", "-n"))


def test_calls_need_a_diff(eng):
    buf, second = R.join(R.rec(b"1", b"5") + b"\n", R.rec(b"1", b"6") + b"\n")
    eng.load(buf)
    eng.index(0)
    st = np.zeros(3, np.uint8)
    k, n = engine.ctypes.c_uint64(), engine.ctypes.c_uint64()
    assert eng.L.vcfxg_diff_status(eng.h, 0, 1, st.ctypes.data) == -5  # VCFXG_E_STATE: no diff on this index
    assert eng.L.vcfxg_diff_text(eng.h, 0, 0, engine.ctypes.byref(k), engine.ctypes.byref(n)) == -5
    s, got, cnt = eng.diff(second)
    assert got.tolist() == [R.UNIQUE, R.UNIQUE] and cnt == (1, 1, 1, 1, 0, 0, R.PATH_HASH, 1)
    assert eng.diff_text(0, 0) == (1, b"1:5:A:T\n") and eng.diff_text(1, 0) == (1, b"1:6:A:T\n") and eng.diff_text(1, 1) == (0, b"")
    assert eng.L.vcfxg_diff_status(eng.h, 2, 1, st.ctypes.data) == -3  # VCFXG_E_ARG
    assert eng.L.vcfxg_diff_text(eng.h, 2, 0, engine.ctypes.byref(k), engine.ctypes.byref(n)) == -3
    assert eng.L.vcfxg_diff_text(eng.h, 0, 2, engine.ctypes.byref(k), engine.ctypes.byref(n)) == -3
    p = engine.DfParams(len(buf) + 1, 0, 0, 0)
    assert eng.L.vcfxg_diff(eng.h, engine.ctypes.byref(p), None) == -3  # file 2 cannot begin past the end
    eng.index(0)  # a new index: the diff is gone
    assert eng.L.vcfxg_diff_status(eng.h, 0, 1, st.ctypes.data) == -5


def _run_bin(argv, env=None):
    r = subprocess.run(argv, executable=BIN, input=b"", capture_output=True, timeout=120, env=dict(os.environ, **(env or {})))
    return r.stdout, r.stderr, r.returncode


def test_gzip_pair_gives_the_plain_output(tmp_path):
    from tests import _bgzf
    f1, f2 = R.gen_file(81, 400, mix=True), R.gen_file(82, 400, mix=True, final_newline=False)
    a, b, ag, bg = tmp_path / "a.vcf", tmp_path / "b.vcf", tmp_path / "a.vcf.gz", tmp_path / "b.vcf.gz"
    a.write_bytes(f1)
    b.write_bytes(f2)
    ag.write_bytes(gzip.compress(f1, mtime=0))
    bg.write_bytes(_bgzf.bgzf(f2))
    for extra in ([], ["-s"]):
        plain = R.run([TOOL, "-a", str(a), "-b", str(b)] + extra)
        assert plain[0].count(b"\n") > 100
        got = tools.run([TOOL, "-a", str(ag), "-b", str(bg)] + extra, b"")
        assert got[1:] == plain[1:] and got[0] == plain[0].replace(str(a).encode(), str(ag).encode()).replace(str(b).encode(), str(bg).encode())
        assert _run_bin([TOOL, "-a", str(ag), "-b", str(b)] + extra)[0] == plain[0].replace(str(a).encode(), str(ag).encode())


def test_ngpu_gives_the_unsharded_bytes(tmp_path):
    a, b = tmp_path / "a.vcf", tmp_path / "b.vcf"
    a.write_bytes(R.gen_file(91, 500, mix=True))
    b.write_bytes(R.gen_file(92, 500, mix=True))
    argv = [TOOL, "-a", str(a), "-b", str(b)]
    assert tools.shard_plan(argv, 2)[0] == 1
    want = R.run(argv)
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": "2"}) == want
