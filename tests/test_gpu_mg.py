"""GPU parity of VCFX_merger: every recorded case of the compiled reference
(tests/golden/merger_cases.json.gz) through the in-process drop-in and the executable (byte for byte
where the case is `ordered`; a ties_* case byte for byte against the stable restatement AND by
same_under_ties against the reference's bytes); per-line statuses, counts, per-file figures, the
order, the path taken and the text of the raw ABI against the plain-Python restatement
(tests/_merger_ref.py, itself held to the recorded cases by tests/test_merger_ref.py), each shape in
the default mode, -s, -n and -s -n: the second tab and the POS digits at the lane window's edge, key
strings around the 8-byte words, 5,000-byte names, NUL and high bytes, every POS form, kept-line
counts around the kernels' and the sort's tiles, 1 to 65 files, the walk seven steps a launch, ties,
a run of 5,000 equal keys, a generated cohort file dealt into three, and VCFX_NGPU=2."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _merger_ref as R
from tests._golden import REPO
from vcfx_amd import engine, synth, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
CASES = R.load_cases()
W = R.WINDOW
MODES = ((False, False), (True, False), (False, True), (True, True))  # (assume_sorted, natural)
rec = R.rec


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


def is_natural(case):
    return any(k == "n" for k, _, _ in R.getopt_long(case["argv"])[0])


def expected_stdout(case):
    """what the drop-in must print: the recorded bytes, or for a ties_* case the stable order (the
    same header, keys and runs as the recorded bytes)"""
    if case["ordered"]:
        return case["stdout"]
    want = R.run(case["argv"], cwd=R.GOLDEN)[0]
    assert R.same_under_ties(want, case["stdout"], is_natural(case))
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
                           env=dict(os.environ, **case["env"]))
        return (r.returncode, r.stdout, r.stderr) == (case["rc"], w, case["stderr"])

    with ThreadPoolExecutor(12) as ex:
        ok = list(ex.map(one, zip(CASES, wants)))
    assert all(ok), [c["name"] for c, v in zip(CASES, ok) if not v]


def check_engine(e, files, modes=MODES, path=None):
    """statuses, summary, counts, per-file figures, the order and the text of the raw ABI against the
    restatement; returns the restatement's results per mode"""
    buf, starts = R.join(files)
    e.load(buf)
    assert e.index(0) == len(R.line_spans(buf))
    res = []
    for assume_sorted, natural in modes:
        where = (assume_sorted, natural)
        m = R.merge(files, assume_sorted, natural)
        s, st, cnt, order = e.merge(starts, assume_sorted, natural)
        assert st.tolist() == m.statuses, (where, [(i, a, b) for i, (a, b) in enumerate(zip(st.tolist(), m.statuses)) if a != b][:10])
        assert cnt == m.counts, where
        if path is not None:
            assert cnt[6] == path, where
        assert (s.n_lines, s.rows, s.data_lines, s.warn_lines, s.general_records) == \
            (len(m.statuses), len(m.order), m.statuses.count(R.KEPT), m.statuses.count(R.BAD), m.waves), where
        assert e.merge_files(len(files)) == (m.first_line, m.bad), where
        assert order.tolist() == m.order, (where, next(i for i in range(len(m.order)) if order[i] != m.order[i]))
        text = e.merged_text(s.rows)
        assert len(text) == len(m.text), where
        assert text == m.text, (where, next(i for i in range(len(text)) if text[i] != m.text[i]))
        res.append(m)
    return res


def run_files(tmp_path, files, extra=(), tag=""):
    """the drop-in on the files against the restatement"""
    paths = []
    for i, f in enumerate(files):
        p = tmp_path / ("f%s_%d.vcf" % (tag, i))
        p.write_bytes(f)
        paths.append(str(p))
    argv = [TOOL, "-m", ",".join(paths)] + list(extra)
    got, want = tools.run(argv, b""), R.run(argv)
    assert got == want, (extra, tag, len(got[0]), len(want[0]))
    return argv, want


def test_status_before_a_merge_is_a_state_error(eng):
    eng.load(b"1\t5\t.\n")
    eng.index(0)
    st, w = np.zeros(4, np.uint8), np.zeros(8, np.uint64)
    assert eng.L.vcfxg_merge_status(eng.h, 0, 1, st.ctypes.data) == -5  # VCFXG_E_STATE: no merge on this index
    assert eng.L.vcfxg_merge_counts(eng.h, w.ctypes.data) == -5
    assert eng.L.vcfxg_merge_files(eng.h, w.ctypes.data, w.ctypes.data) == -5
    assert eng.L.vcfxg_merge_order(eng.h, 0, 0, w.ctypes.data) == -5
    assert eng.L.vcfxg_merge_text(eng.h, 0, None, None) == -5
    s, st, cnt, order = eng.merge([0, 6])
    assert (st.tolist(), order.tolist()) == ([R.KEPT], [0])
    assert eng.L.vcfxg_merge_status(eng.h, 1, 1, st.ctypes.data) == -3  # VCFXG_E_ARG: a bad range
    assert eng.L.vcfxg_merge_order(eng.h, 0, 2, w.ctypes.data) == -3
    assert eng.L.vcfxg_merge_text(eng.h, 2, None, None) == -3
    for starts in ([0, 7], [1, 6], [0, 4, 2, 6]):  # the offsets must be non-decreasing from 0 to the size
        fs = np.array(starts, np.uint64)
        p = engine.MgParams(fs.ctypes.data, len(starts) - 1, 0, 0)
        assert eng.L.vcfxg_merge(eng.h, engine.ctypes.byref(p), None) == -3
    eng.index(0)  # a new index forgets the merge
    assert eng.L.vcfxg_merge_status(eng.h, 0, 1, st.ctypes.data) == -5


def test_golden_fixtures_per_line(eng):
    """every list of fixtures a recorded case merges, through the raw ABI"""
    lists = set()
    for c in CASES:
        opts = R.getopt_long(c["argv"])[0]
        names = R.split_names([v for k, v, _ in opts if k == "m"])
        if names and not c["env"] and c["stdout"] not in (R.HELP, R.VERSION):
            lists.add(tuple(names))
    assert len(lists) >= 35
    for names in sorted(lists):
        files = [f for f in (R.read_input(n, R.GOLDEN) for n in names) if f is not None]
        if files and any(files):
            check_engine(eng, files)


def test_window_edges(eng):
    """the second tab at byte 62, 63, 64 and 65 of the line and far beyond, and POS digits that cross
    the window; lane-path and wave-path lines with EQUAL keys next to each other"""
    lines = []
    for n in (59, 60, 61, 62, 63, 64, 70, 200):  # CHROM of n bytes, POS "5": the second tab at byte n + 2
        lines.append(b"c" * n + b"\t5\t.\tlane or wave %d" % n)
    for z in (40, 57, 58, 59, 60, 61, 62, 63, 100):  # "w", z zeros and "7": the second tab at byte z + 3
        lines.append(b"w\t" + b"0" * z + b"7\t.\t%d zeros" % z)
    lines += [b"w\t7\t.\tshort", b"w\t" + b" " * 80 + b"+7\t.\tspaces", b"w\t7" + b"x" * 90 + b"\t.\ttail",
              b"w\t" + b"0" * 90 + b"\t.", b"w\t" + b"0" * 61 + b"x\t.", b"q" * 64, b"q" * 65, b"q\t" + b"1" * 64, b"q\t" + b"1" * 70 + b"\t.",
              b"chr" + b"9" * 3 + b"s" * 70 + b"\t5\t.", b"chr" + b"0" * 70 + b"9\t5\t.", b"9\t5\t.\tnum 9 again"]
    paths = [R.lane_path(l) for l in lines]
    assert paths.count(True) >= 8 and paths.count(False) >= 12
    rnd = random.Random(5)
    for trial in range(3):
        rnd.shuffle(lines)
        files = [R.HDR + b"\n".join(lines[:15]) + b"\n", b"\n".join(lines[15:]) + b"\n", b"\n".join(lines[:6])]
        res = check_engine(eng, files)
        assert all(m.ties for m in res) and res[0].waves >= 12


def test_key_string_lengths(eng):
    """CHROM (with -n: the suffix) of 0, 1, 7, 8, 9, 15, 16, 17 and 24 bytes, names that differ only past the
    first word, a prefix before its extensions, and two 5,000-byte names that differ in the last byte"""
    stems = [b"", b"a", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefghijklmno", b"abcdefghijklmnop", b"abcdefghijklmnopq",
             b"abcdefghijklmnopqrstuvwx", b"abcdefgh\x00", b"abcdefgi", b"abcdefghj", b"abcdefghijklmnoq", b"abcdefghijklmnopr",
             b"L" * 4999 + b"a", b"L" * 4999 + b"b", b"L" * 4999, b"L" * 5000 + b"\x00"]
    names = stems + [b"chr" + s for s in stems] + [b"7" + s for s in stems] + [b"Chr12" + s for s in stems]
    lines = [rec(n, b"%d" % (3 + i % 2)) for i, n in enumerate(names)] + [rec(n, b"1") for n in names[::3]]
    random.Random(9).shuffle(lines)
    files = [R.HDR + b"".join(l + b"\n" for l in lines[k::3]) for k in range(3)]
    check_engine(eng, files)
    for natural in (False, True):  # and sorted files of them: the sort path under -s
        srt = [R.HDR + b"".join(l + b"\n" for l in sorted(lines[k::3], key=lambda l: R.sort_key(*R.parse(l)[1:], natural)))
               for k in range(3)]
        check_engine(eng, srt, [(True, natural)], path=R.PATH_SORT)


def test_bytes_and_pos_forms(eng):
    """a NUL and bytes >= 0x80 in CHROM; every POS form, both long extremes, the first value past each
    and 30 leading zeros"""
    names = [b"n\x00ul", b"n\x00", b"n", b"\x00", b"\x80", b"\xff\xfe", b"\xc3\xa9", b"chr\xff", b"chr\x00", b"\x7f", b"chr9\x80", b"9\x00"]
    forms = [b" 7", b"\v8", b"\f9", b"\r10", b"+3", b"-5", b"0x10", b"5abc", b"0070", b"0" * 30 + b"12", b"", b"-", b"- 3", b"abc",
             b"9223372036854775808", b"9223372036854775807", b"-9223372036854775808", b"-9223372036854775809",
             b"9223372036854775806", b"-9223372036854775807", b"18446744073709551616", b"18446744073709551621", b"1.5", b"+-3",
             b" +4", b"-" + b"0" * 70 + b"6", b"0" * 200, b"99999999999999999999999", b"0", b"-0", b"+0"]
    lines = [rec(n, b"%d" % i) for i, n in enumerate(names)] + [rec(b"p", f) for f in forms] + [rec(b"chrp", f) for f in forms[::2]]
    random.Random(2).shuffle(lines)
    files = [b"".join(l + b"\n" for l in lines[:30]), R.HDR + b"".join(l + b"\n" for l in lines[30:])]
    res = check_engine(eng, files)
    assert res[0].statuses.count(R.BAD) >= 12 and res[0].hdr == 1


# POS fields at the edges of long, which std::stol's restatement on the device tells apart by the
# exact 64-bit overflow test of the C integer front end it shares with the sorter
POS_EDGES = [b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809"]


@pytest.mark.parametrize("pos", POS_EDGES, ids=[p.decode() for p in POS_EDGES])
def test_long_limits_on_one_line(eng, pos):
    """a header and one data line, then two files of one line each: the first value outside long is
    BAD, the last one inside it is kept and ordered as itself"""
    line = rec(b"p", pos) + b"\n"
    inside = -2 ** 63 <= int(pos) < 2 ** 63
    for files in ([R.HDR + line], [R.HDR + line, rec(b"p", b"-1") + b"\n"]):
        res = check_engine(eng, files)
        assert res[0].statuses.count(R.BAD) == (0 if inside else 1)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_kept_line_counts(eng, n):
    """kept lines around the wave, the block and the sort's tiles, dealt into three files (unsorted:
    the sort path and the walk; sorted: the sort path under -s)"""
    lines = R.gen_records(n, n)
    check_engine(eng, R.deal(lines, 3, header=b""), MODES[:2] if n > 1000 else MODES)
    check_engine(eng, R.deal(lines, 3, natural=False), MODES[1:2], path=R.PATH_SORT)
    check_engine(eng, R.deal(lines, 3, natural=True), MODES[3:], path=R.PATH_SORT)


def test_three_thousand_lines_on_two_byte_names(eng):
    """the radix sort's merge-path sizes: one short word pass whose bit range ends below 64"""
    rnd = random.Random(3)
    names = [bytes([rnd.randrange(33, 127), rnd.randrange(33, 127)]) for _ in range(40)]
    lines = [rec(rnd.choice(names), b"%d" % i) for i in range(3000)]
    check_engine(eng, R.deal(lines, 2), MODES[:1] + MODES[2:3], path=R.PATH_SORT)
    check_engine(eng, R.deal(lines, 2, natural=False), MODES[1:2], path=R.PATH_SORT)


@pytest.mark.parametrize("k", [1, 2, 3, 64, 65])
def test_file_counts(eng, k):
    """K files of a few lines each, some empty, some with only a header, the header first in a late
    file; unsorted files: the walk's lanes stride the files (65: a second round)"""
    lines = R.gen_records(100 + k, 4 * k)
    files = R.deal(lines, k, header=b"")
    for f in range(k):
        if f % 7 == 3:
            files[f] = b""
        elif f % 7 == 5:
            files[f] = R.HDR
        elif f % 7 == 6:
            files[f] = b"##late header %d\n" % f + files[f]
    check_engine(eng, files)
    srt = R.deal(lines, k, natural=False, header=b"\n")
    check_engine(eng, srt, MODES[:2], path=R.PATH_SORT)


def test_a_last_line_without_newline_joins_the_next_file(eng, tmp_path):
    files = [R.HDR + rec(b"2", b"9"), rec(b"1", b"7") + b"\n" + rec(b"1", b"3"), b"#tail header", rec(b"0", b"1"), b"no tabs", b""]
    check_engine(eng, files)
    for extra in ((), ("-s",), ("-n",), ("-s", "-n")):
        run_files(tmp_path, files, extra, tag="".join(extra))


def test_walk_seven_steps_a_launch(monkeypatch, tmp_path):
    """unsorted files under -s: the walk, seven steps a launch (many launches carry the cursors and the
    output count in device memory), against the default step count; the counts show the path"""
    files = R.deal(R.gen_records(61, 200), 5)
    files[2] = b"##only this file has a header under -s\n" + files[2].replace(R.HDR, b"")
    files[0] = files[0].replace(R.HDR, b"")
    files[1] = files[1].replace(R.HDR, b"")
    e = engine.Engine(0)
    try:
        default = check_engine(e, files, (MODES[1], MODES[3]), path=R.PATH_WALK)
    finally:
        e.close()
    monkeypatch.setenv("VCFXG_MG_WALK_STEPS", "7")
    e = engine.Engine(0)
    try:
        seven = check_engine(e, files, (MODES[1], MODES[3]), path=R.PATH_WALK)
        assert [m.order for m in seven] == [m.order for m in default] and seven[0].hdr == 2
        check_engine(e, files, (MODES[0],), path=R.PATH_SORT)
        one_unsorted = R.deal(R.gen_records(62, 90), 3, natural=False)
        one_unsorted[1] = R.deal(R.gen_records(62, 90), 3)[1]
        check_engine(e, one_unsorted, (MODES[1],), path=R.PATH_WALK)
    finally:
        e.close()
    argv, want = run_files(tmp_path, files, ("-s",))
    assert want[1] == b""


def test_sorted_inputs_with_ties_are_stable(eng, tmp_path):
    """equal keys inside a file and across files, on sorted inputs: (file list order, line order), byte
    for byte against the stable restatement, in every mode"""
    rnd = random.Random(8)
    for natural in (False, True):
        files = []
        for f in range(4):
            lines = [rec(rnd.choice((b"1", b"01", b"chr1", b"Chr1", b"X")), rnd.choice((b"5", b"05", b"6", b"+6")), b";f%d_%d" % (f, i))
                     for i in range(60)]
            lines.sort(key=lambda l: R.sort_key(*R.parse(l)[1:], natural))
            files.append(R.HDR + b"".join(l + b"\n" for l in lines))
        res = check_engine(eng, files, [(False, natural), (True, natural)], path=R.PATH_SORT)
        assert all(m.ties for m in res) and res[0].order == res[1].order
        run_files(tmp_path, files, ("-s",) + (("-n",) if natural else ()), tag="n%d" % natural)


def test_a_run_of_five_thousand_equal_keys(eng):
    files = [R.HDR + b"".join(rec(b"1", b"5", b";a%d" % i) + b"\n" for i in range(2000)),
             b"".join(rec(b"1", b"05", b";b%d" % i) + b"\n" for i in range(1500)) + rec(b"1", b"4") + b"\n",
             rec(b"0", b"9") + b"\n" + b"".join(rec(b"1", b"+5", b";c%d" % i) + b"\n" for i in range(1500))]
    res = check_engine(eng, files, MODES[:2])
    assert res[0].path == R.PATH_SORT and res[1].path == R.PATH_WALK  # (file 2 is out of order)
    run = res[0].order[4:5004]  # (after the two header lines, 0:9 and 1:4) file after file, each in line order
    assert run == sorted(run) and len(set(run)) == 5000 and all(k == (b"1", 5) for k in res[0].keys[2:5002])


def test_cohort_file_dealt_into_three(eng):
    """a generated 2,504-sample file's records dealt into three files: the merged data lines are the
    original's, under both modes"""
    buf = synth.generate(300, 2504, 20251226)
    lines = buf.split(b"\n")[:-1]
    head = [l for l in lines if l[:1] == b"#"]
    data = [l for l in lines if l[:1] != b"#"]
    assert len(data) == 300
    keys = [R.sort_key(*R.parse(l)[1:], False) for l in data]
    assert len(set(keys)) == len(keys)
    files = [b"".join(l + b"\n" for l in head + data[k::3]) for k in range(3)]
    for m in check_engine(eng, files, MODES[:2]):
        got = m.text.split(b"\n")[:-1]
        assert got[:len(head)] == head and sorted(got[len(head):]) == sorted(data)
        if keys == sorted(keys):  # the records ascend: the merged text is the original
            assert m.text == buf and m.path == R.PATH_SORT


def _run_bin(argv, env=None):
    r = subprocess.run(argv, executable=BIN, input=b"", capture_output=True, timeout=120, env=dict(os.environ, **(env or {})))
    return r.stdout, r.stderr, r.returncode


def test_bad_line_warnings_per_file_and_ngpu(tmp_path):
    """one warning per malformed line, file after file, with the open failures in their places; the
    same bytes with VCFX_NGPU=2 (one order over all records does not shard)"""
    files = R.deal(R.gen_records(91, 300), 3)
    bad = [b"no tabs at all", b"1\t", b"1\tx\t.", b"1\t9223372036854775808\t."]
    files[0] += b"".join(l + b"\n" for l in bad[:3])
    files[2] = b"".join(l + b"\n" for l in bad) + files[2] + bad[0]
    paths = []
    for i, f in enumerate(files):
        p = tmp_path / ("w%d.vcf" % i)
        p.write_bytes(f)
        paths.append(str(p))
    missing = str(tmp_path / "missing.vcf")
    argv = [TOOL, "-m", ",".join([paths[0], missing, paths[1], paths[2]])]
    want = R.run(argv)
    warn = [b"Warning: skipping malformed line in " + p.encode() + b"\n" for p in paths]
    assert want[1] == warn[0] * 3 + b"Failed to open file: " + missing.encode() + b"\n" + warn[2] * 5
    assert tools.run(argv, b"") == want
    assert tools.shard_plan(argv, 2)[0] == 1
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": "2"}) == want
    quiet = R.run(argv + ["-s"])
    assert quiet[1] == b"Failed to open file: " + missing.encode() + b"\n"
    assert _run_bin(argv + ["-s"], env={"VCFX_NGPU": "2"}) == quiet
