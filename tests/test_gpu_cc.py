"""GPU parity of VCFX_cross_sample_concordance, byte for byte: every golden case of the compiled
reference (tests/golden/concordance_cases.json.gz) through the in-process drop-in and the
executable; generated inputs in both modes against the plain-Python restatement
(tests/_concordance_ref.py, itself held to the goldens by tests/test_concordance_ref.py) at the
sample counts around the wave width and a wave step (256 fixed-stride samples a step); the digit
pairs under every ALT count, '.' in either slot, records whose distinct keys overflow 64 bits,
mixed separators, GT:AD:DP, repeated '#CHROM' lines and -s subsets; the file mode's row order
for every T; the raw ABI's summary, totals and per-line values; BGZF input; a vcfx_pipe chain;
VCFX_NGPU=2; the schedule knobs."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _concordance_ref as R
from tests._golden import REPO
from vcfx_amd import engine, synth, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
PIPE = os.path.join(REPO, "build", "bin", "vcfx_pipe")
CASES = R.load_cases()
NS = [1, 2, 63, 64, 65, 130, 255, 256, 257, 600]


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


def both_modes(buf, tmp_path, tag="", extra=(), threads=("1", "3")):
    """the drop-in in file mode (at each T) and stdin mode against the restatement"""
    path = tmp_path / ("in%s.vcf" % tag)
    path.write_bytes(buf)
    runs = [([TOOL, "-t", t, "-i", str(path)] + list(extra), b"") for t in threads] + [([TOOL] + list(extra), buf)]
    for argv, stdin in runs:
        got, want = tools.run(argv, stdin), R.run(argv, stdin)
        assert got[2] == want[2] and got[1] == want[1], (argv[1:3], tag)
        assert got[0] == want[0], (argv[1:3], tag, len(got[0]), len(want[0]))


@pytest.mark.parametrize("ns", NS)
def test_ragged_inputs_match_restatement(ns, tmp_path):
    """the traps of parseGenotypeToId in every column, ragged and over-wide lines, a trailing tab,
    empty CHROM and ALT, '#' and empty lines, with and without '\\r' and a final newline"""
    for k, (crlf, fin) in enumerate([(False, True), (True, True), (False, False), (True, False)]):
        both_modes(R.ragged_vcf(100 * ns + k, 90, ns, crlf=crlf, final_newline=fin), tmp_path, "r%d" % k)


@pytest.mark.parametrize("ns", NS)
def test_fixed_stride_inputs_match_restatement(ns, tmp_path):
    """one-digit alleles and one separator per record (the last sample has no tab after it; the
    last record no newline), without and with missing calls, up to nine ALT alleles"""
    both_modes(R.clean_vcf(ns, 120, ns, max_alt=1), tmp_path, "a")
    both_modes(R.clean_vcf(ns + 1, 120, ns, missing=0.02, max_alt=3)[:-1], tmp_path, "b")
    both_modes(R.clean_vcf(ns + 2, 60, ns, missing=0.001, max_alt=9), tmp_path, "c")


@pytest.mark.parametrize("phased", [False, True])
def test_every_digit_pair_under_each_alt_count(phased, tmp_path):
    """a record per ALT count 0, 1, 2, 5, 9 holding all 100 digit pairs and '.' in either slot:
    validity depends on the larger allele alone"""
    sep = b"|" if phased else b"/"
    pairs = [b"%d%s%d" % (a, sep, b) for a in range(10) for b in range(10)]
    pairs += [b"." + sep + b"1", b"1" + sep + b".", b"." + sep + b"."]
    out = [R.header(len(pairs))]
    for r, na in enumerate([0, 1, 2, 5, 9]):
        out.append(R.record(10 + r, pairs, alt=R.alt_of(na)) + b"\n")
        out.append(R.record(20 + r, pairs[::-1], alt=R.alt_of(na)) + b"\n")
    buf = b"".join(out)
    both_modes(buf, tmp_path)
    want = R.file_mode(buf, set(), 1, True)[0]
    rows = want.split(b"\n")[1:-1]
    assert [int(x.split(b"\t")[6]) for x in rows[::2]] == [1, 3, 6, 21, 55]
    eng = _engine(WALK)  # (412-byte records: the walk only when forced)
    try:
        eng.load(buf)
        s, totals, text = eng.concordance(R.region_file(buf)[0], engine.MODE_FILE, n_samples=len(pairs), threads=1)
        assert R.HEADER + text == want
        assert eng.L.vcfxg_last_schedule(eng.h) == b"cc_walk" and s.general_records == 0
    finally:
        eng.close()


def test_more_than_64_distinct_keys(tmp_path):
    """257 samples carrying the 276 pairs over alleles 0..22 (a 64-bit key set overflows), and a
    record of 136 samples all distinct (file mode takes the short record, stdin mode skips it)"""
    p22 = [b"%d/%d" % (a, b) for a in range(23) for b in range(a, 23)]
    p15 = [b"%d|%d" % (b, a) for a in range(16) for b in range(a, 16)]
    assert len(p22) == 276 and len(p15) == 136
    alt = b",".join([b"T"] * 22)
    buf = R.header(257) + R.record(1, p22[:257], alt=alt) + b"\n" + R.record(2, p22[19:276], alt=alt) + b"\n" + \
        R.record(3, (p15 + p15)[:257], alt=alt) + b"\n" + R.record(4, p15, alt=alt) + b"\n"
    rows = R.file_mode(buf, set(), 1, True)[0].split(b"\n")[1:-1]
    nu = [tuple(int(v) for v in x.split(b"\t")[5:7]) for x in rows]
    assert nu == [(257, 257), (257, 257), (257, 136), (136, 136)]
    assert R.stdin_mode(buf, set(), True)[0].split(b"\n")[1:-1] == rows[:3]
    both_modes(buf, tmp_path)


def test_mixed_separators_and_gt_ad_dp(tmp_path):
    ns = 130
    rnd = np.random.RandomState(5)
    out = [R.header(ns)]
    for r in range(40):
        f = [b"%d%s%d" % (rnd.randint(2), b"/|"[rnd.randint(2):][:1], rnd.randint(2)) for _ in range(ns)]
        out.append(R.record(r, f) + b"\n")
        g = [x + b":%d,%d:%d" % (rnd.randint(40), rnd.randint(40), rnd.randint(99)) for x in f]
        out.append(R.record(100 + r, g, fmt=b"GT:AD:DP") + b"\n")
    both_modes(b"".join(out), tmp_path)
    both_modes(synth.generate(150, 257, 74, 0, 0.002, 0, 0.0, 0, format_mode=1), tmp_path, "synth")


def test_repeated_chrom_lines_and_subsets(tmp_path):
    """a second identical '#CHROM' line doubles N and not U (file mode; stdin takes the first);
    -s picking the first, the last, every second sample and none"""
    ns = 65
    buf = R.clean_vcf(8, 80, ns, missing=0.05, max_alt=2)
    lines = buf.split(b"\n")
    twice = b"\n".join(lines[:2] + [lines[1]] + lines[2:])
    apart = b"\n".join(lines[:30] + [b"\t".join([R.HDR9] + R.names(9))] + lines[30:])
    nm = [x.decode() for x in R.names(ns)]
    for tag, data in (("once", buf), ("twice", twice), ("apart", apart)):
        both_modes(data, tmp_path, tag)
        for sel in (nm[0], nm[-1], ",".join(nm[::2]), "nobody", nm[3] + "," + nm[3]):
            both_modes(data, tmp_path, tag, extra=("-s", sel), threads=("2",))
    one = tools.run([TOOL, "-q", "-t", "1", "-i", str(tmp_path / "inonce.vcf")])[0].split(b"\n")[1:-1]
    two = tools.run([TOOL, "-q", "-t", "1", "-i", str(tmp_path / "intwice.vcf")])[0].split(b"\n")[1:-1]
    assert len(one) == len(two) == 80
    for a, b in zip(one, two):
        fa, fb = a.split(b"\t"), b.split(b"\t")
        assert int(fb[5]) == 2 * int(fa[5]) and fb[6] == fa[6]


def test_cohort_with_missing_calls(tmp_path):
    """2,504 samples, 0.1 % missing calls: about 10 KB a record"""
    both_modes(synth.generate(200, 2504, 75, 0, 0.001, 0, 0.0, 0), tmp_path, threads=("7",))


def order_input(n, seed):
    """n collected data lines over 3 samples, some of which give no row (under five fields, an
    empty CHROM), '#' and empty lines among them (these do not count)"""
    rnd = np.random.RandomState(seed)
    out = [R.header(3)]
    for k in range(n):
        x = rnd.rand()
        if x < 0.1:
            out.append(b"1\t%d\t.\tA\n" % k)
        elif x < 0.15:
            out.append(R.record(k, [b"0/1"] * 3, chrom=b"") + b"\n")
        else:
            out.append(R.record(k, [b"%d/%d" % (rnd.randint(2), rnd.randint(2)) for _ in range(3)]) + b"\n")
        if rnd.rand() < 0.1:
            out.append(rnd.choice([b"\n", b"#x\n", b"\r\n"]))
    return b"".join(out)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_row_order_for_every_worker_count(n, tmp_path):
    buf = order_input(n, n)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    seen = set()
    for t in (1, 2, 3, 7, 64, n, n + 1):
        argv = [TOOL, "-t", str(t), "-i", str(path)]
        got = tools.run(argv)
        assert got == R.run(argv), (n, t)
        seen.add(got[0])
    if n >= 63:
        assert len(seen) >= 4  # T = 2, 3, 7 each give an order of their own; T = 1 and T >= n record order


def test_default_worker_count_is_the_hosts(tmp_path):
    """without -t the order is that of hardware_concurrency() workers: the run reports its T"""
    buf = order_input(300, 3)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    got = tools.run([TOOL, "-i", str(path)])
    t = int(re.search(rb"Threads used: (\d+)\n", got[1]).group(1))
    assert 1 <= t <= 300
    assert got == R.run([TOOL, "-i", str(path)], default_threads=t)
    assert got == R.run([TOOL, "-t", str(t), "-i", str(path)])


@pytest.mark.parametrize("walk", [False, True])
@pytest.mark.parametrize("mode", [engine.MODE_FILE, engine.MODE_STDIN])
def test_raw_abi_summary_totals_and_lines(mode, walk):
    ns = 65
    buf = R.ragged_vcf(77, 300, ns, crlf=True)
    lines = buf.split(b"\n")
    lines.insert(120, b"\t".join([R.HDR9] + R.names(ns)[:40]) + b"\r")
    buf = b"\n".join(lines)
    eng = _engine(WALK if walk else {"VCFXG_AF_FUSED": "8"})
    try:
        eng.load(buf)
        if mode == engine.MODE_FILE:
            ds, mult, per, nd = R.region_file(buf)
            assert max(mult) == 2
            assert eng.chrom_lines(ds).tolist() == [buf.index(b"\n#CHROM", ds) + 1]
            for t in (0, 1, 5):
                s, totals, text = eng.concordance(ds, mode, mult=mult, threads=t)
                want = R.file_mode(buf, set(), t or 1, True)[0][len(R.HEADER):]
                assert text == want  # (T = 0 and T = 1 are both record order)
                check_lines(eng, s, totals, per, nd, len(text), walk)
            sub = [1 if i % 3 == 0 else 0 for i in range(ns)]
            ds, _, per, nd = R.region_file(buf.replace(lines[120], b"#x"), {b"S%d" % i for i in range(0, ns, 3)})
            eng.load(buf.replace(lines[120], b"#x"))
            s, totals, text = eng.concordance(ds, mode, mult=sub, threads=4)
            check_lines(eng, s, totals, per, nd, len(text), walk)
            s, totals, text = eng.concordance(ds, mode, mult=[], threads=4)
            assert totals[0] == totals[1] == 0 and totals[2] == s.rows > 0
        else:
            found, names, indices, rest = R.stdin_scan(buf, set())
            ds = buf.index(b"\n", buf.index(b"\n#CHROM") + 1) + 1
            per = [R.stdin_line(ln, len(names), indices)[1:] for ln in rest]
            nd = sum(1 for ln in rest if ln and ln[:1] != b"#")
            s, totals, text = eng.concordance(ds, mode, n_samples=ns)
            assert R.HEADER + text == R.stdin_mode(buf, set(), True)[0]
            check_lines(eng, s, totals, per, nd, len(text), walk)
        with pytest.raises(engine.EngineError):
            eng.concordance(ds, 2)
    finally:
        eng.close()


def check_lines(eng, s, totals, per, nd, text_bytes, walk=False):
    assert s.n_lines == len(per) and s.text_bytes == text_bytes and s.data_lines == nd
    n, u, st = eng.lines(s.n_lines)
    assert st.tolist() == [p[2] for p in per]
    rows = st != 0
    assert n[rows].tolist() == [p[0] for p in per if p[2]] and u[rows].tolist() == [p[1] for p in per if p[2]]
    assert totals == (sum(p[2] == R.CONCORDANT for p in per), sum(p[2] == R.DISCORDANT for p in per),
                      sum(p[2] == R.NO_GENOTYPES for p in per), nd)
    assert s.rows == int(rows.sum())
    if walk:  # only what the walk left
        assert s.general_records <= nd
    else:  # every data line takes the per-line kernel
        assert s.general_records == nd and eng.L.vcfxg_last_schedule(eng.h) == b"cc_two_sweep"


def _run_bin(argv, stdin=b"", env=None):
    r = subprocess.run(argv, executable=BIN, input=stdin, capture_output=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    return r.stdout, r.stderr, r.returncode


def _engine(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return engine.Engine(0)  # (a fresh context reads the knobs)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


WALK = {"VCFXG_AF_FUSED": "7", "VCFXG_WALK_CHUNK": "4096"}  # records straddle the 4 KiB chunks


@pytest.mark.parametrize("fused", ["3", "7", "8"])
def test_each_schedule_at_every_sample_count(fused, tmp_path):
    """the walk (7) and the two-sweep schedules (3, 8) forced, with 4 KiB walker chunks, on clean
    and ragged inputs at every sample count, both modes (a process each: the knobs are read when
    the context opens)"""
    env = {"VCFXG_AF_FUSED": fused, "VCFXG_WALK_CHUNK": "4096"}
    runs = []
    for ns in NS:
        for tag, buf in (("c", R.clean_vcf(40 + ns, 60, ns, missing=0.01, max_alt=2)),
                         ("r", R.ragged_vcf(50 + ns, 60, ns, crlf=ns % 2 == 1))):
            path = tmp_path / ("%s%d.vcf" % (tag, ns))
            path.write_bytes(buf)
            runs.append(([TOOL, "-t", "5", "-i", str(path)], b""))
            if tag == "c":
                runs.append(([TOOL, "-q"], buf))
    with ThreadPoolExecutor(12) as ex:
        got = list(ex.map(lambda r: _run_bin(r[0], r[1], env), runs))
    for (argv, stdin), g in zip(runs, got):
        assert g == R.run(argv, stdin), (fused, argv[1:])


@pytest.mark.parametrize("ns", [1, 64, 130, 257, 600])
def test_walk_takes_clean_records_itself(ns):
    """on the walk schedule a clean fixed-stride input leaves nothing to the per-line kernel
    (general_records == 0), in both modes and with an all-ones multiplicity array; a record with
    another sample count, mixed separators or a multi-digit allele is left to it"""
    buf = R.clean_vcf(60 + ns, 150, ns, missing=0.01, max_alt=9)
    ds, mult, per, nd = R.region_file(buf)
    assert mult == [1] * ns and nd == 150
    found, names, indices, rest = R.stdin_scan(buf, set())
    per_stdin = [R.stdin_line(ln, len(names), indices)[1:] for ln in rest]
    eng = _engine(WALK)
    try:
        eng.load(buf)
        for kw in ({"n_samples": ns}, {"mult": mult}):
            s, totals, text = eng.concordance(ds, engine.MODE_FILE, threads=3, **kw)
            assert eng.L.vcfxg_last_schedule(eng.h) == b"cc_walk"
            assert R.HEADER + text == R.file_mode(buf, set(), 3, True)[0]
            check_lines(eng, s, totals, per, nd, len(text), walk=True)
            assert s.general_records == 0
        s, totals, text = eng.concordance(ds, engine.MODE_STDIN, n_samples=ns)
        assert R.HEADER + text == R.stdin_mode(buf, set(), True)[0]
        check_lines(eng, s, totals, per_stdin, nd, len(text), walk=True)
        assert s.general_records == 0
        # a subset or a doubled column: not the walk
        eng.concordance(ds, engine.MODE_FILE, mult=[2] * ns, threads=3)
        assert eng.L.vcfxg_last_schedule(eng.h) == b"cc_two_sweep"
        # three records the fixed-stride sweep must not take
        lines = buf.split(b"\n")
        odd = [R.record(7, [b"0/1"] * (ns + 1)), R.record(8, [b"0/1"] * (ns - 1) + [b"0|1"]) if ns > 1 else
               R.record(8, [b"0/1", b"1/1"]), R.record(9, [b"10/1"] + [b"0/1"] * (ns - 1), alt=R.alt_of(10))]
        buf2 = b"\n".join(lines[:40] + odd + lines[40:])
        ds, mult, per, nd = R.region_file(buf2)
        eng.load(buf2)
        s, totals, text = eng.concordance(ds, engine.MODE_FILE, n_samples=ns, threads=2)
        assert R.HEADER + text == R.file_mode(buf2, set(), 2, True)[0]
        check_lines(eng, s, totals, per, nd, len(text), walk=True)
        assert s.general_records == 3
    finally:
        eng.close()


def test_bgzf_input_gives_the_plain_output(tmp_path):
    from tests import _bgzf
    buf = R.ragged_vcf(9, 400, 65)
    plain, comp = tmp_path / "in.vcf", tmp_path / "in.vcf.gz"
    plain.write_bytes(buf)
    comp.write_bytes(_bgzf.bgzf(buf))
    want = R.run([TOOL, "-t", "3", "-i", str(plain)])
    assert tools.run([TOOL, "-t", "3", "-i", str(plain)]) == want
    assert tools.run([TOOL, "-t", "3", "-i", str(comp)]) == want
    # inflated on the device (the host then fetches nothing but header lines)
    assert _run_bin([TOOL, "-t", "3", str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1"}) == want


def test_ngpu_gives_the_unsharded_bytes(tmp_path):
    buf = R.ragged_vcf(11, 700, 20, crlf=True)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    argv = [TOOL, "-t", "6", "-i", str(path)]
    assert tools.shard_plan(argv, 2)[0] == 1  # the row order spans the file: one context
    want = R.run(argv)
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": "2"}) == want


def test_pipe_chain_ending_in_the_tool():
    """vcfx_pipe 'VCFX_nonref_filter | VCFX_cross_sample_concordance' against the restatement on
    the filter's output"""
    buf = synth.generate(400, 130, 73, 0, 0.01, 0, 0.1, 0)
    kept = tools.run(["VCFX_nonref_filter"], buf)
    assert kept[2] == 0 and kept[0].count(b"\n") > 100
    want = R.run([TOOL, "-q"], kept[0])
    r = subprocess.run([PIPE, "VCFX_nonref_filter | %s -q" % TOOL], input=buf, capture_output=True, timeout=120)
    assert (r.stdout, r.returncode) == (want[0], 0)
    assert len(want[0].split(b"\n")) > 100
