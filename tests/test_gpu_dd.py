"""GPU parity of VCFX_duplicate_remover, byte for byte: every golden case of the compiled reference
(tests/golden/duplicate_remover_cases.json.gz) through the in-process drop-in and the executable;
constructed and generated inputs in both modes against the plain-Python restatement
(tests/_duplicate_remover_ref.py, itself held to the goldens by tests/test_duplicate_remover_ref.py):
the edges of the lane path's head window, kilobyte fields, ALT token counts, every POS form, line
counts around the kernels' and the sort's tiles, one long run, hash collisions forced through the
raw ABI, line mixes, wide records, BGZF input, VCFX_NGPU=2 and a vcfx_pipe chain."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _duplicate_remover_ref as R
from tests._golden import REPO
from vcfx_amd import engine, synth, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
PIPE = os.path.join(REPO, "build", "bin", "vcfx_pipe")
CASES = R.load_cases()
W = R.WINDOW
MODES = ((engine.MODE_FILE, False), (engine.MODE_STDIN, True))


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


def both_modes(buf, tmp_path, tag="", extra=()):
    """the drop-in in file mode and stdin mode against the restatement"""
    path = tmp_path / ("in%s.vcf" % tag)
    path.write_bytes(buf)
    for argv, stdin in (([TOOL, "-i", str(path)] + list(extra), b""), ([TOOL] + list(extra), buf)):
        got, want = tools.run(argv, stdin), R.run(argv, stdin)
        assert got[2] == want[2] and got[1] == want[1], (argv[1:2], tag)
        assert got[0] == want[0], (argv[1:2], tag, len(got[0]), len(want[0]))


def lane_path(line):
    """the line is settled by the key kernel's lane pass: its ALT ends inside the first W bytes and
    its POS is 1..9 digits from the field's first byte (else the wave takes it)"""
    if not line or line[:1] == b"#":
        return True
    t = R.tab_offsets(line, 0, min(len(line), W))
    if len(t) < 5 and len(line) > W:
        return False
    if len(t) < 4:
        return True  # a short line
    pos = line[t[0] + 1:t[1]]
    d = len(pos) - len(pos.lstrip(b"0123456789"))
    return 1 <= d <= 9


def check_engine(eng, buf, hash_bits=0):
    """statuses, summary and counts of the raw ABI in both modes; returns the wave-path lines"""
    spans = R.line_spans(buf)
    wave = sum(not lane_path(buf[a:b]) for a, b in spans)
    eng.load(buf)
    assert eng.index(0) == len(spans)
    for mode, stdin in MODES:
        want = R.statuses(buf, stdin)[0]
        s, st, cnt = eng.dedup(mode, hash_bits)
        assert st.tolist() == want, (stdin, hash_bits, [i for i, (a, b) in enumerate(zip(st.tolist(), want)) if a != b][:10])
        assert cnt[:5] == tuple(want.count(k) for k in range(5))
        assert cnt[5] == s.general_records == wave
        assert (s.n_lines, s.rows, s.data_lines, s.warn_lines) == \
            (len(want), want.count(R.KEPT), want.count(R.KEPT) + want.count(R.DUP), want.count(R.SHORT))
    return wave


def test_golden_fixtures_per_line(eng):
    """every fixture through the raw ABI: per-line statuses; the POS fixtures' irregular forms take
    the wave path"""
    d = os.path.join(R.GOLDEN, "duplicate_remover")
    waves = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            buf = f.read()
        if buf:
            waves[name] = check_engine(eng, buf)
    assert waves["pos_forms.vcf"] >= 25 and waves["pos_scan.vcf"] >= 8 and waves["one_line.vcf"] == 0


def test_head_window_edges(eng, tmp_path):
    """the fifth tab at byte W - 1, W and W + 1 of the line, the line's end there without a fifth
    tab, the first tab past W; each such line between lines of the same key on the other path"""
    lines = []
    for k, at in enumerate((W - 2, W - 1, W, W + 1, W + 40)):
        key = [b"%d" % k, b"100", b"A", b"C,G"]
        lines.append(R.record(key[0], key[1], b".", key[2], b"G,C"))
        bare = b"\t".join([key[0], key[1], b"", key[2], key[3], b"rest"])
        lines.append(bare.replace(b"\t\t", b"\t" + b"i" * (at - bare.index(b"\trest")) + b"\t"))
        assert lines[-1].index(b"\trest") == at
        lines.append(R.record(key[0], key[1], b"again", key[2], key[3]))
        # ALT runs to the line's end, which is byte `at`
        bare = b"\t".join([b"e%d" % k, b"7", b"", b"T", b"A"])
        lines.append(bare.replace(b"\t\t", b"\t" + b"j" * (at - len(bare)) + b"\t"))
        assert len(lines[-1]) == at
        lines.append(R.record(b"e%d" % k, b"7", b".", b"T", b"A"))
    far = b"c" * (W + 6)
    lines += [R.record(far, b"5", b".", b"A", b"T"), R.record(far, b"5", b"x", b"A", b"T"), R.record(far[:-1], b"5", b".", b"A", b"T"),
              R.record(b"1", b"5", b"y" * (2 * W), b"A", b"T"), b"1\t5\t" + b"z" * (3 * W) + b"\tA", b"1\t5\tq\tA\tT"]
    buf = R.HDR + b"\n".join(lines) + b"\n"
    wave = check_engine(eng, buf)
    assert wave == sum(not lane_path(x) for x in lines) and 8 <= wave <= len(lines) - 8
    both_modes(buf, tmp_path)


def test_long_fields(eng, tmp_path):
    """a 5,000-byte REF and a 5,000-byte ALT; two such lines equal but for ALT order, two that
    differ in the last byte of REF, of ALT"""
    rnd = random.Random(5)
    ref = bytes(rnd.choice(b"ACGT") for _ in range(5000))
    toks = [bytes(rnd.choice(b"ACGT") for _ in range(999)) for _ in range(5)]
    alt = b",".join(toks)
    assert len(alt) == 4999
    lines = [R.record(b"1", b"9", b"a", ref, alt),
             R.record(b"1", b"9", b"b", ref, b",".join(toks[::-1])),
             R.record(b"1", b"9", b"c", ref[:-1] + b"N", alt),
             R.record(b"1", b"9", b"d", ref, alt[:-1] + b"N"),
             R.record(b"1", b"9", b"e", ref, b",".join(toks[1:] + toks[:1])),
             R.record(b"1", b"9", b"f", ref[:-1] + b"N", b",".join(toks[2:] + toks[:2])),
             R.record(b"1", b"9", b"g", ref, b",".join(toks[:4] + [toks[3]])),
             R.record(b"1", b"9", b"h", ref, b"<" + alt.replace(b",", b"x") + b">"),
             R.record(b"1", b"9", b"i", ref, b"<" + alt.replace(b",", b"x") + b">")]
    buf = R.HDR + b"\n".join(lines) + b"\n"
    assert R.statuses(buf, False)[0][2:] == [R.KEPT, R.DUP, R.KEPT, R.KEPT, R.DUP, R.DUP, R.KEPT, R.KEPT, R.DUP]
    assert check_engine(eng, buf) == len(lines)
    both_modes(buf, tmp_path)


@pytest.mark.parametrize("count", [1, 2, 3, 8, 9, 40])
def test_alt_token_counts(eng, count, tmp_path):
    """`count` ALT tokens permuted, one token changed, one token twice; short lines (lane path) and
    the same keys behind a long ID (wave path)"""
    rnd = random.Random(count)
    toks = [b"%s%d" % (rnd.choice((b"A", b"C", b"G", b"T")), i) for i in range(count)]
    lines = []
    other = toks[:]
    other[rnd.randrange(count)] += b"x"
    twice = toks[:-1] + toks[:1] if count > 1 else toks + toks
    for pad in (b".", b"p" * (2 * W)):
        for k in range(4):
            perm = toks[:]
            rnd.shuffle(perm)
            lines.append(R.record(b"1", b"5", pad, b"A", b",".join(perm)))
        lines += [R.record(b"1", b"5", pad, b"A", b",".join(other)), R.record(b"1", b"5", pad, b"A", b",".join(twice)),
                  R.record(b"1", b"5", pad, b"A", b",".join(twice[::-1]))]
    buf = R.HDR + b"\n".join(lines) + b"\n"
    want = R.statuses(buf, False)[0][2:]
    assert want[:7] == [R.KEPT, R.DUP, R.DUP, R.DUP, R.KEPT, R.KEPT, R.DUP] and want.count(R.KEPT) == 3
    check_engine(eng, buf)
    both_modes(buf, tmp_path)


def test_repeated_and_empty_tokens(eng, tmp_path):
    """A,A,C against A,C,C; empty tokens count in stdin mode only"""
    alts = [b"A,A,C", b"A,C,C", b"C,A,A", b"C,A,C", b"A,C", b"G,,C", b"G,C,", b"C,G", b",,G,C", b"", b",", b"G,,C"]
    lines = [R.record(b"1", b"5", b"%d" % i, b"A", a) for i, a in enumerate(alts)]
    lines += [b"\t".join([b"1", b"5", b"w" * (2 * W), b"A", a]) for a in alts]
    buf = R.HDR + b"\n".join(lines) + b"\n"
    k, d = R.KEPT, R.DUP
    assert R.statuses(buf, True)[0][2:14] == [k, k, d, d, k, k, d, k, k, k, k, d]
    assert R.statuses(buf, False)[0][2:14] == [k, k, d, d, k, k, d, d, d, k, d, d]
    check_engine(eng, buf)
    both_modes(buf, tmp_path)


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_data_lines(eng, n, tmp_path):
    for tail in (b"\n", b""):
        for second in (b"1\t5\tx\tA\tC,G", b"1\t5\tx\tA\tG,C", b"1\t6\tx\tA\tG,C"):
            buf = b"1\t5\t.\tA\tG,C" + (b"\n" + second if n == 2 else b"") + tail
            check_engine(eng, buf)
            both_modes(buf, tmp_path)


@pytest.mark.parametrize("name", ["n255", "n256", "n257", "n4097"])
def test_line_counts_at_the_tile_edges(eng, name, tmp_path):
    buf = R.generated(name)
    check_engine(eng, buf)
    both_modes(buf, tmp_path, name)


def test_one_long_run(eng, tmp_path):
    """5,000 lines of one key (every second one with other bytes after ALT): only the first survives"""
    lines = [R.record(b"7", b"123", b"id%d" % i, b"AC", b"T,G" if i % 2 else b"G,T", b"q%d" % i) for i in range(5000)]
    buf = b"\n".join(lines) + b"\n"
    check_engine(eng, buf)
    out, err, rc = tools.run([TOOL], buf)
    assert (out, err, rc) == (lines[0] + b"\n", b"", 0)


@pytest.mark.parametrize("hash_bits", [1, 2, 4, 0])
def test_forced_collisions(eng, hash_bits):
    """the hash cut to 1, 2 and 4 bits puts every data line into one of 2, 4 and 16 runs: the verify
    pass resolves the collisions in line order; the statuses do not depend on the hash"""
    buf = R.generated("g600")
    check_engine(eng, buf, hash_bits)
    check_engine(eng, R.generated("mix"), hash_bits)


@pytest.mark.parametrize("name", ["mix", "mix_crlf", "mix_no_final_newline"])
def test_line_mixes(eng, name, tmp_path):
    """'#' and empty lines between the data lines, lines of fewer than four tabs with and without
    -q, CRLF, no final newline"""
    buf = R.generated(name)
    st = R.statuses(buf, False)[0]
    # (with CRLF an empty line is "\\r": no tab, so SHORT)
    assert min(st.count(k) for k in (R.HEADER, R.SHORT, R.KEPT, R.DUP) + ((R.EMPTY,) if name != "mix_crlf" else ())) >= 5
    check_engine(eng, buf)
    both_modes(buf, tmp_path, name)
    both_modes(buf, tmp_path, name, extra=("-q",))
    out, err, rc = tools.run([TOOL], buf)
    assert err == R.WARN * R.statuses(buf, True)[0].count(R.SHORT) and rc == 0
    assert tools.run([TOOL, "--quiet"], buf) == (out, b"", 0)


def test_wide_records(eng, tmp_path):
    """300 lines x 2,504 samples, every third one repeated later under a new ID with its sample
    columns cut short: the sample bytes do not matter and are not needed"""
    buf = synth.generate(300, 2504, 11)
    k = buf.index(b"\n#CHROM") + 1
    k = buf.index(b"\n", k) + 1
    head, recs = buf[:k], buf[k:].split(b"\n")[:-1]
    assert len(recs) == 300 and min(len(r) for r in recs) > 5000
    extra = []
    for i, r in enumerate(recs[::3]):
        f = r.split(b"\t")
        f[2] = b"again%d" % i
        extra.append(b"\t".join(f[:9 + (i % 7)]))
    rnd = random.Random(3)
    lines = recs + extra
    rnd.shuffle(lines)
    buf = head + b"\n".join(lines) + b"\n"
    st = R.statuses(buf, False)[0]
    assert st.count(R.DUP) == 100 and st.count(R.KEPT) == 300
    check_engine(eng, buf)
    both_modes(buf, tmp_path)


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
    want = R.run([TOOL, "-i", str(plain)])
    assert want[0].count(b"\n") > 500 and want[1]
    assert tools.run([TOOL, "-i", str(plain)]) == want
    assert tools.run([TOOL, "-i", str(comp)]) == want
    # inflated on the device (the host then fetches the written lines from there)
    assert _run_bin([TOOL, str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1"}) == want
    # ... through a read-back window that moves many times
    assert _run_bin([TOOL, str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1", "VCFX_WINDOW_BYTES": "1024"}) == want


def test_ngpu_gives_the_unsharded_bytes(tmp_path):
    buf = R.generated("routes")
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    argv = [TOOL, "-i", str(path)]
    assert tools.shard_plan(argv, 2)[0] == 1
    want = R.run(argv)
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": "2"}) == want


def test_pipe_chain_starting_with_the_tool():
    """vcfx_pipe 'VCFX_duplicate_remover | VCFX_variant_counter' against the counter on the
    restatement's output"""
    buf = R.generated("routes")
    kept = R.run([TOOL, "-q"], buf)[0]
    want = tools.run(["VCFX_variant_counter"], kept)
    assert want[2] == 0 and want[0]
    r = subprocess.run([PIPE, "%s -q | VCFX_variant_counter" % TOOL], input=buf, capture_output=True, timeout=120)
    assert (r.stdout, r.returncode) == (want[0], 0)
    assert str(R.statuses(buf, True)[0].count(R.KEPT)).encode() in r.stdout


def test_status_call_needs_a_dedup(eng):
    eng.load(b"1\t5\t.\tA\tC\n")
    eng.index(0)
    st = np.zeros(1, np.uint8)
    assert eng.L.vcfxg_dedup_status(eng.h, 0, 1, st.ctypes.data) == -5  # VCFXG_E_STATE: no dedup on this index
    eng.dedup(engine.MODE_FILE)
    assert eng.L.vcfxg_dedup_status(eng.h, 0, 1, st.ctypes.data) == 0 and st[0] == R.KEPT
    assert eng.L.vcfxg_dedup_status(eng.h, 1, 1, st.ctypes.data) == -3  # VCFXG_E_ARG
