"""GPU parity of VCFX_sample_extractor, byte for byte: every golden case of the compiled
reference (tests/golden/sample_extractor_cases.json.gz) through the in-process drop-in and the
executable; generated inputs in both modes against the plain-Python restatement
(tests/_sample_extractor_ref.py, itself held to the goldens by tests/test_sample_extractor_ref.py)
at the shapes where the kernel can go wrong -- sample counts around the wave width, line lengths
around a wave step (1 KiB) and around 16 B, kept fields that straddle a lane's window or a step,
lines wider than the kernel's staging ring, ragged lines, CRLF, no final newline, blocks of one
line; the raw ABI's summary and statuses; BGZF input; VCFX_NGPU=2 and 3; a vcfx_pipe chain."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import _sample_extractor_ref as R
from tests._golden import REPO
from tests._sample_extractor_cases import GOLDEN, case_stdin, load_cases
from vcfx_amd import engine, synth, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
PIPE = os.path.join(REPO, "build", "bin", "vcfx_pipe")
CASES = load_cases()
SX_STAGE = 2048  # kSxStage (vcfxg_sx.hip): the per-wave staging ring a line passes through
WAVE_STEP = 1024


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_in_process(case):
    out, err, rc = tools.run(case["argv"], case_stdin(case), cwd=GOLDEN)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_golden_binary():
    """the executable on every golden case (a process each, twelve at a time; argv[0] is the
    tool's name, as recorded, so that getopt's messages match)"""
    assert os.access(BIN, os.X_OK)

    def one(case):
        r = subprocess.run(case["argv"], executable=BIN, input=case_stdin(case), capture_output=True, cwd=GOLDEN,
                           timeout=120)
        return (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])

    with ThreadPoolExecutor(12) as ex:
        ok = list(ex.map(one, CASES))
    assert all(ok), [c["name"] for c, v in zip(CASES, ok) if not v]


def both_modes(buf, sel, tmp_path, tag=""):
    """the drop-in in file and stdin mode against the restatement"""
    path = tmp_path / ("in%s.vcf" % tag)
    path.write_bytes(buf)
    for argv, stdin in (([TOOL, "-s", sel, "-i", str(path)], b""), ([TOOL, "-s", sel], buf)):
        got, want = tools.run(argv, stdin), R.run(argv, stdin)
        assert got[2] == want[2] and got[1] == want[1], (argv[1:3], tag)
        assert got[0] == want[0], (argv[1:3], tag, len(got[0]), len(want[0]))


def selections(ns):
    """kept sets over ns samples: the first and the last column, adjacent ones, every second,
    one in the middle, all, none found"""
    nm = [n.decode() for n in R.names(ns)]
    sels = {"first": nm[:1], "last": nm[-1:], "first_last": [nm[0], nm[-1]], "adjacent": nm[ns // 2:ns // 2 + 3],
            "every_second": nm[::2], "odd": nm[1::2], "all": nm, "none": ["nobody"], "some_missing": [nm[-1], "nobody"]}
    return {k: ",".join(v) for k, v in sels.items() if v}


@pytest.mark.parametrize("ns", [1, 2, 63, 64, 65, 130])
def test_ragged_inputs_match_restatement(ns, tmp_path):
    """ragged lines (6 fields and up, a trailing tab, extra columns), '#' and empty lines among
    them, with and without '\\r', with and without a final newline"""
    for k, (crlf, fin) in enumerate([(False, True), (True, True), (False, False), (True, False)]):
        buf = R.ragged_vcf(100 * ns + k, 120, ns, crlf=crlf, final_newline=fin)
        for tag, sel in selections(ns).items():
            both_modes(buf, sel, tmp_path, "%d_%s" % (k, tag))


def test_line_lengths_around_a_wave_step_and_16_bytes(tmp_path):
    """lines of 1023, 1024 and 1025 bytes (a wave's 16 B x 64 step), of 2047..2049, and of a
    multiple of 16 and one more and one less"""
    lengths = [1023, 1024, 1025, 2047, 2048, 2049, 1007, 1008, 1009, 2063, 2064, 2065, 3071, 3072, 3073]
    for ns in (65, 130):
        buf = R.sized_vcf(ns, lengths)
        assert [len(x) for x in buf.split(b"\n")[2:-1]] == lengths
        for tag, sel in selections(ns).items():
            both_modes(buf, sel, tmp_path, "%d_%s" % (ns, tag))


def test_kept_fields_straddle_a_lane_window_and_a_wave_step(tmp_path):
    """11-byte fields at every alignment: the kept column's bytes cross a lane's 16 B window in
    some lines and the wave's 1 KiB step in others (checked on the input's own offsets)"""
    ns, col = 130, 82  # (the field starts about 1,014 + k bytes into line k)
    out = [R.header(ns)]
    for k in range(64):
        out.append(R.record(k, [b"0/1:12,3:%02d" % (i % 100) for i in range(ns)], info=b"P" * (1 + k), fmt=b"GT:AD:DP")
                   + b"\n")
    buf = b"".join(out)
    lane = step = 0
    pos = 0
    for line in buf.split(b"\n")[:-1]:
        f = line.split(b"\t")
        if len(f) > 9 + col:
            a = pos + len(b"\t".join(f[:9 + col])) + 1
            b = a + len(f[9 + col]) - 1
            base = pos & ~15
            lane += a // 16 != b // 16
            step += (a - base) // WAVE_STEP != (b - base) // WAVE_STEP
        pos += len(line) + 1
    assert lane > 10 and step >= 2
    both_modes(buf, "S%d" % col, tmp_path, "one")
    both_modes(buf, "S%d,S%d,S%d" % (col - 1, col, col + 1), tmp_path, "adjacent")
    both_modes(buf, ",".join("S%d" % i for i in range(0, ns, 2)), tmp_path, "every_second")


def test_lines_wider_than_the_staging_ring(tmp_path):
    """a line passes through a ring of SX_STAGE bytes per wave in steps of 1 KiB: lines of a few
    rings, and one of 300 KB, keep their tab count and output offset across the steps"""
    ns = 130
    lengths = [SX_STAGE * 2 + 5, SX_STAGE * 3, 5 * SX_STAGE - 1, 300001, 700, SX_STAGE + WAVE_STEP + 1]
    buf = R.sized_vcf(ns, lengths)
    wide = b"\t".join([b"1\t9\t.\tA\tT\t.\tPASS\t.\tGT:PL"] + [b"0/1:" + b"%d" % i * 40 for i in range(ns)]) + b"\n"
    assert len(wide) > 4 * SX_STAGE
    buf += wide * 3 + wide[:-1] + b"\tmore\n" + wide[:len(wide) // 2] + b"\n"
    for tag, sel in selections(ns).items():
        both_modes(buf, sel, tmp_path, tag)


def _run_bin(argv, stdin=b"", env=None):
    r = subprocess.run(argv, executable=BIN, input=stdin, capture_output=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    return r.stdout, r.stderr, r.returncode


@pytest.mark.parametrize("block", ["1", "7", "64"])
def test_block_knob_makes_many_blocks(block, tmp_path):
    """VCFXG_SX_BLOCK lines per device call: a few hundred ragged records in many blocks, and in
    blocks of one line; stdin mode selects again at a '#CHROM' line inside a block"""
    ns = 20
    buf = R.ragged_vcf(7, 300, ns, crlf=True)
    mid = buf.split(b"\n")
    mid.insert(150, b"\t".join([R.HDR9, b"S3", b"Q", b"S1"]) + b"\r")
    mid.insert(220, b"#CHROM\tshort\r")
    buf2 = b"\n".join(mid)
    path = tmp_path / "in.vcf"
    for data in (buf, buf2):
        path.write_bytes(data)
        runs = [(argv, stdin) for sel in ("S1,S19", "S0,S3,nobody", ",".join("S%d" % i for i in range(ns)))
                for argv, stdin in (([TOOL, "-s", sel, "-i", str(path)], b""), ([TOOL, "-s", sel], data))]
        with ThreadPoolExecutor(6) as ex:  # (a process each: the knob is read when the context opens)
            got = list(ex.map(lambda r: _run_bin(r[0], r[1], {"VCFXG_SX_BLOCK": block}), runs))
        for (argv, stdin), g in zip(runs, got):
            assert g == R.run(argv, stdin), (block, argv[1:])


@pytest.fixture(scope="module")
def synth_inputs():
    return {"fixed_stride": synth.generate(300, 2504, 71, 0, 0.001, 0, 0.0, 0),
            "gt_ad_dp": synth.generate(200, 2504, 72, 0, 0.002, 0, 0.0, 0, format_mode=1)}


def _sample_names(buf):
    for line in buf.split(b"\n"):
        if line[:6] == b"#CHROM":
            return [x.decode() for x in line.split(b"\t")[9:]]
    raise AssertionError("no #CHROM line")


@pytest.mark.parametrize("which", ["fixed_stride", "gt_ad_dp"])
@pytest.mark.parametrize("keep", [1, 25, 626, 2504])
def test_cohort_inputs(synth_inputs, which, keep, tmp_path):
    """2,504 samples x a few hundred records, a/b\\t records and GT:AD:DP ones, keeping 1, 25,
    626 and every sample; keeping all in file mode gives the input back"""
    buf = synth_inputs[which]
    nm = _sample_names(buf)
    assert len(nm) == 2504
    pick = nm if keep == 2504 else nm[1::len(nm) // keep][:keep]
    assert len(pick) == keep
    both_modes(buf, ",".join(pick), tmp_path)
    if keep == 2504:
        path = tmp_path / "in.vcf"
        assert tools.run([TOOL, "-s", ",".join(pick), "-i", str(path)])[0] == buf


def _data_part(buf):
    """(offset of the byte after the first '#CHROM' line, that line's fields)"""
    pos = 0
    for line in buf.split(b"\n"):
        if line[:6] == b"#CHROM":
            return pos + len(line) + 1, line.rstrip(b"\r").split(b"\t")
        pos += len(line) + 1
    raise AssertionError("no #CHROM line")


def _engine(env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return engine.Engine(0)  # (a fresh context reads the knobs)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("mode", [engine.MODE_FILE, engine.MODE_STDIN])
@pytest.mark.parametrize("block", [None, "1", "37"])
def test_raw_abi_summary_and_statuses(mode, block):
    """Engine.sample_extract over the lines after the '#CHROM' line: text, per-line statuses,
    rows, data_lines, warn_lines and text_bytes against the restatement, block by block"""
    ns = 65
    buf = R.ragged_vcf(55, 250, ns, crlf=True)
    lines = buf.split(b"\n")
    lines.insert(100, b"\t".join([R.HDR9, b"S2"]) + b"\r")  # stdin mode: a CHROM status
    buf = b"\n".join(lines)
    ds, _ = _data_part(buf)
    stdin_mode = mode == engine.MODE_STDIN
    eng = _engine({"VCFXG_SX_BLOCK": block} if block else None)
    try:
        eng.load(buf)
        n = eng.index(ds)
        for cols, seen in (([9, 10, 40, 73], True), ([], True), (list(range(9, 9 + ns)), True), ([73], False)):
            want = R.lines(buf[ds:], cols, stdin_mode, seen)
            assert len(want) == n
            text, st, sums = eng.sample_extract_all(0, n, cols, mode, seen)
            assert text == b"".join(o for _, o in want)
            assert st.tolist() == [s for s, _ in want]
            assert len(sums) == (1 if block is None else -(-n // int(block)))
            assert sum(s.n_lines for s in sums) == n
            assert sum(s.rows for s in sums) == sum(s == R.ROW for s, _ in want)
            assert sum(s.data_lines for s in sums) == sum(s in (R.ROW, R.SHORT, R.NO_SAMPLES, R.PRE) for s, _ in want)
            assert sum(s.warn_lines for s in sums) == sum(s in (R.SHORT, R.NO_SAMPLES, R.PRE, R.CHROM) for s, _ in want)
            assert sum(s.text_bytes for s in sums) == len(text)
            assert all(s.general_records == 0 for s in sums)  # no schedule beside the general one
        with pytest.raises(engine.EngineError):
            eng.sample_extract(0, n, [10, 9], mode)  # not ascending
        with pytest.raises(engine.EngineError):
            eng.sample_extract(0, n, [8], mode)  # not a sample column
    finally:
        eng.close()


def test_many_columns_keep_the_mask_in_global_memory(tmp_path):
    """more than 262,144 columns: the kept-field bitmask no longer fits the kernel's LDS share"""
    ns = 270000
    hdr = b"\t".join([R.HDR9] + [b"s%x" % i for i in range(ns)]) + b"\n"
    row = lambda k: b"\t".join([b"1\t%d\t.\tA\tT\t.\tPASS\t.\tGT" % k] + [b"%d" % ((i + k) % 10) for i in range(ns)]) + b"\n"  # noqa: E731
    buf = hdr + row(1) + row(2)[:400001] + b"\n" + row(3)
    both_modes(buf, "s0,s1f,s3ffff,s40000,s41eaf,nobody", tmp_path)


def test_bgzf_input_gives_the_plain_output(tmp_path):
    from tests import _bgzf
    buf = R.ragged_vcf(9, 400, 65)
    plain, comp = tmp_path / "in.vcf", tmp_path / "in.vcf.gz"
    plain.write_bytes(buf)
    comp.write_bytes(_bgzf.bgzf(buf))
    sel = "S1,S64,S30"
    want = R.run([TOOL, "-s", sel, "-i", str(plain)])
    assert tools.run([TOOL, "-s", sel, "-i", str(plain)]) == want
    assert tools.run([TOOL, "-s", sel, "-i", str(comp)]) == want
    # inflated on the device (the host then fetches nothing but header lines)
    assert _run_bin([TOOL, "-s", sel, str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1"}) == want
    # ... with the small read-back window of the other tools' kept lines
    assert _run_bin([TOOL, "-s", sel, str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1", "VCFX_WINDOW_BYTES": "1024"}) == want


@pytest.mark.parametrize("ngpu", [2, 3])
def test_ngpu_gives_the_single_context_bytes(ngpu, tmp_path):
    buf = R.ragged_vcf(11, 700, 20, crlf=True)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    argv = [TOOL, "-s", "S3,S19,nobody", "-i", str(path)]
    assert tools.shard_plan(argv, ngpu)[:2] == (ngpu, 1)  # a record view per rank
    want = R.run(argv)
    assert want[1].count(b"Warning") > 10
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": str(ngpu)}) == want


def test_pipe_chain_into_allele_freq(tmp_path):
    """vcfx_pipe 'VCFX_sample_extractor -s ... | VCFX_allele_freq_calc' against the restatement's
    subset fed to the allele-frequency drop-in"""
    buf = synth.generate(400, 130, 73, 0, 0.01, 0, 0.1, 0)
    nm = _sample_names(buf)
    sel = ",".join(nm[3:90:2])
    subset = R.run([TOOL, "-s", sel], buf)[0]
    want = tools.run(["VCFX_allele_freq_calc"], subset)
    assert want[2] == 0 and want[0].count(b"\n") > 300
    r = subprocess.run([PIPE, "%s -s %s | VCFX_allele_freq_calc" % (TOOL, sel)], input=buf, capture_output=True,
                       timeout=120)
    assert (r.stdout, r.returncode) == (want[0], 0)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    subset_f = R.run([TOOL, "-s", sel, "-i", str(path)])[0]
    r = subprocess.run([PIPE, "%s -s %s -i %s | VCFX_allele_freq_calc" % (TOOL, sel, path)], capture_output=True,
                       timeout=120)
    assert (r.stdout, r.returncode) == (tools.run(["VCFX_allele_freq_calc"], subset_f)[0], 0)
