"""GPU parity of VCFX_inbreeding_calculator: every golden case of the compiled reference
(tests/golden/inbreeding_cases.json.gz) through the in-process drop-in and the executable;
generated inputs in both modes and with the five flag sets against the numpy restatement
(tests/_inbreeding_ref.py, itself held to the goldens by tests/test_inbreeding_ref.py); the
raw per-sample accumulators, sumExp compared as bit patterns; the walk at several chunk sizes
against the index schedule; chain blocks of 1, 7 and 64 records; BGZF input; VCFX_NGPU=2."""
import os
import subprocess

import numpy as np
import pytest

from tests import _inbreeding_ref as R
from tests._golden import REPO
from tests._inbreeding_cases import case_input, load_cases
from vcfx_amd import engine, synth, tools

pytestmark = pytest.mark.gpu

TOOL = "VCFX_inbreeding_calculator"
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
CASES = load_cases()
FLAGS = [[], ["--freq-mode", "global"], ["--skip-boundary"], ["--skip-boundary", "--count-boundary-as-used"],
         ["--freq-mode", "global", "--skip-boundary"]]
FLAG_KW = [dict(), dict(glob=True), dict(skipb=True), dict(skipb=True, countb=True), dict(glob=True, skipb=True)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_in_process(case, tmp_path):
    stdin, cwd = case_input(case, tmp_path)
    out, err, rc = tools.run(case["argv"], stdin, cwd=cwd)
    assert rc == case["rc"]
    assert out == case["stdout"]
    assert err == case["stderr"]


def test_golden_binary(tmp_path):
    """the executable on every golden case (a process each, eight at a time)"""
    from concurrent.futures import ThreadPoolExecutor
    assert os.access(BIN, os.X_OK)

    def one(k):
        case = CASES[k]
        d = tmp_path / str(k)
        d.mkdir()
        stdin, cwd = case_input(case, d)
        r = subprocess.run([BIN] + case["argv"][1:], input=stdin, capture_output=True, cwd=cwd, timeout=120)
        return (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])

    with ThreadPoolExecutor(8) as ex:
        ok = list(ex.map(one, range(len(CASES))))
    assert all(ok), [CASES[k]["name"] for k, v in enumerate(ok) if not v]


# (records, samples, seed): the chain's lane and wave edges
RAGGED = [(300, 1, 31), (400, 2, 32), (300, 63, 33), (500, 64, 34), (400, 65, 35), (600, 130, 36)]


@pytest.mark.parametrize("cfg", RAGGED, ids=["s%d" % c[1] for c in RAGGED])
def test_ragged_inputs_match_restatement(cfg, tmp_path):
    nrec, ns, seed = cfg
    buf = R.ragged_vcf(seed, nrec, ns, crlf=seed % 3 == 0)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    for fl in FLAGS:
        for argv, stdin in (([TOOL, "-i", str(path)] + fl, b""), ([TOOL] + fl, buf)):
            assert tools.run(argv, stdin) == R.run(argv, stdin), (argv[1:], cfg)


def _synth_cases():
    return {
        "fixed_stride": synth.generate(1500, 2504, 91, 0, 0.001, 0, 0.0, 0),  # a/b\t records
        "gt_ad_dp": synth.generate(400, 2504, 92, 0, 0.002, 0, 0.0, 0, format_mode=1),
        "irregular": synth.generate(2000, 130, 93, 1, 0.02, 0, 0.3, 1),
    }


@pytest.fixture(scope="module")
def synth_inputs():
    return _synth_cases()


@pytest.mark.parametrize("which", ["fixed_stride", "gt_ad_dp", "irregular"])
def test_synth_inputs_match_restatement(synth_inputs, which, tmp_path):
    buf = synth_inputs[which]
    got = _engine_run(buf, engine.MODE_FILE)
    assert got[0].general_records == _expect_general(buf)
    if which == "gt_ad_dp":  # no record of it is fixed-stride: the per-field decode
        assert got[0].general_records == got[0].data_lines > 300
    if which == "irregular":  # some are, some are not
        assert 100 < got[0].general_records < got[0].data_lines - 100
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    for fl in FLAGS:
        for argv, stdin in (([TOOL, "-q", "-i", str(path)] + fl, b""), ([TOOL] + fl, buf)):
            assert tools.run(argv, stdin) == R.run(argv, stdin), (argv[1:], which)


def _header(buf, mode):
    """(sample names, data start) as the drop-in's host side finds them"""
    pos, names = 0, []
    for line in buf.split(b"\n"):
        s = line[:-1] if line.endswith(b"\r") else line
        if mode == engine.MODE_FILE:
            if s and s[:1] != b"#":
                return names, pos
            if s[:6] == b"#CHROM":
                f = s.split(b"\t")
                if f[-1] == b"":
                    f.pop()
                names += f[9:]
        elif s[:1] == b"#" and b"#CHROM" in s:
            return s.split(b"\t")[9:], pos + len(line) + 1
        pos += len(line) + 1
    return names, len(buf)


def _engine_run(buf, mode, env=None, **kw):
    """(summary, text, sum_exp, obs_het, used, schedule) on a fresh context (it reads the knobs)"""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        eng = engine.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    eng.load(buf)
    names, ds = _header(buf, mode)
    s = eng.inbreeding_region(ds, mode, names, freq_mode=int(kw.get("glob", False)),
                              skip_boundary=kw.get("skipb", False), count_boundary_as_used=kw.get("countb", False))
    text = eng.text(s.text_bytes)
    se, oh, us = eng.inbreeding_samples()
    sched = eng.L.vcfxg_last_schedule(eng.h).decode()
    eng.close()
    return s, text, se, oh, us, sched


def _ref_acc(buf, mode, **kw):
    return (R.accumulate_file if mode == engine.MODE_FILE else R.accumulate_stdin)(buf, **kw)


_FIXED = None


def _expect_general(buf):
    """file mode: the parsed records whose sample bytes are not "a s b" fields of one separator
    with a tab between them, i.e. the records the fixed-stride sweep cannot take"""
    import re
    global _FIXED
    if _FIXED is None:
        _FIXED = re.compile(rb"[0-9.]([/|])[0-9.](\t[0-9.]\1[0-9.])*")
    n = 0
    for line in buf[_header(buf, engine.MODE_FILE)[1]:].split(b"\n"):
        s = line[:-1] if line.endswith(b"\r") else line
        f = s.split(b"\t")
        if not s or s[:1] == b"#" or len(f) < 10 or f[4] == b"" or b"," in f[4] or (len(f) == 10 and f[9] == b""):
            continue
        n += _FIXED.fullmatch(b"\t".join(f[9:])) is None
    return n


def _same_acc(got, ref):
    _, text, se, oh, us, _ = got
    assert (se.view(np.uint64) == ref.sum_exp.view(np.uint64)).all()  # bit patterns
    assert (oh == ref.obs_het).all() and (us == ref.used).all()
    assert text == R.rows(ref)


@pytest.mark.parametrize("mode", [engine.MODE_FILE, engine.MODE_STDIN])
@pytest.mark.parametrize("k", range(5))
def test_accumulators_bit_identical(synth_inputs, mode, k):
    """vcfxg_inbreeding_samples against the restatement, per flag set: a ragged input (stale
    codes in file mode) and the fixed-stride one"""
    for buf in (R.ragged_vcf(41, 500, 130), synth_inputs["fixed_stride"]):
        ref = _ref_acc(buf, mode, **FLAG_KW[k])
        got = _engine_run(buf, mode, **FLAG_KW[k])
        _same_acc(got, ref)
        assert (got[0].rows, got[0].data_lines) == (ref.variants, ref.parsed)
        if mode == engine.MODE_FILE:
            assert got[0].general_records == _expect_general(buf)


@pytest.mark.parametrize("mode", [engine.MODE_FILE, engine.MODE_STDIN])
def test_walk_chunks_and_index_schedule_agree(synth_inputs, mode):
    buf = synth_inputs["fixed_stride"]
    ref = _ref_acc(buf, mode)
    base = _engine_run(buf, mode, {"VCFXG_AF_FUSED": "8"})
    assert base[5] == "ib:index"
    _same_acc(base, ref)
    # every parsed record is a/b\t here: the clean step of the fixed-stride sweep makes the codes
    assert base[0].data_lines > 1400 and _expect_general(buf) == 0 and base[0].general_records == 0
    for chunk in ("131072", "20000", "4096"):
        got = _engine_run(buf, mode, {"VCFXG_AF_FUSED": "7", "VCFXG_WALK_CHUNK": chunk})
        assert got[5] == "ib:walk", chunk
        assert got[1] == base[1], chunk
        assert (got[2].view(np.uint64) == base[2].view(np.uint64)).all(), chunk
        assert (got[3] == base[3]).all() and (got[4] == base[4]).all(), chunk
        assert (got[0].rows, got[0].data_lines) == (base[0].rows, base[0].data_lines), chunk
        assert (got[0].general_records, got[0].n_lines) == (0, base[0].n_lines), chunk


def test_walk_on_ragged_records():
    buf = R.ragged_vcf(42, 2000, 20)
    got = _engine_run(buf, engine.MODE_FILE, {"VCFXG_AF_FUSED": "7", "VCFXG_WALK_CHUNK": "4096"})
    assert got[5] == "ib:walk"
    _same_acc(got, _ref_acc(buf, engine.MODE_FILE))


def test_walker_overflow_falls_back_to_the_index():
    """a walker's line slots are sized from the first records (~600 B here); 6,000 records of
    two columns after them are more lines per chunk than that, so the call repeats on the index"""
    head = R.ragged_vcf(45, 300, 130, odd=0.02, short=0.0, junk=0.0)
    if not head.endswith(b"\n"):
        head += b"\n"
    gts = [b"0/0", b"0/1", b"1/1", b"1|0"]
    tail = b"".join(b"1\t%d\t.\tA\tT\t.\tPASS\t.\tGT\t%s\t%s\n" % (5000 + i, gts[i % 4], gts[(i // 4) % 4])
                    for i in range(6000))
    buf = head + tail
    got = _engine_run(buf, engine.MODE_FILE, {"VCFXG_AF_FUSED": "7"})
    assert got[5] == "ib:index"
    _same_acc(got, _ref_acc(buf, engine.MODE_FILE))


@pytest.mark.parametrize("sched", ["7", "8"])
def test_chain_blocks_cross_record_edges(sched):
    """VCFXG_IB_BLOCK 1, 7, 64 and the default on a 300-record ragged file-mode input: the
    carried codes and the sums cross block edges.  On the walk a block is whole walkers (about
    50 line slots each at this chunk size), so 150 and 400 are what change its launches there."""
    buf = R.ragged_vcf(43, 300, 65, short=0.4)
    ref = _ref_acc(buf, engine.MODE_FILE)
    assert ref.variants > 100
    base = _engine_run(buf, engine.MODE_FILE, {"VCFXG_AF_FUSED": sched, "VCFXG_WALK_CHUNK": "4096"})
    _same_acc(base, ref)
    assert base[0].general_records == _expect_general(buf)
    for blk in ("1", "7", "64", "150", "400"):
        got = _engine_run(buf, engine.MODE_FILE, {"VCFXG_AF_FUSED": sched, "VCFXG_WALK_CHUNK": "4096",
                                                  "VCFXG_IB_BLOCK": blk})
        _same_acc(got, ref)
        assert (got[0].n_lines, got[0].general_records) == (base[0].n_lines, base[0].general_records), blk


def test_bgzf_input_gives_the_plain_output(synth_inputs, tmp_path):
    from tests import _bgzf
    buf = synth_inputs["irregular"]
    plain, comp = tmp_path / "in.vcf", tmp_path / "in.vcf.gz"
    plain.write_bytes(buf)
    comp.write_bytes(_bgzf.bgzf(buf))
    want = tools.run([TOOL, "-q", "-i", str(plain)])
    assert want == R.run([TOOL, "-q", "-i", str(plain)])
    assert tools.run([TOOL, "-q", "-i", str(comp)]) == want
    # device inflate of a small file too (the tool then fetches nothing but header lines)
    r = subprocess.run([BIN, "-q", str(comp)], capture_output=True, timeout=120,
                       env=dict(os.environ, VCFX_BGZF_DEVICE_MIN="1"))
    assert (r.stdout, r.stderr, r.returncode) == want


def test_ngpu_runs_on_one_context(tmp_path):
    buf = R.ragged_vcf(44, 800, 20)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    argv = [TOOL, "-i", str(path), "--skip-boundary"]
    assert tools.shard_plan(argv, 2)[0] == 1  # unsharded: record order is the contract
    want = R.run(argv)
    one = subprocess.run([BIN] + argv[1:], capture_output=True, timeout=120)
    two = subprocess.run([BIN] + argv[1:], capture_output=True, timeout=120, env=dict(os.environ, VCFX_NGPU="2"))
    assert (one.stdout, one.stderr, one.returncode) == want
    assert (two.stdout, two.stderr, two.returncode) == want
