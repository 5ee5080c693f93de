"""GPU parity of VCFX_haplotype_extractor, byte for byte: every golden case of the compiled reference
(tests/golden/haplotype_extractor_cases.json.gz) through the in-process drop-in and the executable;
generated inputs against the plain-Python restatement (tests/_haplotype_extractor_ref.py, itself held to
the goldens by tests/test_haplotype_extractor_ref.py) through the tool in both modes and through the raw
ABI (statuses, POS, member and block numbers, first-flip index, block table, 64-bit row offsets, the
whole text): sample counts around the wave width and the tile's, block lengths around the tile's, runs
of one-member blocks, blocks across tile edges, non-members between members, GT widths mixed inside a
block and a tile, fixed-stride blocks beside others, records longer than a sweep step, flips at the
wave's edges and across non-members, CRLF, BGZF input, VCFX_NGPU=2, a vcfx_pipe chain."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import _haplotype_extractor_ref as R
from tests._golden import REPO
from vcfx_amd import engine, tools

pytestmark = pytest.mark.gpu

TOOL = R.TOOL
BIN = os.path.join(REPO, "build", "src", TOOL, TOOL)
PIPE = os.path.join(REPO, "build", "bin", "vcfx_pipe")
CASES = R.load_cases()
MODES = ((engine.MODE_FILE, False), (engine.MODE_STDIN, True))
TM, TS = R.TILE_MEMBERS, R.TILE_SAMPLES
NONE64, NONE32 = (1 << 64) - 1, (1 << 32) - 1


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


def both_modes(buf, tmp_path, tag="", extra=()):
    """the drop-in in file mode and stdin mode, batch and streaming, against the restatement"""
    path = tmp_path / ("in%s.vcf" % tag)
    path.write_bytes(buf)
    for argv, stdin in (([TOOL, "-i", str(path)], b""), ([TOOL, "-s"], buf)):
        argv = argv + list(extra)
        got, want = tools.run(argv, stdin), R.run(argv, stdin)
        assert got[2] == want[2] and got[1] == want[1], (argv[1:2], tag)
        assert got[0] == want[0], (argv[1:2], tag, len(got[0]), len(want[0]))


def check_engine(e, buf, T=100000, check=False):
    """the raw ABI in both modes as the drop-in drives it, every array against the restatement's device
    view.  Returns the view of the file mode."""
    first = None
    for mode, stdin in MODES:
        v = R.device_view(buf, stdin, T, check)
        assert v is not None and v["status"]
        first = first or v
        ns, nm, nb = len(v["names"]), len(v["fixed"]), len(v["blocks"])
        e.load(buf)
        assert e.index(v["start"]) == len(v["status"])
        s, st, pos, mem, blk, flip = e.haplotype_scan(ns, T, check, mode)
        assert (int(s.n_lines), int(s.rows), int(s.data_lines)) == (len(v["status"]), nm, nb)
        assert int(s.general_records) == v["fixed"].count(False), stdin  # (the members with a row of the cell matrix)
        assert st.tolist() == v["status"], stdin
        assert pos.tolist() == v["pos"], stdin
        assert mem.tolist() == [NONE64 if x < 0 else x for x in v["member"]], stdin
        assert blk.tolist() == [NONE64 if x < 0 else x for x in v["block"]], stdin
        assert flip.tolist() == [NONE32 if x < 0 else x for x in v["flip"]], stdin
        s, fm, lm, bs, be, off, ln = e.haplotype_blocks()
        assert (int(s.rows), int(s.data_lines), int(s.text_bytes)) == (nb, nm, len(v["text"]))
        got = [list(x) for x in zip(fm.tolist(), lm.tolist(), bs.tolist(), be.tolist(), off.tolist(), ln.tolist())]
        assert got == v["blocks"], stdin
        text = e.haplotype_text()
        assert len(text) == len(v["text"])
        if text != v["text"]:
            k = next(i for i, (a, b) in enumerate(zip(text, v["text"])) if a != b)
            raise AssertionError((stdin, k, text[max(0, k - 20):k + 20], v["text"][max(0, k - 20):k + 20]))
    return first


def check(e, buf, tmp_path, tag="", T=100000, check=False):
    extra = (["-b", str(T)] if T != 100000 else []) + (["-c"] if check else [])
    both_modes(buf, tmp_path, tag, extra)
    return check_engine(e, buf, T, check)


@pytest.mark.parametrize("ns", (1, 63, 64, 65, 2 * TS + 1))
def test_sample_counts(eng, tmp_path, ns):
    """samples around the wave and the tile: mixed widths, non-members in between"""
    v = check(eng, R.gen_blocks(100 + ns, ns, [3, TM + 1, 1, 2], widths=(1, 3, 4, 5), between=0.3), tmp_path)
    assert [b[1] - b[0] + 1 for b in v["blocks"]] == [3, TM + 1, 1, 2] and len(set(v["status"])) >= 4


@pytest.mark.parametrize("length", (1, TM - 1, TM, TM + 1, 2 * TM + 1))
def test_block_lengths(eng, tmp_path, length):
    """block lengths around the tile, alone and after a block that shifts them off the tile's edge"""
    v = check(eng, R.gen_blocks(200 + length, 5, [length], widths=(3, 5)), tmp_path, "a")
    assert [b[1] - b[0] + 1 for b in v["blocks"]] == [length]
    v = check(eng, R.gen_blocks(300 + length, TS + 1, [TM // 2 + 1, length, 3], widths=(1, 3, 4)), tmp_path, "b")
    assert [b[1] - b[0] + 1 for b in v["blocks"]] == [TM // 2 + 1, length, 3]


def test_many_one_member_blocks(eng, tmp_path):
    """several hundred one-member blocks: by distance (-b 5), and by alternating CHROMs"""
    buf = R.gen_blocks(400, 3, [300], widths=(3, 4))
    v = check(eng, buf, tmp_path, "b5", T=5)
    assert len(v["blocks"]) == 300 and all(b[0] == b[1] for b in v["blocks"])
    v = check(eng, R.gen_blocks(401, 70, [1] * 260, widths=(1, 3, 5), between=0.2), tmp_path, "chrom")
    assert len(v["blocks"]) == 260
    v = check(eng, buf, tmp_path, "b0", T=0)
    assert len(v["blocks"]) == 300
    v = check(eng, buf, tmp_path, "neg", T=-1)  # (signed: no positive distance fits)
    assert len(v["blocks"]) == 300


def test_block_from_mid_tile_into_the_next(eng, tmp_path):
    """a block that starts in the middle of a tile and ends in the next, among non-members, so member
    numbers and line numbers differ"""
    v = check(eng, R.gen_blocks(500, TS + 3, [TM // 2, TM, TM // 2 + 3, 2 * TM + 5, 1], widths=(1, 3, 4, 5), between=0.5),
              tmp_path)
    assert v["blocks"][1][0] == TM // 2 and v["blocks"][1][1] == TM // 2 + TM - 1
    assert v["member"].count(-1) > 20 and v["status"].count(R.UNPHASED) > 3 and v["status"].count(R.NOGT) > 3


def test_mixed_widths_with_long_gts(eng, tmp_path):
    """GTs of 1, 3, 4, 5 and 300 bytes inside one block and one tile; the lines are longer than one
    sweep step"""
    buf = R.gen_blocks(600, 40, [TM + 3, 4], widths=(1, 3, 4, 5, 300))
    assert max(len(ln) for ln in buf.split(b"\n")) > 2048
    v = check(eng, buf, tmp_path)
    assert max(b[5] for b in v["blocks"]) > 40000
    check(eng, R.gen_blocks(601, 3, [5], widths=(300,)), tmp_path, "all_long")


def test_fixed_stride_block_beside_another(eng, tmp_path):
    buf = R.gen_blocks(700, TS + 1, [TM + 2, TM + 2, 3], widths=(1, 4, 5), fixed_blocks=(1,))
    v = check(eng, buf, tmp_path)
    assert all(v["fixed"][TM + 2:2 * TM + 4]) and not any(v["fixed"][:TM + 2])
    v = check(eng, R.gen_blocks(701, 300, [2 * TM + 1]), tmp_path, "all_fixed")  # (a record longer than a sweep step)
    assert all(v["fixed"]) and v["blocks"][0][5] == len(b"chr1\t100\t%d" % (100 + 20 * TM)) + 300 * 4 * (2 * TM + 1) + 1


def test_formats_with_gt_late(eng, tmp_path):
    v = check(eng, R.gen_blocks(800, 66, [TM + 1, 2], widths=(3, 5, 300), fmt=b"AD:DP:GT", between=0.3), tmp_path, "late")
    assert len(v["blocks"]) == 2
    check(eng, R.gen_blocks(801, 66, [4, TM], widths=(1, 3), fmt=b"GT:AD:DP"), tmp_path, "first")


@pytest.mark.parametrize("at", ((0,), (63,), (64,), (2 * TS,), (5, 70)))
def test_flips(eng, tmp_path, at):
    """-c: a flip at sample 0, 63, 64 and the last sample; two flips name the first"""
    ns = 2 * TS + 1
    for gap, poly in ((0, False), (4, True)):  # (... and across non-members, with polyploid GTs)
        buf = R.gen_flips(ns, at, gap_lines=gap, polyploid=poly)
        v = check(eng, buf, tmp_path, "g%d" % gap, check=True)
        assert [f for f in v["flip"] if f >= 0] == [ns, ns, at[0], ns] and len(v["blocks"]) == 2
        assert len(check_engine(eng, buf, check=False)["blocks"]) == 1
    path = tmp_path / "dbg.vcf"
    path.write_bytes(R.gen_flips(66, at[:1] if at[0] < 66 else (65,), gap_lines=2))
    for argv in ([TOOL, "-c", "-d", "-i", str(path)], [TOOL, "-cdq", "-s", str(path)]):
        assert tools.run(argv) == R.run(argv)


def test_flip_hidden_by_distance_and_chrom(eng, tmp_path):
    """a would-be flip is not examined when CHROM or the distance already opens a block"""
    rec, ns = R.record, 3
    a, b = [b"0|1"] * ns, [b"1|0"] * ns
    buf = b"\n".join([R.chrom_line(ns), rec(b"1", 100, a), rec(b"2", 100, b), rec(b"2", 900000, a), rec(b"2", 900001, b)]) + b"\n"
    v = check(eng, buf, tmp_path, check=True)
    assert [f for f in v["flip"] if f >= 0] == [ns, ns, ns, 0] and len(v["blocks"]) == 4


@pytest.mark.parametrize("final", (True, False))
def test_crlf(eng, tmp_path, final):
    buf = R.gen_blocks(900 + final, 5, [3, TM + 1, 2], widths=(1, 3, 5), between=0.4, crlf=True, final_newline=final)
    v = check(eng, buf, tmp_path)
    assert b"\r" not in v["text"] and len(v["blocks"]) == 3
    parts = buf.split(b"\n")
    lone = b"\n".join(parts[:4] + [b"\r"] + parts[4:])  # a line of '\r' alone: file mode skips it, stdin warns
    both_modes(lone, tmp_path, "lone")
    assert R.device_view(lone, True)["status"].count(R.SHORT) > R.device_view(lone, False)["status"].count(R.SHORT)
    check_engine(eng, lone)


def _run_bin(argv, stdin=b"", env=None):
    r = subprocess.run(argv, executable=BIN, input=stdin, capture_output=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    return r.stdout, r.stderr, r.returncode


def test_bgzf_input_gives_the_plain_output(tmp_path):
    from tests import _bgzf
    buf = R.gen_blocks(41, 20, [TM + 5, 7, 1], widths=(1, 3, 4), between=0.3)
    plain, comp = tmp_path / "in.vcf", tmp_path / "in.vcf.gz"
    plain.write_bytes(buf)
    comp.write_bytes(_bgzf.bgzf(buf))
    want = R.run([TOOL, "-i", str(plain)])
    assert want[0].count(b"\n") == 4 and want[1].count(b"Warning") > 5
    assert tools.run([TOOL, "-i", str(plain)]) == want
    assert tools.run([TOOL, "-i", str(comp)]) == want
    # inflated on the device (the host then fetches the header and the warned lines from there)
    assert _run_bin([TOOL, str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1"}) == want
    # ... and the text through a read-back window that moves many times
    assert _run_bin([TOOL, "-c", str(comp)], env={"VCFX_BGZF_DEVICE_MIN": "1", "VCFX_WINDOW_BYTES": "4096"}) == \
        R.run([TOOL, "-c", str(plain)])


def test_ngpu_gives_the_unsharded_bytes(tmp_path):
    buf = R.gen_blocks(42, 10, [TM + 1, 3], widths=(3, 5), between=0.2)
    path = tmp_path / "in.vcf"
    path.write_bytes(buf)
    argv = [TOOL, "-i", str(path)]
    assert tools.shard_plan(argv, 2)[0] == 1
    want = R.run(argv)
    assert _run_bin(argv) == want
    assert _run_bin(argv, env={"VCFX_NGPU": "2"}) == want


def test_pipe_chain_ending_in_the_tool():
    """vcfx_pipe 'VCFX_nonref_filter | VCFX_haplotype_extractor' against the extractor on the filter's own
    output"""
    lines = R.gen_blocks(43, 10, [40]).split(b"\n")
    homref = b"\t".join(lines[2].split(b"\t")[:9] + [b"0|0"] * 10)
    buf = b"\n".join(lines[:2] + [x for ln in lines[2:-1] for x in (ln, homref)]) + b"\n"
    kept = tools.run(["VCFX_nonref_filter"], buf)
    assert kept[2] == 0 and 20 < kept[0].count(b"\n") < buf.count(b"\n")
    want = R.run([TOOL], kept[0])
    assert want[0].startswith(b"CHROM\tSTART\tEND\tS0\t") and want[0].count(b"\n") == 2
    r = subprocess.run([PIPE, "VCFX_nonref_filter | %s" % TOOL], input=buf, capture_output=True, timeout=120)
    assert (r.stdout, r.returncode) == (want[0], 0)


def test_calls_out_of_order(eng):
    eng.load(b"1\t5\t.\tA\tC\t.\t.\t.\tGT\t0|1\n")
    assert eng.index(0) == 1
    assert eng.L.vcfxg_haplotype_blocks(eng.h, None) == -5  # VCFXG_E_STATE: no scan on this index
    assert eng.L.vcfxg_haplotype_lines(eng.h, 0, 1, None, None, None, None, None) == -5
    s, st, pos, mem, blk, flip = eng.haplotype_scan(1)
    assert (st.tolist(), pos.tolist(), mem.tolist(), blk.tolist(), flip.tolist()) == ([R.MEMBER], [5], [0], [0], [1])
    assert eng.L.vcfxg_haplotype_text(eng.h, None) == -5    # ... and no layout yet
    assert eng.haplotype_blocks()[0].text_bytes == 10 and eng.haplotype_text() == b"1\t5\t5\t0|1\n"
    import ctypes
    p = engine.HxParams(engine.MODE_FILE, 0, 5, 0)
    assert eng.L.vcfxg_haplotype_scan(eng.h, ctypes.byref(p), None) == -3  # VCFXG_E_ARG: no sample
