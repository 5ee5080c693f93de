"""The device context's state (vcfxg_ctx.h): every buffer is freed when its context closes
(vcfxg_device_bytes_live, the exact sum of the live buffers' capacities, is back where it was); the
one per-line status buffer is served only to the call that wrote it last; and a new index outdates
every tool's results.  Inputs are a header and three data lines of two samples: every buffer is
sized to 4 KiB at least, so the smallest input allocates them all."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import _field_extractor_ref as FX
from vcfx_amd import engine

pytestmark = pytest.mark.gpu

E_STATE = -5
HEAD = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n"
# a multi-allelic line, a line and its duplicate (out of order after the first: the sorter moves them)
DATA = (b"1\t200\t.\tA\tC,G\t.\tPASS\tAC=1,2\tGT\t0|1\t1|2\n"
        b"1\t100\t.\tA\tC\t.\tPASS\tDP=4\tGT\t0|1\t1|1\n"
        b"1\t100\t.\tA\tC\t.\tPASS\tDP=5\tGT\t0|0\t0|1\n")
BUF = HEAD + DATA
N = BUF.count(b"\n")
M = engine.MODE_FILE


def _load_tables(eng):
    eng.regions_load([b"1"], [0], [150], [250])
    cols, pool = FX.table(["CHROM", "POS"], FX.names_of(BUF, False)[0], False)
    eng.fields_load(cols, pool, M)


def _bytes(call, *args):
    """a raw status fetch of N lines: (return code, the bytes)"""
    st = np.zeros(N, np.uint8)
    rc = call(*args, st.ctypes.data)
    return rc, st.tobytes()


# the status calls that work on a plain index: name -> (run, fetch)
def _status_tools(eng):
    L, h = eng.L, eng.h
    return {
        "dedup": (lambda: eng.dedup(M), lambda: _bytes(L.vcfxg_dedup_status, h, 0, N)),
        "sort": (lambda: eng.sort(M), lambda: _bytes(L.vcfxg_sort_status, h, 0, N)),
        "region": (lambda: eng.region_filter(M), lambda: _bytes(L.vcfxg_region_status, h, 0, N)),
        "fasta": (lambda: eng.fasta_scan(0, N, 2), lambda: _fasta_status(eng)),
        "haplotype": (lambda: eng.haplotype_scan(2), lambda: _hx_status(eng)),
    }


def _fasta_status(eng):
    st = np.zeros(N, np.uint8)
    rc = eng.L.vcfxg_fasta_status(eng.h, 0, N, st.ctypes.data, None)
    return rc, st.tobytes()


def _hx_status(eng):
    st = np.zeros(N, np.uint8)
    rc = eng.L.vcfxg_haplotype_lines(eng.h, 0, N, st.ctypes.data, None, None, None, None)
    return rc, st.tobytes()


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(0)
    e.load(BUF)
    _load_tables(e)
    yield e
    e.close()


@pytest.fixture(scope="module")
def alone(eng):
    """each tool's statuses from a run of its own on a fresh index"""
    out = {}
    for name, (run, fetch) in _status_tools(eng).items():
        assert eng.index(0) == N
        run()
        rc, b = fetch()
        assert rc == 0, name
        out[name] = b
    assert len(set(out.values())) == len(out), out  # (the tools class these lines differently)
    return out


def _use_every_tool(e):
    """the calls whose buffers vcfxg_close once missed (allele counter, phaser, splitter), a keyed tool, a
    table tool and the field extractor"""
    ds = len(HEAD)
    e.load(BUF)
    _load_tables(e)
    assert e.index(ds) == 3
    e.allele_counter(0, 3, [0, 1], ["S1", "S2"])
    e.haplotype_phaser(ds, M, 0.1, 2)
    assert e.index(0) == N
    assert e.multiallelic_split(0, N, [(b"AC", 0, 1)])[0].rows == 2
    assert e.sort(M)[0].rows == N
    assert e.region_filter(M)[0].rows == 1
    assert e.fields_scan()[0].rows == 3


def test_nothing_outlives_close():
    start = engine.device_bytes_live()  # (other engines of the session may be open: deltas)
    ends = []
    for _ in range(2):
        e = engine.Engine(0)
        try:
            opened = engine.device_bytes_live()
            assert opened > start
            _use_every_tool(e)
            assert engine.device_bytes_live() > opened
        finally:
            e.close()
        ends.append(engine.device_bytes_live())
    assert ends == [start, start]


def test_a_failed_open_holds_nothing():
    start = engine.device_bytes_live()
    n = ctypes.c_int()
    engine.lib().vcfxg_device_count(ctypes.byref(n))
    with pytest.raises(engine.EngineError):
        engine.Engine(n.value)  # out of range
    assert engine.device_bytes_live() == start


def test_a_status_fetch_is_its_own_or_e_state(eng, alone):
    tools = _status_tools(eng)
    assert eng.index(0) == N
    for a, b in itertools.permutations(tools, 2):
        run_a, fetch_a = tools[a]
        run_b, fetch_b = tools[b]
        run_a()
        assert fetch_a() == (0, alone[a]), (a, b)
        run_b()
        assert fetch_a()[0] == E_STATE, (a, b)
        assert fetch_b() == (0, alone[b]), (a, b)
        run_a()
        assert fetch_a() == (0, alone[a]), (a, b)
        assert fetch_b()[0] == E_STATE, (a, b)


def test_a_call_without_a_fetch_takes_the_statuses_too(eng, alone):
    tools = _status_tools(eng)
    assert eng.index(0) == N
    for a, (run, fetch) in tools.items():
        run()
        assert fetch() == (0, alone[a]), a
        eng.sample_extract(0, N, [9])
        assert fetch()[0] == E_STATE, a
        run()
        assert fetch() == (0, alone[a]), a


def test_a_new_index_outdates_every_result(eng, alone):
    L, h = eng.L, eng.h
    tools = _status_tools(eng)
    u64 = lambda n: np.zeros(n, np.uint64)
    s, k, nb = engine.Summary(), ctypes.c_uint64(), ctypes.c_uint64()
    others = {
        "sort_order": lambda: L.vcfxg_sort_order(h, 0, N, np.zeros(N, np.uint32).ctypes.data),
        "sort_text": lambda: L.vcfxg_sort_text(h, 0, ctypes.byref(k), ctypes.byref(nb)),
        "ms_line_ranges": lambda: L.vcfxg_ms_line_ranges(h, 0, N, u64(N + 1).ctypes.data),
        "haplotype_blocks": lambda: L.vcfxg_haplotype_blocks(h, ctypes.byref(s)),
        "fields_lines": lambda: L.vcfxg_fields_lines(h, 0, N, np.zeros(N, np.uint8).ctypes.data, None, None),
    }

    def run_all():
        eng.multiallelic_split(0, N, [(b"AC", 0, 1)])
        eng.fields_scan()
        for name, (run, fetch) in tools.items():  # (each fetched before the next call runs)
            run()
            assert fetch() == (0, alone[name]), name
        assert [(name, f()) for name, f in others.items()] == [(name, 0) for name in others]

    assert eng.index(0) == N
    run_all()
    assert eng.index(0) == N
    assert [(name, fetch()[0]) for name, (run, fetch) in tools.items()] == [(name, E_STATE) for name in tools]
    assert [(name, f()) for name, f in others.items()] == [(name, E_STATE) for name in others]
    run_all()
