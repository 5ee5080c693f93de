"""Which schedule each region entry point takes, pinned per (entry, knobs, input).

The parity tests compare the schedules' outputs with each other; this table pins which one a
call runs, read from the per-kernel launch counts (vcfxg_kernel_stats) and, where the entry
notes one, vcfxg_last_schedule.  The expected column is the entry points' own predicates:
records of >= 512 B on average, a FORMAT of exactly "GT" where the walk's kernel needs one,
VCFXG_AF_FUSED 3 / 7 / 8, VCFXG_FQ_WALK -1 / 1, and the walk_overflowed flag an overflowing
walk leaves on the loaded input for every later call, whichever tool makes it.

Inputs (VCFXG_WALK_CHUNK=4096, so 40 records are several walkers):
  a  40 GT-only records x 300 samples (about 1.2 KB a record)
  b  the same with FORMAT GT:DP
  c  40 records x 8 samples (under 512 B a record)
  d  300 records of shape a, then 600 of shape c: the hints say "long" (2 * 4096 / 1240 + 16 =
     22 line slots a walker) and a walker of the tail meets about 60 lines"""

import pytest

from vcfx_amd import engine
from vcfx_amd.engine import MODE_FILE

pytestmark = pytest.mark.gpu

NAMES = ["S%03d" % i for i in range(300)]
HEAD = ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(NAMES) +
        "\n").encode()
GTS = ("0/0", "0/1", "1/1")


def _records(n, ns, fmt, pos0):
    dp = ":12" if fmt == "GT:DP" else ""
    return "".join("1\t%d\t.\tA\tC\t50\tPASS\tDP=10\t%s\t%s\n" % (
        pos0 + i, fmt, "\t".join(GTS[(i * 7 + j * 3 + j // 5) % 3] + dp for j in range(ns))) for i in range(n)).encode()


INPUTS = {
    "a": (HEAD + _records(40, 300, "GT", 100000), 300),
    "b": (HEAD + _records(40, 300, "GT:DP", 100000), 300),
    "c": (HEAD + _records(40, 8, "GT", 100000), 8),
    "d": (HEAD + _records(300, 300, "GT", 100000) + _records(600, 8, "GT", 200000), 300),
}

ENTRIES = {
    "af": lambda e, ds, ns: e.allele_freq_region(ds, MODE_FILE),
    "hwe": lambda e, ds, ns: e.hwe_region(ds, MODE_FILE),
    "ib": lambda e, ds, ns: e.inbreeding_region(ds, MODE_FILE, NAMES[:ns]),
    "dose": lambda e, ds, ns: e.dosage_region(ds, MODE_FILE),
    "ph": lambda e, ds, ns: e.haplotype_phaser(ds, MODE_FILE, 0.8, ns),
    "md": lambda e, ds, ns: e.missing_region(ds, MODE_FILE),
    "gq": lambda e, ds, ns: e.genotype_query_region(ds, "0/1"),
    "nr": lambda e, ds, ns: e.nonref_filter_region(ds, MODE_FILE),
    "ld": lambda e, ds, ns: e.ld_prepare_region(ds, ns),
}
# the profiled name of each entry's walk kernel (the phaser's index walk is the dosage walk)
WALK = {"af": "af_walk", "hwe": "hwe_walk", "ib": "ib_walk", "dose": "dose_walk", "ph": "dose_walk", "md": "md_walk",
        "gq": "fq_walk", "nr": "fq_walk", "ld": "ld_walk"}
WALKS = sorted(set(WALK.values()))
# the schedule names of the entries that note one: (walk, index)
NOTED = {"af": ("af_walk", "af_two_sweep"), "ib": ("ib:walk", "ib:index"), "ph": ("ph_head_walk", "ph_index"),
         "gq": ("fq_walk", "fq_two_sweep"), "nr": ("fq_walk", "fq_two_sweep"), "ld": ("ld_walk", "ld_index")}

DEFAULT, AF3, AF7, AF8 = {}, {"VCFXG_AF_FUSED": "3"}, {"VCFXG_AF_FUSED": "7"}, {"VCFXG_AF_FUSED": "8"}
FQ_NEVER, FQ_ALWAYS = {"VCFXG_FQ_WALK": "-1"}, {"VCFXG_FQ_WALK": "1"}
INDEX_ALL = {"VCFXG_AF_FUSED": "8", "VCFXG_FQ_WALK": "-1"}

# (knobs, entry, input, walks, schedule noted if it is not the entry's usual name)
ROWS = []
# default knobs: long records walk; AF (unless "GT:..."), HWE, dosage, the phaser and md need FORMAT "GT"
for name in ENTRIES:
    gt_only = name in ("af", "hwe", "dose", "ph", "md")
    ROWS.append((DEFAULT, name, "a", True, None))
    ROWS.append((DEFAULT, name, "b", not gt_only or name == "af", "af_walk_gt_first" if name == "af" else None))
    ROWS.append((DEFAULT, name, "c", False, None))
# 7 forces the walk for AF, HWE and IB; the dosage and phaser walks are not forced by it
for name in ("af", "hwe", "ib"):
    ROWS.append((AF7, name, "c", True, None))
for name in ("dose", "ph"):
    ROWS.append((AF7, name, "c", False, None))
# 3 and 8 exclude the walk for all five
for name in ("af", "hwe", "ib", "dose", "ph"):
    ROWS.append((AF3, name, "a", False, "af_two_sweep_sync" if name == "af" else None))
    ROWS.append((AF8, name, "a", False, None))
# VCFXG_FQ_WALK: -1 never, 1 always (md then walks without FORMAT "GT", and both on short records)
for name in ("gq", "md"):
    for inp in ("b", "c"):
        ROWS.append((FQ_NEVER, name, inp, False, None))
        ROWS.append((FQ_ALWAYS, name, inp, True, None))


def _row_id(row):
    knobs, name, inp, _, _ = row
    return "-".join([name, inp] + ["%s=%s" % (k[6:], v) for k, v in sorted(knobs.items())])


@pytest.fixture(scope="module", autouse=True)
def walk_chunk():
    # (read when a context opens and again at each load)
    mp = pytest.MonkeyPatch()
    mp.setenv("VCFXG_WALK_CHUNK", "4096")
    yield
    mp.undo()


@pytest.fixture(scope="module")
def engines():
    """one profiling context per knob setting (the knobs are read when the context opens)"""
    cache = {}

    def get(knobs):
        key = tuple(sorted(knobs.items()))
        if key not in cache:
            mp = pytest.MonkeyPatch()
            for k in ("VCFXG_AF_FUSED", "VCFXG_FQ_WALK"):
                mp.delenv(k, raising=False)
            for k, v in knobs.items():
                mp.setenv(k, v)
            try:
                cache[key] = engine.Engine(0)
            finally:
                mp.undo()
            cache[key].set_profiling(True)
        return cache[key]

    yield get
    for e in cache.values():
        e.close()


def _launches(eng, names):
    return {k: eng.kernel_stats(k)[1] for k in names}


def _call(eng, name, inp, load=True):
    """(result, launches of every walk kernel and of the index sweep, last schedule)"""
    buf, ns = INPUTS[inp]
    if load:
        eng.load(buf)
    eng.reset_kernel_stats()
    res = ENTRIES[name](eng, engine.data_start_of(buf), ns)
    return res, _launches(eng, WALKS + ["line_count", "ib_lines"]), eng.L.vcfxg_last_schedule(eng.h).decode()


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_schedule_taken(engines, row):
    knobs, name, inp, walks, noted = row
    _, n, sched = _call(engines(knobs), name, inp)
    others = {k: v for k, v in n.items() if k in WALKS and k != WALK[name] and v}
    assert not others, others
    if walks:
        assert n[WALK[name]] >= 1 and n["line_count"] == 0 and n["ib_lines"] == 0, n
    else:
        assert n[WALK[name]] == 0 and n["line_count"] >= 1 and (name != "ib" or n["ib_lines"] >= 1), n
    if name in NOTED:
        assert sched == (noted or NOTED[name][0 if walks else 1]), sched


def _output(eng, name, res):
    if name == "ld":
        return res, eng.ld_prefixes(res)
    s = (res.n_lines, res.rows, res.data_lines, res.warn_lines, res.general_records, res.text_bytes)
    if name in ("md", "gq", "nr"):
        return s, eng.statuses(res.n_lines).tobytes()
    return s, eng.text(res.text_bytes)


@pytest.mark.parametrize("k", range(len(ENTRIES)), ids=list(ENTRIES))
def test_overflowing_walk_falls_back_and_is_remembered(engines, k):
    """input d: the first call launches its walk once, overflows and takes the index path with
    the index schedule's output; the next call on the loaded context, through another entry
    point, launches no walk at all; after a reload the walk is tried again"""
    names = list(ENTRIES)
    name, other = names[k], names[(k + 1) % len(names)]
    buf, ns = INPUTS["d"]
    ref = engines(INDEX_ALL)
    if name == "ld":  # (no knob of the context turns the LD walk off: the indexed calls themselves)
        ref.load(buf)
        ref.index(engine.data_start_of(buf))
        r = ref.ld_prepare(ns)
        want = _output(ref, name, r)
    else:
        r, n, _ = _call(ref, name, "d")
        assert not any(n[w] for w in WALKS), n
        want = _output(ref, name, r)
    eng = engines(DEFAULT)
    r, n, _ = _call(eng, name, "d")
    assert n[WALK[name]] == 1 and n["line_count"] >= 1, n
    assert _output(eng, name, r) == want
    _, n, _ = _call(eng, other, "d", load=False)
    assert not any(n[w] for w in WALKS) and n["line_count"] >= 1, n
    _, n, _ = _call(eng, name, "d")
    assert n[WALK[name]] == 1, n
