"""Diagnostics: VCFX_field_extractor's device work on the bench shard (427,409 records x 2,504 samples,
INFO "AF=..;DP=..", device-resident) for three field lists:
  (a) the seven fixed columns            CHROM,POS,ID,REF,ALT,QUAL,FILTER
  (b) (a) and two INFO keys              ...,AF,DP
  (c) (b) and two sample cells           ...,S1:GT,S2504:GT
per list the cell pass (fx_cells), the two scans (fx_number) and the writer (fx_write), the rows and the
text bytes, and the bytes the cell pass must touch (the line's bytes up to the end of the last needed
field, summed on the host over a sample of the lines).  Two yardsticks in the same process: k_sx_len
(vcfxg_sample_extract keeping the one sample at the same last column, 2,512: the same sweep, merged
earlier) and a plain stream of every resident byte (vcfxg_count_byte, the method of tools/af_ceiling.py).
Device events summed over a call; two warm-up calls, then the median of five.  Writes
profiles/fx_bench.json.

The bytes fetched per launch of the cell pass come from counter runs of their own, without tracing, one
list each, which leave the JSON alone (FX_TIME_OUT elsewhere):

    FX_TIME_LIST=a FX_TIME_ONLY=1 FX_TIME_OUT=/tmp/a.json rocprofv3 --pmc FETCH_SIZE --output-format csv \
        -d DIR_a -o p -- python3 -u tools/fx_time.py            (and the same with b, DIR_b)
    python3 tools/fx_time.py --fold a=DIR_a b=DIR_b

--fold reads the *counter_collection.csv files, takes the mean FETCH_SIZE (KB) over the dispatches of
k_fx_cells, writes raw and doubled bytes (gfx950 reports half the bytes of wide coalesced reads; see
tools/pmc_traffic.py) into profiles/fx_bench.json and ASSERTS the issue's one condition: for (a) and (b)
the doubled bytes are below a quarter of the shard.  The bound is set from the design, not from a run: a
record of the shard is about 10 KB and the sweep reads whole 1 KiB steps, so a cell pass that stops after
the first step fetches about a tenth of the shard; a quarter leaves room for cache-line granularity and
the line index, and a pass that read three steps or more of every record would miss it."""
import ctypes
import csv
import glob
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from vcfx_amd import engine, synth  # noqa: E402
import _field_extractor_ref as R  # noqa: E402  (the table builder)

RECORDS = int(os.environ.get("FX_TIME_RECORDS", 427409))
SAMPLES = 2504
WARM, REPS = 2, 5
A = "CHROM,POS,ID,REF,ALT,QUAL,FILTER"
LISTS = {"a": A, "b": A + ",AF,DP", "c": A + ",AF,DP,S1:GT,S%d:GT" % SAMPLES}
LAST_FIELD = {"a": 6, "b": 7, "c": 9 + SAMPLES - 1}


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def clocks():
    """the clock state as the SMI tool reports it (read only), or why not"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, timeout=20)
        return json.loads(r.stdout) if r.returncode == 0 else "rocm-smi rc=%d" % r.returncode
    except Exception as e:  # noqa: BLE001
        return "not available: %s" % e


def timed(eng, call, kernels):
    for _ in range(WARM):
        call()
    per = {k: [] for k in kernels}
    eng.set_profiling(True)
    for _ in range(REPS):
        eng.reset_kernel_stats()
        call()
        for k in kernels:
            per[k].append(eng.kernel_stats(k)[0])
    eng.set_profiling(False)
    return {k: {"median_ms": round(med(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in per.items()}


def touched_bytes(arr, offs, last_field, step=997):
    """the bytes of a line up to the end of field last_field, scaled from every step-th record"""
    tot = 0
    idx = range(0, len(offs) - 1, step)
    for i in idx:
        line = bytes(arr[offs[i]:offs[i + 1] - 1])
        p = -1
        for _ in range(last_field + 1):
            p = line.find(b"\t", p + 1)
            if p < 0:
                p = len(line)
                break
        tot += p
    return int(tot * (len(offs) - 1) / len(idx))


def main():
    out = {"shape": {"records": RECORDS, "samples": SAMPLES}, "warmup_calls": WARM, "timed_calls": REPS,
           "how": "device events around each launch group, summed per call, median of the timed calls; one process, "
                  "the input resident, the lists and the yardsticks in turn",
           "clocks_before": clocks(), "lists": {}}
    arr, offs = synth.generate_array(RECORDS, SAMPLES, seed=20251226, info_mode=1, rec_offsets=True)
    offs = offs.astype(np.int64)
    eng = engine.Engine(0)
    eng.load(arr)
    nl = eng.index(0)
    out["bytes"] = int(arr.size)
    only = os.environ.get("FX_TIME_LIST")
    for tag, fields in LISTS.items():
        if only and tag != only:
            continue
        cols, pool = R.table(fields.split(","), {}, False)
        eng.fields_load(cols, pool, engine.MODE_FILE)
        res = {}

        def call():
            s = engine.Summary()
            eng._chk(eng.L.vcfxg_fields_scan(eng.h, 0, ctypes.byref(s)), "fields_scan")
            eng._chk(eng.L.vcfxg_fields_text(eng.h, ctypes.byref(s)), "fields_text")
            res["s"] = s
        k = timed(eng, call, ("fx_cells", "fx_number", "fx_write"))
        s = res["s"]
        out["lists"][tag] = {"fields": fields, "rows": int(s.rows), "text_bytes": int(s.text_bytes), "kernels": k,
                             "bytes_the_cell_pass_must_touch": touched_bytes(arr, offs, LAST_FIELD[tag]),
                             "bytes_the_writer_writes": int(s.text_bytes)}
    if not os.environ.get("FX_TIME_ONLY"):
        def sx():
            l0 = 0
            while l0 < nl:
                l0 += eng.sample_extract(l0, nl, [9 + SAMPLES - 1], engine.MODE_FILE, True).n_lines
        out["sx_len"] = timed(eng, sx, ("sx_len",))["sx_len"]
        out["stream"] = timed(eng, lambda: eng.count_byte(0, 10), ("count_byte",))["count_byte"]
        L = out["lists"]
        if all(t in L for t in "abc"):
            st = out["stream"]["median_ms"]
            out["derived"] = {"fx_cells_c_over_sx_len": round(L["c"]["kernels"]["fx_cells"]["median_ms"] / out["sx_len"]["median_ms"], 3),
                              "fx_cells_a_share_of_stream": round(L["a"]["kernels"]["fx_cells"]["median_ms"] / st, 4),
                              "fx_cells_b_share_of_stream": round(L["b"]["kernels"]["fx_cells"]["median_ms"] / st, 4),
                              "touched_share_a": round(L["a"]["bytes_the_cell_pass_must_touch"] / arr.size, 5),
                              "touched_share_b": round(L["b"]["bytes_the_cell_pass_must_touch"] / arr.size, 5)}
    eng.close()
    out["clocks_after"] = clocks()
    out["fetched_bytes_per_launch"] = "not folded in yet: counter runs of their own, then --fold (see the docstring)"
    dst = os.environ.get("FX_TIME_OUT", os.path.join(REPO, "profiles", "fx_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("lists", "sx_len", "stream", "derived") if k in out}, indent=1))


def fold(args):
    """--fold a=DIR b=DIR: the counter runs' FETCH_SIZE of k_fx_cells into profiles/fx_bench.json"""
    dst = os.path.join(REPO, "profiles", "fx_bench.json")
    with open(dst) as f:
        out = json.load(f)
    res = {}
    for a in args:
        tag, d = a.split("=", 1)
        vals = []
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if row.get("Counter_Name") == "FETCH_SIZE" and "k_fx_cells" in row["Kernel_Name"]:
                        vals.append(float(row["Counter_Value"]))
        assert vals, "no k_fx_cells dispatch with FETCH_SIZE under %s" % d
        kb = sum(vals) / len(vals)
        res[tag] = {"dispatches": len(vals), "fetch_size_kb_raw_mean": round(kb, 1), "fetch_bytes_raw": int(kb * 1024),
                    "fetch_bytes_doubled": int(kb * 2048), "share_of_shard_doubled": round(kb * 2048 / out["bytes"], 4)}
    out["fetched_bytes_per_launch"] = {"how": "rocprofv3 --pmc FETCH_SIZE, a run per list with no tracing, the mean over the "
                                              "dispatches of k_fx_cells; doubled as tools/pmc_traffic.py does for gfx950",
                                       "bound": "doubled bytes < shard bytes / 4 for (a) and (b)", "lists": res}
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1))
    for tag in ("a", "b"):
        if tag in res:
            assert res[tag]["fetch_bytes_doubled"] < out["bytes"] / 4, (tag, res[tag], "the early stop is not working")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--fold":
        fold(sys.argv[2:])
    else:
        main()
