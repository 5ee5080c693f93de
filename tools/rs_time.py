"""Diagnostics: VCFX_region_subsampler's device work on the bench shard (427,409 records x 2,504
samples, device-resident): vcfxg_index from offset 0 (line_count, line_compact: the unavoidable read
of the input), vcfxg_region_filter (rs_class: the lane pass, the wave pass and the finish) against a
table of one interval and against a generated table of about 200,000 intervals over the shard's
chromosome, vcfxg_regions_load alone for 1,000,000 intervals over 24 names (rs_build: dictionary,
keys, radix sort, the reach scan, bounds, the merged rows), and in the same process vcfxg_dedup, whose
dd_key pass (the parent commit's code, reading the same line heads) is the yardstick.  Device events
summed over a call, and the host clock around each whole call (all end in a synchronisation).  Two
warm-up calls, then the median of five.  Writes profiles/rs_bench.json."""
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vcfx_amd import engine, synth  # noqa: E402

RECORDS = int(os.environ.get("RS_TIME_RECORDS", 427409))
SAMPLES = 2504
TABLE = int(os.environ.get("RS_TIME_TABLE", 200000))
BUILD = int(os.environ.get("RS_TIME_BUILD", 1000000))
WARM, REPS = 2, 5
IDX_KERNELS = ("line_count", "line_compact", "line_emit")
DD_KERNELS = ("dd_key", "dd_sort", "dd_verify")


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
    """per kernel the median over REPS calls of its summed time in a call (profiling on), and
    the call's median wall time with profiling off"""
    for _ in range(WARM):
        call()
    per = {k: [] for k in kernels}
    eng.set_profiling(True)
    for _ in range(REPS):
        eng.reset_kernel_stats()
        call()
        for k in kernels:
            per[k].append(eng.kernel_stats(k)[0])
    launches = {k: eng.kernel_stats(k)[1] for k in kernels}
    eng.set_profiling(False)
    wall = []
    for _ in range(REPS):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
    return ({k: {"median_ms": round(med(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                 "launches_per_call": launches[k]} for k, v in per.items() if launches[k]},
            {"median_ms": round(med(wall), 3), "min_ms": round(min(wall), 3), "max_ms": round(max(wall), 3)})


def first_fields(arr, off):
    """(CHROM bytes, POS) of the record at byte off"""
    f = bytes(arr[off:off + 64]).split(b"\t")
    return f[0], int(f[1])


def class_pass(eng, names, cid, s1, e1):
    eng.regions_load(names, cid, s1, e1)
    res = [None]

    def call():
        res[0] = eng.region_filter(engine.MODE_FILE)
    k, w = timed(eng, call, ("rs_class",))
    summ, st, cnt = res[0]
    return {"intervals": len(cid), "merged_intervals": len(eng.regions_merged()), "kept": summ.rows,
            "data_lines": summ.data_lines, "wave_path_lines": cnt[7], "kernels": k, "call": w}


def main():
    out = {"shape": {"records": RECORDS, "samples": SAMPLES, "table_intervals": TABLE, "build_intervals": BUILD},
           "warmup_calls": WARM, "timed_calls": REPS,
           "how": "kernel figures: device events around each launch group, summed per call, median of the timed calls; "
                  "call figures: host clock around the call (each ends in a stream synchronisation; the filter and "
                  "dedup calls include the fetch of the per-line statuses), profiling off",
           "clocks_before": clocks()}
    arr, offs = synth.generate_array(RECORDS, SAMPLES, seed=20251226, rec_offsets=True)
    offs = offs.astype(np.int64)
    chrom, lo = first_fields(arr, offs[0])
    hi = first_fields(arr, offs[len(offs) - 2])[1]
    eng = engine.Engine(0)
    eng.load(arr)
    ik, iw = timed(eng, lambda: eng.index(0), IDX_KERNELS)
    out["bytes"] = int(arr.size)
    out["index"] = {"kernels": ik, "call": iw}
    # one interval: the middle half of the shard's positions
    q = (hi - lo) // 4
    out["one_interval"] = class_pass(eng, [chrom], [0], [lo + q], [hi - q])
    # ~TABLE intervals of 50..150 bases at random places of the shard's span (about half of it covered),
    # on the shard's chromosome and, a tenth of them, on 23 other names
    rnd = np.random.default_rng(7)
    names = [chrom] + [b"chr%d" % i for i in range(1, 24)]
    s1 = rnd.integers(lo, hi, TABLE).astype(np.int32)
    e1 = (s1 + rnd.integers(50, 150, TABLE)).astype(np.int32)
    cid = np.where(rnd.random(TABLE) < 0.9, 0, rnd.integers(1, 24, TABLE)).astype(np.uint32)
    out["large_table"] = class_pass(eng, names, cid, s1, e1)
    # the yardstick: dedup's key pass over the same line heads
    dk, dw = timed(eng, lambda: eng.dedup(engine.MODE_FILE), DD_KERNELS)
    out["dedup"] = {"kernels": dk, "call": dw}
    # the table build alone
    s1 = rnd.integers(1, 200000000, BUILD).astype(np.int32)
    e1 = (s1 + rnd.integers(0, 2000, BUILD)).astype(np.int32)
    cid = rnd.integers(0, 24, BUILD).astype(np.uint32)
    bk, bw = timed(eng, lambda: eng.regions_load(names, cid, s1, e1), ("rs_build",))
    out["build"] = {"intervals": BUILD, "merged_intervals": len(eng.regions_merged()), "kernels": bk, "call": bw}
    eng.close()
    one, large = out["one_interval"]["kernels"]["rs_class"]["median_ms"], out["large_table"]["kernels"]["rs_class"]["median_ms"]
    out["derived"] = {"index_kernels_ms": round(sum(v["median_ms"] for v in ik.values()), 3),
                      "class_pass_over_dd_key": round(one / dk["dd_key"]["median_ms"], 3),
                      "large_table_over_one_interval": round(large / one, 3)}
    out["clocks_after"] = clocks()
    dst = os.environ.get("RS_TIME_OUT", os.path.join(REPO, "profiles", "rs_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("one_interval", "large_table", "dedup", "build", "derived")}, indent=1))


if __name__ == "__main__":
    main()
