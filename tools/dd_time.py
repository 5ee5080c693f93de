"""Diagnostics: VCFX_duplicate_remover's device work on the bench shard (427,409 records x 2,504
samples, device-resident), without duplicates and with every tenth record repeated 50,000 records
later: vcfxg_index from offset 0 (line_count, line_compact: the unavoidable read of the input, the
yardstick; this change leaves its code as the parent commit has it) and vcfxg_dedup after it
(dd_key, dd_sort = compaction scan + gather + radix sort, dd_verify = run heads + their scan + the
verify and resolve kernels) in the same process on the same bytes; device events summed over a
call, and the host clock around each whole call (both end in a synchronisation).  Two warm-up
calls, then the median of five.  Writes profiles/dd_bench.json."""
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vcfx_amd import engine, synth  # noqa: E402

RECORDS = int(os.environ.get("DD_TIME_RECORDS", 427409))
SAMPLES = 2504
EVERY, LATER = 10, int(os.environ.get("DD_TIME_LATER", 50000))
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


def with_repeats(arr, offs):
    """the shard with record i (i % EVERY == 0) standing again after record i + LATER (after the
    last record when there is none)"""
    offs = offs.astype(np.int64)
    n = len(offs) - 1
    pieces, start = [arr[:offs[0]]], 0
    for j in range(LATER, n, EVERY):  # record j - LATER follows record j
        pieces.append(arr[offs[start]:offs[j + 1]])
        pieces.append(arr[offs[j - LATER]:offs[j - LATER + 1]])
        start = j + 1
    pieces.append(arr[offs[start]:offs[n]])
    first_late = ((n - LATER + EVERY - 1) // EVERY) * EVERY if n > LATER else 0
    for i in range(max(first_late, 0), n, EVERY):
        pieces.append(arr[offs[i]:offs[i + 1]])
    return np.concatenate(pieces), (n + EVERY - 1) // EVERY


def measure(eng, arr):
    eng.load(arr)
    ik, iw = timed(eng, lambda: eng.index(0), IDX_KERNELS)
    s = [None]

    def call():
        s[0] = eng.dedup(engine.MODE_FILE)
    dk, dw = timed(eng, call, DD_KERNELS)
    summ, st, cnt = s[0]
    idx_ms = sum(v["median_ms"] for v in ik.values())
    dd_ms = sum(v["median_ms"] for v in dk.values())
    return {"bytes": int(arr.size), "lines": summ.n_lines, "kept": summ.rows, "data_lines": summ.data_lines,
            "duplicates": cnt[2], "wave_path_lines": cnt[5],
            "index": {"kernels": ik, "call": iw}, "dedup": {"kernels": dk, "call": dw},
            "derived": {"index_kernels_ms": round(idx_ms, 3), "dedup_kernels_ms": round(dd_ms, 3),
                        "dedup_kernels_over_index_kernels": round(dd_ms / idx_ms, 3),
                        "dedup_call_over_index_call": round(dw["median_ms"] / iw["median_ms"], 3),
                        "index_GBps": round(arr.size / idx_ms / 1e6, 1)}}


def main():
    out = {"shape": {"records": RECORDS, "samples": SAMPLES, "repeat_every": EVERY, "repeat_later": LATER},
           "warmup_calls": WARM, "timed_calls": REPS,
           "how": "kernel figures: device events around each launch group, summed per call, median of the timed calls; "
                  "call figures: host clock around the call (each ends in a stream synchronisation; the dedup call "
                  "includes the fetch of the per-line statuses), profiling off",
           "clocks_before": clocks()}
    arr, offs = synth.generate_array(RECORDS, SAMPLES, seed=20251226, rec_offsets=True)
    eng = engine.Engine(0)
    out["no_duplicates"] = measure(eng, arr)
    rep, k = with_repeats(arr, offs)
    out["every_tenth_repeated"] = measure(eng, rep)
    out["every_tenth_repeated"]["repeats"] = int(k)
    eng.close()
    assert out["every_tenth_repeated"]["duplicates"] == out["no_duplicates"]["duplicates"] + k
    out["clocks_after"] = clocks()
    dst = os.environ.get("DD_TIME_OUT", os.path.join(REPO, "profiles", "dd_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("no_duplicates", "every_tenth_repeated")}, indent=1))


if __name__ == "__main__":
    main()
