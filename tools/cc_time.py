"""Diagnostics: VCFX_cross_sample_concordance on the bench shard (427,409 records x 2,504 samples,
device-resident): the call's kernels (cc_walk, walk_compact, cc_lines, cc_rows, cc_format; device
events, summed over a call), the whole vcfxg_concordance_region call (host clock around the call,
which ends in a synchronisation) in record order and in the order of 64 workers, the same on the
schedule without the walk (a second context opened with VCFXG_AF_FUSED=8: the line index and
k_cc_lines on every line), and the AF walk and the HWE walk of the same process on the same
bytes.  Two warm-up calls, then the median of five.  Writes profiles/cc_bench.json."""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vcfx_amd import engine, synth  # noqa: E402

RECORDS = int(os.environ.get("CC_TIME_RECORDS", 427409))
SAMPLES = 2504
WARM, REPS = 2, 5
CC_KERNELS = ("cc_walk", "walk_compact", "line_count", "line_compact", "cc_lines", "cc_rows", "cc_format")


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


def concordance(eng, ds, threads):
    s = [None]

    def call():
        s[0] = eng.concordance(ds, engine.MODE_FILE, n_samples=SAMPLES, threads=threads)
    k, w = timed(eng, call, CC_KERNELS)
    summ, totals, text = s[0]
    return {"kernels": k, "call": w, "rows": summ.rows, "data_lines": summ.data_lines, "text_bytes": summ.text_bytes,
            "general_records": summ.general_records, "lines": summ.n_lines,
            "totals": dict(zip(("concordant", "discordant", "no_genotypes", "data_lines"), totals)),
            "schedule": eng.L.vcfxg_last_schedule(eng.h).decode()}


def main():
    out = {"shape": {"records": RECORDS, "samples": SAMPLES}, "warmup_calls": WARM, "timed_calls": REPS,
           "how": "kernel figures: device events around each launch, summed per call, median of the timed calls; "
                  "call figures: host clock around the call (it ends in a stream synchronisation and includes the "
                  "fetch of the text), profiling off",
           "clocks_before": clocks()}
    arr = synth.generate_array(RECORDS, SAMPLES, seed=20251226)
    out["shape"]["bytes"] = int(arr.size)
    ds = engine.data_start_of(arr[:1 << 20].tobytes())
    eng = engine.Engine(0)
    eng.load(arr)
    out["concordance_region"] = {"record_order": concordance(eng, ds, 0), "workers_64": concordance(eng, ds, 64)}
    k, w = timed(eng, lambda: eng.allele_freq_region(ds, engine.MODE_FILE), ("af_walk",))
    out["allele_freq_region"] = {"kernels": k, "call": w}
    k, w = timed(eng, lambda: eng.hwe_region(ds, engine.MODE_FILE), ("hwe_walk",))
    out["hwe_region"] = {"kernels": k, "call": w}
    eng.close()
    os.environ["VCFXG_AF_FUSED"] = "8"  # (read when a context opens)
    eng = engine.Engine(0)
    eng.load(arr)
    out["concordance_region"]["two_sweep"] = concordance(eng, ds, 0)
    eng.close()
    cc = out["concordance_region"]["record_order"]["kernels"]
    af = out["allele_freq_region"]["kernels"]["af_walk"]["median_ms"]
    out["derived"] = {
        "cc_walk_over_af_walk": round(cc["cc_walk"]["median_ms"] / af, 3),
        "cc_walk_over_hwe_walk": round(cc["cc_walk"]["median_ms"] / out["hwe_region"]["kernels"]["hwe_walk"]["median_ms"], 3),
        "cc_walk_GBps": round(arr.size / cc["cc_walk"]["median_ms"] / 1e6, 1),
        "af_walk_GBps": round(arr.size / af / 1e6, 1),
        "two_sweep_cc_lines_over_cc_walk": round(
            out["concordance_region"]["two_sweep"]["kernels"]["cc_lines"]["median_ms"] / cc["cc_walk"]["median_ms"], 2),
    }
    out["clocks_after"] = clocks()
    dst = os.environ.get("CC_TIME_OUT", os.path.join(REPO, "profiles", "cc_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("derived", "concordance_region", "allele_freq_region", "hwe_region")}, indent=1))


if __name__ == "__main__":
    main()
