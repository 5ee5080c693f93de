"""Diagnostics: VCFX_inbreeding_calculator on the bench shard (427,409 records x 2,504 samples,
device-resident): the stage kernels (ib_walk, ib_table, ib_pack, ib_chain, ib_rows; device events, summed
over a call's blocks), the whole vcfxg_inbreeding_region call (host clock around the call,
which ends in a synchronisation), the LD walk and the AF walk on the same bytes, and the
chain's lower bound: records x the dependent fp64 add latency (build/bin/vcfx_dadd_latency).
Two warm-up calls, then the median of five.  Writes profiles/ib_bench.json; the "reference_cpu" entry of
an existing profiles/ib_bench.json (the compiled reference's wall time on a CPU host, measured by
hand: the reference is not part of this repository) is carried over."""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vcfx_amd import engine, synth  # noqa: E402

RECORDS = int(os.environ.get("IB_TIME_RECORDS", 427409))
SAMPLES = 2504
WARM, REPS = 2, 5


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
                 "launches_per_call": launches[k]} for k, v in per.items()},
            {"median_ms": round(med(wall), 3), "min_ms": round(min(wall), 3), "max_ms": round(max(wall), 3)})


def main():
    out = {"shape": {"records": RECORDS, "samples": SAMPLES}, "warmup_calls": WARM, "timed_calls": REPS,
           "how": "kernel figures: device events around each launch, summed per call, median of the timed calls; "
                  "call figures: host clock around the call (it ends in a stream synchronisation), profiling off",
           "clocks_before": clocks()}
    lat_bin = os.path.join(REPO, "build", "bin", "vcfx_dadd_latency")
    if not os.path.exists(lat_bin):  # (not part of the default build)
        subprocess.check_call(["make", "-s", "-C", REPO, "build/bin/vcfx_dadd_latency"])
    lat = subprocess.run([lat_bin], capture_output=True, timeout=120)
    out["dadd_latency"] = json.loads(lat.stdout)
    arr = synth.generate_array(RECORDS, SAMPLES, seed=20251226)
    out["shape"]["bytes"] = int(arr.size)
    head = arr[:1 << 20].tobytes()
    ds = engine.data_start_of(head)
    names = head[:ds].split(b"\n")[-2].split(b"\t")[9:]
    assert len(names) == SAMPLES
    eng = engine.Engine(0)
    eng.load(arr)
    res = {}
    for tag, kw in (("excludeSample", {}), ("global", {"freq_mode": 1})):
        s = [None]

        def call():
            s[0] = eng.inbreeding_region(ds, engine.MODE_FILE, names, **kw)
        k, w = timed(eng, call, ("ib_walk", "ib_table", "ib_pack", "ib_chain", "ib_rows"))
        res[tag] = {"kernels": k, "call": w, "used_records": s[0].rows, "parsed_records": s[0].data_lines,
                    "general_records": s[0].general_records, "lines": s[0].n_lines,
                    "schedule": eng.L.vcfxg_last_schedule(eng.h).decode()}
    out["inbreeding_region"] = res
    k, w = timed(eng, lambda: eng.ld_prepare_region(ds, SAMPLES), ("ld_walk",))
    out["ld_prepare_region"] = {"kernels": k, "call": w}
    k, w = timed(eng, lambda: eng.allele_freq_region(ds, engine.MODE_FILE), ("af_walk",))
    out["allele_freq_region"] = {"kernels": k, "call": w}
    eng.close()
    ex = res["excludeSample"]["kernels"]
    bound_ms = RECORDS * out["dadd_latency"]["ns_per_dependent_add"] * 1e-6
    out["derived"] = {
        "ib_walk_over_ld_walk": round(ex["ib_walk"]["median_ms"] / out["ld_prepare_region"]["kernels"]["ld_walk"]["median_ms"], 2),
        "ib_walk_over_af_walk": round(ex["ib_walk"]["median_ms"] / out["allele_freq_region"]["kernels"]["af_walk"]["median_ms"], 2),
        "ib_walk_GBps": round(arr.size / ex["ib_walk"]["median_ms"] / 1e6, 1),
        "chain_bound_ms": round(bound_ms, 3),
        "chain_over_bound": round(ex["ib_chain"]["median_ms"] / bound_ms, 2),
    }
    out["clocks_after"] = clocks()
    dst = os.environ.get("IB_TIME_OUT", os.path.join(REPO, "profiles", "ib_bench.json"))
    out["general_records"] = res["excludeSample"]["general_records"]
    # the reference's CPU wall time is measured by hand on another host: kept across reruns
    keep = os.path.join(REPO, "profiles", "ib_bench.json")
    if os.path.exists(keep):
        with open(keep) as f:
            old = json.load(f)
        if "reference_cpu" in old:
            out["reference_cpu"] = old["reference_cpu"]
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("derived", "inbreeding_region", "ld_prepare_region", "allele_freq_region",
                                          "dadd_latency")}, indent=1))


if __name__ == "__main__":
    main()
