"""The AF walk against a plain stream of the same bytes, in the same process.

Each of P fresh processes loads the bench's shard (427,409 x 2,504 by default), then alternates
vcfxg_count_byte (k_count_byte: every resident byte read once, 16 B per lane, nothing else) and
vcfxg_allele_freq_region, R times each after a warmup, with the kernels timed by HIP events on
the engine's stream (the "count_byte" and "af_walk" profiler names).  The box's state changes
between processes, so walk / stream is taken per process; the summary holds every process's
medians and ratio.

    python tools/af_ceiling.py [--procs 3] [--reps 30] [--label NAME] [--out profiles/af_ceiling.json]

VCFXG_GPU_LIB / VCFXG_AF_DEPTH in the environment select the library and the sweep depth measured
(an --out file that exists gains or replaces the entry `label`).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def child(a):
    from vcfx_amd import engine, synth
    arr = synth.generate_array(a.records, a.samples, seed=20251226)
    ds = engine.data_start_of(arr[:1 << 20].tobytes())
    eng = engine.Engine(0)
    eng.load(arr)
    eng.set_profiling(True)
    walk, stream, depth = [], [], None
    for i in range(a.warmup + a.reps):
        nl = eng.count_byte(ds, 10)
        s = eng.allele_freq_region(ds, engine.MODE_FILE)
        assert nl == s.n_lines == a.records and s.rows == a.records, (nl, s.n_lines, s.rows)
        if i >= a.warmup:
            stream.append(eng.kernel_ms("count_byte"))
            walk.append(eng.kernel_ms("af_walk"))
    if hasattr(eng.L, "vcfxg_last_af_depth"):
        depth = list(eng.last_af_depth())
    eng.close()
    nbytes = int(arr.size - ds)
    w, st = statistics.median(walk), statistics.median(stream)
    print(json.dumps({"bytes": nbytes, "reps": a.reps, "af_depth": depth,
                      "af_walk_ms_median": round(w, 4), "af_walk_ms_min": round(min(walk), 4),
                      "count_byte_ms_median": round(st, 4), "count_byte_ms_min": round(min(stream), 4),
                      "count_byte_tbps": round(nbytes / st / 1e9, 3), "af_walk_tbps": round(nbytes / w / 1e9, 3),
                      "walk_over_stream": round(w / st, 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=427409)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--label", default="af")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.procs):  # one after the other: a fresh process each
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup",
                            str(a.warmup), "--records", str(a.records), "--samples", str(a.samples)],
                           stdout=subprocess.PIPE, check=True)
        runs.append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
        sys.stderr.write(json.dumps(runs[-1]) + "\n")
    ratios = [r["walk_over_stream"] for r in runs]
    entry = {"records": a.records, "samples": a.samples, "processes": runs,
             "walk_over_stream_median": statistics.median(ratios),
             "walk_over_stream_range": [min(ratios), max(ratios)]}
    out = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out[a.label] = entry
    text = json.dumps(out, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({a.label: {k: entry[k] for k in ("walk_over_stream_median", "walk_over_stream_range")}}))


if __name__ == "__main__":
    sys.exit(main())
