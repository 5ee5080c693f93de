"""Where the AF walk's launch spends its time: T(n) = a + b * n over parts of the bench's shard
(DESIGN §3, §8.1).

One process, one context, one placement of the input in HBM: the shard (427,409 x 2,504 by
default) is loaded once and vcfxg_allele_freq_region runs on its last n records, for n = 1/8,
1/4, 1/2, 3/4 and all of them (the region is [data_start, end): a later data_start is a smaller
region of the same records, without another load), plus two quantisation points: the region
whose uniform walkers are an exact whole number of generations of the resident walkers, and the
one 20 walkers past it.  The walk kernel alone is timed by the engine's events ("af_walk"), R
launches of each region, interleaved.  The fit is least squares over the five fractions; `a` is
what a launch costs beyond streaming (ramp, generation boundaries, drain), `b` the steady rate.

    python tools/af_drain.py [--reps 30] [--label NAME] [--out profiles/af_drain.json]

VCFXG_GPU_LIB / VCFXG_WALK_LAYOUT / VCFXG_WALK_CHUNK in the environment select what is measured
(an --out file that exists gains or replaces the entry `label`).  The resident walkers come from
the library (vcfxg_last_walk_layout after a `fit` walk of a small input); a library without that
entry takes --resident.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def resident_walkers(a):
    """S, from a `fit` walk of a small input in a context of its own"""
    from vcfx_amd import engine, synth
    if not hasattr(engine.lib(), "vcfxg_last_walk_layout"):
        return a.resident
    keep = os.environ.get("VCFXG_WALK_LAYOUT")
    os.environ["VCFXG_WALK_LAYOUT"] = "fit"
    try:
        buf = synth.generate(300, a.samples, 42)
        eng = engine.Engine(0)
        eng.load(buf)
        eng.allele_freq_region(engine.data_start_of(buf), engine.MODE_FILE)
        S = eng.last_walk_layout()["resident"]
        eng.close()
    finally:
        if keep is None:
            del os.environ["VCFXG_WALK_LAYOUT"]
        else:
            os.environ["VCFXG_WALK_LAYOUT"] = keep
    return S or a.resident


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=427409)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--chunk", type=int, default=128 * 1024, help="the uniform chunk the quantisation points are for")
    ap.add_argument("--resident", type=int, default=4096, help="resident walkers, for a library that cannot say")
    ap.add_argument("--label", default="af")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vcfx_amd import engine, synth
    S = resident_walkers(a)
    arr, offs = synth.generate_array(a.records, a.samples, seed=20251226, rec_offsets=True)
    end = int(arr.size)

    def start_for(nbytes):  # the record start that leaves the largest region of at most nbytes
        lo, hi = 0, a.records - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if end - int(offs[mid]) <= nbytes:
                hi = mid
            else:
                lo = mid + 1
        return lo

    points = {}
    for name, frac in (("1/8", 8), ("1/4", 4), ("1/2", 2), ("3/4", 4 / 3.0), ("1", 1)):
        points[name] = a.records - int(round(a.records / frac))
    gens = (end - int(offs[0])) // (S * a.chunk) - 1  # whole generations, the most that fit below the shard
    points["whole_generations"] = start_for(gens * S * a.chunk)
    points["whole_plus_20"] = start_for((gens * S + 20) * a.chunk)
    eng = engine.Engine(0)
    eng.load(arr)
    eng.set_profiling(True)
    ms = {k: [] for k in points}
    for i in range(a.warmup + a.reps):
        for k, first in points.items():
            s = eng.allele_freq_region(int(offs[first]), engine.MODE_FILE)
            assert s.rows == a.records - first, (k, s.rows)
            if i >= a.warmup:
                ms[k].append(eng.kernel_ms("af_walk"))
    layout = eng.last_walk_layout() if hasattr(eng.L, "vcfxg_last_walk_layout") else None
    eng.close()
    rows = {}
    for k, first in points.items():
        nbytes = end - int(offs[first])
        rows[k] = {"records": a.records - first, "bytes": nbytes, "uniform_walkers": -(-nbytes // a.chunk),
                   "generations": round(-(-nbytes // a.chunk) / S, 4), "af_walk_ms_median": round(statistics.median(ms[k]), 5),
                   "af_walk_ms_min": round(min(ms[k]), 5)}
    fit = [rows[k] for k in ("1/8", "1/4", "1/2", "3/4", "1")]
    xs, ys = [r["bytes"] / 1e9 for r in fit], [r["af_walk_ms_median"] for r in fit]
    mx, my = sum(xs) / len(xs), sum(ys) / len(ys)
    b = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    a0 = my - b * mx
    for r in rows.values():
        r["ms_over_fit"] = round(r["af_walk_ms_median"] - (a0 + b * r["bytes"] / 1e9), 5)
    entry = {"records": a.records, "samples": a.samples, "reps": a.reps, "resident_walkers": S, "chunk": a.chunk,
             "layout_of_last_call": layout, "intercept_ms": round(a0, 5), "slope_ms_per_gb": round(b, 5),
             "steady_tbps": round(1.0 / b, 3), "points": rows}
    out = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out[a.label] = entry
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(json.dumps({a.label: entry}))


if __name__ == "__main__":
    sys.exit(main())
