"""Diagnostics: VCFX_diff_tool's device work, device-resident, on two pairs: the bench shard (427,409
records x 2,504 samples, CHROM 21, POS ascending: sorted under both orders, every key once) against
a copy of it made by a seeded rule (every record i with i % 100 == 49 gets ",<DF>" appended to its
ALT, every record with i % 1000 == 999 is dropped: the unique counts are known in closed form and
checked), and the sites-only pair of the same records (their first eight columns).  Both modes, -s
with and without -n.  Yardsticks in the same process on the same resident bytes: vcfxg_count_byte
(the read floor) and vcfxg_dedup (its key pass reads the same fields).  vcfxg_diff: df_key (the cut,
the key pass), df_text (the two scans and the key text), df_sort / df_classes (default mode),
df_ordered / df_bounds / df_walk (-s), df_place; vcfxg_diff_text block after block: df_gather.
Device events summed over a call, and the host clock around each whole call; two warm-up calls, then
the median of five.  The serial walk: a shuffled sites-only pair of 20,000 lines in all, then (the
time per step known) of as many lines as take about a second.  The reference binary's wall time on
the sites-only pair, where one was placed at oracle/_ref/VCFX_diff_tool (built by hand with the
flags of oracle/Makefile.ref; it is not one of that file's targets): a CPU reference time, not a
ceiling; without one the entry says "not measured".
Writes profiles/df_bench.json.

`--once`: every mode run once on the wide pair after a warm-up, for a separate
`rocprofv3 --kernel-trace --stats` run; `--merge-trace CSV` adds that run's k_df_* rows to the JSON."""
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vcfx_amd import engine, synth  # noqa: E402

RECORDS = int(os.environ.get("DF_TIME_RECORDS", 427409))
SAMPLES = int(os.environ.get("DF_TIME_SAMPLES", 2504))
WARM, REPS = 2, 5
HBM_PEAK_GBS = 8000.0  # bench.py's HBM_PEAK_GBS
DF_KERNELS = ("df_key", "df_text", "df_sort", "df_classes", "df_ordered", "df_bounds", "df_walk", "df_place")
DD_KERNELS = ("dd_key", "dd_sort", "dd_verify")
MODES = (("default", False, False), ("sorted", True, False), ("sorted_natural", True, True))
PATHS = {0: "hash", 1: "bounds", 2: "serial walk"}
OUT = os.environ.get("DF_TIME_OUT", os.path.join(REPO, "profiles", "df_bench.json"))
REF_BIN = os.path.join(REPO, "oracle", "_ref", "VCFX_diff_tool")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v):
    return {"median_ms": round(med(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def timed(eng, call, kernels, warm=WARM, reps=REPS):
    """per kernel the median over the timed calls of its summed time in a call (profiling on), and
    the call's median wall time with profiling off"""
    for _ in range(warm):
        call()
    per = {k: [] for k in kernels}
    eng.set_profiling(True)
    for _ in range(reps):
        eng.reset_kernel_stats()
        call()
        for k in kernels:
            per[k].append(eng.kernel_stats(k)[0])
    launches = {k: eng.kernel_stats(k)[1] for k in kernels}
    eng.set_profiling(False)
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t) * 1e3)
    return {k: dict(stats(v), launches_per_call=launches[k]) for k, v in per.items() if launches[k]}, stats(wall)


def changed(i):
    return i % 100 == 49


def dropped(i):
    return i % 1000 == 999


def closed_form(n):
    chg, drp = sum(1 for i in range(n) if changed(i)), sum(1 for i in range(n) if dropped(i))
    return {"unique_1": chg + drp, "unique_2": chg, "data_1": n, "data_2": n - drp}


def copy_by_rule(arr, offs):
    """the copy: header kept, record i dropped or its ALT extended by the rule"""
    offs = offs.astype(np.int64)
    n = len(offs) - 1
    pieces, at = [], 0
    for i in range(n):
        if dropped(i):
            pieces.append(arr[at:offs[i]])
            at = offs[i + 1]
        elif changed(i):
            head = arr[offs[i]:min(offs[i] + 4096, offs[i + 1])].tobytes()
            tabs, p = [], -1
            for _ in range(5):
                p = head.index(b"\t", p + 1)
                tabs.append(p)
            pieces.append(arr[at:offs[i] + tabs[4]])
            pieces.append(np.frombuffer(b",<DF>", np.uint8))
            at = offs[i] + tabs[4]
    pieces.append(arr[at:])
    return np.concatenate(pieces)


def sites_of(arr, offs):
    """the records' first eight columns, each with its newline, after the same header lines; and
    the record offsets of the result"""
    offs = offs.astype(np.int64)
    n = len(offs) - 1
    head = arr[:offs[0]].tobytes()
    lines = []
    for i in range(n):
        rec = arr[offs[i]:min(offs[i] + 4096, offs[i + 1])].tobytes()
        p = -1
        for _ in range(8):
            p = rec.index(b"\t", p + 1)
        lines.append(rec[:p] + b"\n")
    out = np.frombuffer(head + b"".join(lines), np.uint8)
    return out, np.cumsum([len(head)] + [len(x) for x in lines], dtype=np.int64)


def text_loop(eng):
    calls = total = 0
    for side in (0, 1):
        j = 0
        while True:
            k, n = engine.ctypes.c_uint64(), engine.ctypes.c_uint64()
            eng._chk(eng.L.vcfxg_diff_text(eng.h, side, j, engine.ctypes.byref(k), engine.ctypes.byref(n)), "diff_text")
            if not k.value:
                break
            j += k.value
            total += n.value
            calls += 1
    return calls, total


def load_pair(eng, f1, f2):
    assert f1[-1] == 10
    eng.ingest([f1, f2])
    eng.index(0)
    return int(f1.size)


def measure_pair(eng, f1, f2, want):
    second = load_pair(eng, f1, f2)
    nbytes = int(f1.size + f2.size)
    ck, cw = timed(eng, lambda: eng.count_byte(0, 10), ("count_byte",))
    dk, dw = timed(eng, lambda: eng.dedup(engine.MODE_FILE), DD_KERNELS)
    floor = ck["count_byte"]["median_ms"]
    out = {"bytes": nbytes, "second_start": second, "count_byte": {"kernels": ck, "call": cw},
           "dedup": {"kernels": dk, "call": dw, "kernels_ms": round(sum(v["median_ms"] for v in dk.values()), 3)}}
    for name, assume_sorted, natural in MODES:
        got = [None]

        def call():
            got[0] = eng.diff(second, assume_sorted, natural)
        k, w = timed(eng, call, DF_KERNELS)
        s, st, cnt = got[0]
        assert cnt[:4] == (want["unique_1"], want["unique_2"], want["data_1"], want["data_2"]), (name, cnt, want)
        res = [None]

        def loop():
            res[0] = text_loop(eng)
        gk, gw = timed(eng, loop, ("df_gather",))
        total = sum(v["median_ms"] for v in k.values())
        out[name] = {"lines": int(s.n_lines), "counts": {"unique_1": cnt[0], "unique_2": cnt[1], "data_1": cnt[2], "data_2": cnt[3],
                                                         "skipped": cnt[4], "wave_path_lines": cnt[5], "cut_line": cnt[7]},
                     "path": PATHS[cnt[6]], "diff": {"kernels": k, "call": w}, "text": {"kernels": gk, "loop": gw, "blocks": res[0][0],
                                                                                        "bytes": res[0][1]},
                     "derived": {"diff_kernels_ms": round(total, 3), "diff_kernels_over_count_byte": round(total / floor, 2),
                                 "diff_kernels_over_dedup_kernels": round(total / out["dedup"]["kernels_ms"], 2),
                                 "key_pass_over_dedup_key_pass": round(k["df_key"]["median_ms"] / dk["dd_key"]["median_ms"], 2),
                                 "key_pass_over_count_byte": round(k["df_key"]["median_ms"] / floor, 2),
                                 "count_byte_GBps": round(nbytes / floor / 1e6, 1)}}
    return out


def shuffled_pair(sites, soffs, lines_total, seed=11):
    """two files of lines_total / 2 records each, drawn from the sites-only records, shuffled"""
    rnd = np.random.RandomState(seed)
    n = len(soffs) - 1
    half = lines_total // 2
    files = []
    for _ in range(2):
        pick = rnd.choice(n, half, replace=False)
        files.append(np.concatenate([sites[soffs[i]:soffs[i + 1]] for i in pick]))
    return files


def measure_walk(eng, sites, soffs):
    """the serial walk on shuffled pairs: 20,000 lines in all first; then, the time per step known,
    as many as take about a second (at most the records there are)"""
    out = []
    lines_total = 20000
    for _ in range(2):
        f1, f2 = shuffled_pair(sites, soffs, lines_total)
        second = load_pair(eng, f1, f2)
        got = [None]

        def call():
            got[0] = eng.diff(second, True, False)
        k, w = timed(eng, call, ("df_walk", "df_ordered"), warm=1, reps=3)
        cnt = got[0][2]
        assert cnt[6] == 2, cnt
        ms = k["df_walk"]["median_ms"]
        out.append({"lines_in_all": lines_total, "unique_1": cnt[0], "unique_2": cnt[1], "kernels": k, "call": w,
                    "us_per_line": round(ms * 1e3 / lines_total, 3),
                    "note": "a step moves one pointer or both: between lines / 2 and lines steps; the figure is per line"})
        per_line_ms = ms / lines_total
        grown = int(min(1000.0 / max(per_line_ms, 1e-6), 2 * (len(soffs) - 1) * 0.9, 2000000))
        if grown <= lines_total * 2:
            break
        lines_total = grown - grown % 2
    return out


def reference_time(f1, f2):
    if not os.access(REF_BIN, os.X_OK):
        return "not measured: no reference binary on this host"
    d = tempfile.mkdtemp()
    a, b = os.path.join(d, "a.vcf"), os.path.join(d, "b.vcf")
    f1.tofile(a)
    f2.tofile(b)
    out = {}
    try:
        for name, extra in (("default", []), ("sorted", ["-s"])):
            wall = []
            for _ in range(3):
                t = time.perf_counter()
                r = subprocess.run([REF_BIN, "-a", a, "-b", b] + extra, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                wall.append((time.perf_counter() - t) * 1e3)
                assert r.returncode == 0
            out[name] = dict(stats(wall), what="CPU reference time: wall clock of the reference process, files in the page cache, "
                                               "output discarded; one thread")
    finally:
        os.remove(a)
        os.remove(b)
        os.rmdir(d)
    return out


def build_pairs():
    arr, offs = synth.generate_array(RECORDS, SAMPLES, seed=20251226, rec_offsets=True)
    wide2 = copy_by_rule(arr, offs)
    sites, soffs = sites_of(arr, offs)
    sites2 = copy_by_rule(sites, soffs)
    return arr, wide2, sites, soffs, sites2


def once():
    arr, wide2, _, _, _ = build_pairs()
    eng = engine.Engine(0)
    second = load_pair(eng, arr, wide2)
    for _ in range(2):
        for _, assume_sorted, natural in MODES:
            eng.diff(second, assume_sorted, natural)
            text_loop(eng)
    eng.close()


def merge_trace(path):
    with open(OUT) as f:
        out = json.load(f)
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "k_df_" in name or "k_text_gather" in name:
                short = name.split("(")[0].split("::")[-1]
                rows[short] = {"calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1),
                               "average_us": round(float(r["AverageNs"]) / 1e3, 1)}
    out["rocprofv3_kernel_stats_wide_pair"] = dict(
        rows, what="a separate rocprofv3 --kernel-trace --stats run of `df_time.py --once`: the three modes twice each on the "
                   "wide pair (the first round is the warm-up and is in the figures), with the text loops")
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    if "--once" in sys.argv:
        return once()
    if "--merge-trace" in sys.argv:
        return merge_trace(sys.argv[sys.argv.index("--merge-trace") + 1])
    out = {"shape": {"records": RECORDS, "samples": SAMPLES, "rule": "record i: i % 100 == 49 ALT + ',<DF>', i % 1000 == 999 dropped"},
           "warmup_calls": WARM, "timed_calls": REPS, "hbm_peak_GBps": HBM_PEAK_GBS,
           "how": "kernel figures: device events around each launch group (the scans and the sort included in the group "
                  "they serve), summed per call, median of the timed calls; call figures: host clock around the call (each "
                  "ends in a stream synchronisation; the diff call includes the fetch of the statuses; the text is not "
                  "fetched), profiling off"}
    arr, wide2, sites, soffs, sites2 = build_pairs()
    want = closed_form(RECORDS)
    out["closed_form"] = want
    eng = engine.Engine(0)
    out["wide_pair"] = measure_pair(eng, arr, wide2, want)
    out["sites_only_pair"] = measure_pair(eng, sites, sites2, want)
    out["serial_walk_shuffled_sites_only"] = measure_walk(eng, sites, soffs)
    eng.close()
    out["cpu_reference_sites_only_pair"] = reference_time(sites, sites2)
    out["not_measured"] = ["the reference binary on the wide pair (8.6 GB of files on the GPU host's disk)",
                          "BGZF / gzip input (inflated on the host before the device sees it)",
                          "inputs with many-token ALT fields or long keys in bulk (the wave paths of the key text)",
                          "the executable end to end (process start, file mapping, H2D copy, output write)",
                          "counters (--pmc): no occupancy or bandwidth figure is claimed for any df kernel"]
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
