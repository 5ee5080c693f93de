"""Diagnostics: VCFX_merger's device work, device-resident.  Input: the bench shard (427,409 records x
2,504 samples) dealt round-robin into K = 2 and K = 8 files, every file with the shard's header, in
the default mode, -s and -s -n.  Each file is sorted, so -s takes the sort path.  Closed form: the
merged text is the shard itself (checked: the order against its formula in every mode, the bytes
once per K).  Yardsticks in the same process on the same resident bytes: vcfxg_sort, vcfxg_count_byte
(the read floor) and a hipMemcpyAsync device-to-device copy of the same byte count.  vcfxg_merge:
mg_key (the cut, the key pass and the class pass), mg_order (compaction, the ordered check, the radix
passes and the part gathers between them, or the walk), mg_place (the output lines' lengths and their
scan); vcfxg_merge_text block after block: mg_gather.  Device events summed over a call, and the host
clock around each whole call; warm-up calls, then the median of the timed ones.  One walk-path figure:
a sites-only set, shuffled, in two files under -s, per line.  Writes profiles/mg_bench.json.  No time
here is a pass/fail threshold."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from vcfx_amd import engine, synth  # noqa: E402
import srt_time as S  # noqa: E402  (the shared helpers: timed, device_copy, sites_only, block_shuffled, clocks)

RECORDS = int(os.environ.get("MG_TIME_RECORDS", 427409))
SAMPLES = int(os.environ.get("MG_TIME_SAMPLES", 2504))
WALK_LINES = int(os.environ.get("MG_TIME_WALK_LINES", 100000))
MG_KERNELS = ("mg_key", "mg_order", "mg_place")
MODES = (("default", False, False), ("s", True, False), ("sn", True, True))
S.WARM, S.REPS = 1, 3


def deal(arr, offs, k):
    """the header + records f, f + k, ... for every f; (the joined text, the k + 1 file starts)"""
    offs = offs.astype(np.int64)
    n, head = len(offs) - 1, arr[:offs[0]]
    parts, starts, total = [], [0], 0
    for f in range(k):
        parts.append(head)
        total += head.size
        for i in range(f, n, k):
            parts.append(arr[offs[i]:offs[i + 1]])
        total += int(sum(offs[i + 1] - offs[i] for i in range(f, n, k)))
        starts.append(total)
    return np.concatenate(parts), starts


def gather_loop(eng, rows, sink=None):
    j = calls = 0
    while j < rows:
        k, n = engine.ctypes.c_uint64(), engine.ctypes.c_uint64()
        eng._chk(eng.L.vcfxg_merge_text(eng.h, j, engine.ctypes.byref(k), engine.ctypes.byref(n)), "merge_text")
        if sink is not None:
            sink(eng.text_range(0, n.value))
        j += k.value
        calls += 1
    return calls


def expected_order(n, k, head_lines):
    """the input line of every output line: the header of file 0, then record r = line r // k of file r % k"""
    per = [(n - f + k - 1) // k for f in range(k)]
    first = np.concatenate([[0], np.cumsum([head_lines + p for p in per])])[:k]
    r = np.arange(n, dtype=np.int64)
    return np.concatenate([np.arange(head_lines, dtype=np.int64), first[r % k] + head_lines + r // k])


def measure(eng, arr, offs, k, copy_ms):
    joined, starts = deal(arr, offs, k)
    n = len(offs) - 1
    head_lines = int((arr[:int(offs[0])] == 10).sum())
    eng.load(joined)
    eng.index(0)
    cnt = [0]

    def sweep():
        cnt[0] = eng.count_byte(0, 10)
    ck, cw = S.timed(eng, sweep, ("count_byte",))
    sk, sw = S.timed(eng, lambda: eng.sort(engine.MODE_FILE, False), S.SORT_KERNELS)
    out = {"files": k, "bytes": int(joined.size), "count_byte": {"kernels": ck, "call": cw},
           "vcfxg_sort_of_the_same_bytes": {"kernels": sk, "call": sw}}
    want = expected_order(n, k, head_lines)
    for name, assume_sorted, natural in MODES:
        res = [None]

        def call():
            res[0] = eng.merge(starts, assume_sorted, natural)
        mk, mw = S.timed(eng, call, MG_KERNELS)
        summ, st, counts, order = res[0]
        ok_order = bool(order.size == want.size and (order.astype(np.int64) == want).all())
        calls = [0]

        def loop():
            calls[0] = gather_loop(eng, summ.rows)
        gk, gw = S.timed(eng, loop, ("mg_gather",))
        ok_bytes = None
        if name == "default":  # the merged text is the shard, byte for byte
            pos, same = [0], [True]

            def sink(b):
                a = np.frombuffer(b, np.uint8)
                same[0] = same[0] and pos[0] + a.size <= arr.size and bool((arr[pos[0]:pos[0] + a.size] == a).all())
                pos[0] += a.size
            gather_loop(eng, summ.rows, sink)
            ok_bytes = same[0] and pos[0] == arr.size
        mms = sum(v["median_ms"] for v in mk.values())
        gms = gk["mg_gather"]["median_ms"]
        out[name] = {"lines": summ.n_lines, "written": summ.rows, "kept": summ.data_lines, "wave_path_lines": counts[5],
                     "path": counts[6], "header_file": counts[7], "order_is_the_closed_form": ok_order,
                     "text_is_the_shard": ok_bytes, "merge": {"kernels": mk, "call": mw},
                     "gather": {"kernels": gk, "loop": gw, "blocks": calls[0]},
                     "derived": {"merge_kernels_ms": round(mms, 3),
                                 "merge_kernels_over_sort_kernels": round(mms / sum(v["median_ms"] for v in sk.values()), 3),
                                 "gather_over_device_copy": round(gms / copy_ms, 3),
                                 "gather_over_count_byte": round(gms / ck["count_byte"]["median_ms"], 3),
                                 "gather_GBps_read_plus_written": round((joined.size + arr.size) / gms / 1e6, 1),
                                 "gather_fraction_of_hbm_peak": round((joined.size + arr.size) / gms / 1e6 / S.HBM_PEAK_GBS, 3)}}
    return out


def measure_walk(eng):
    """two sites-only files, each shuffled in blocks: -s walks; per kept line"""
    a, ao = S.sites_only(WALK_LINES // 2)
    fa = S.block_shuffled(a, ao, seed=3)
    fb = S.block_shuffled(a, ao, seed=4)
    joined = np.concatenate([fa, fb])
    eng.load(joined)
    eng.index(0)
    res = [None]

    def call():
        res[0] = eng.merge([0, int(fa.size), int(joined.size)], True, False)
    mk, mw = S.timed(eng, call, MG_KERNELS)
    summ, st, counts, order = res[0]
    ms = mk["mg_order"]["median_ms"]
    return {"lines": summ.n_lines, "kept": summ.data_lines, "path": counts[6], "merge": {"kernels": mk, "call": mw},
            "walk_ns_per_kept_line": round(ms * 1e6 / max(summ.data_lines, 1), 1),
            "what": "mg_order holds the compaction, the ordered check and the walk's launches"}


def main():
    out = {"shape": {"records": RECORDS, "samples": SAMPLES, "walk_lines": WALK_LINES}, "warmup_calls": S.WARM,
           "timed_calls": S.REPS, "hbm_peak_GBps": S.HBM_PEAK_GBS,
           "how": "kernel figures: device events around each launch group, summed per call (mg_gather: per block loop), "
                  "median of the timed calls; call figures: host clock around the call (each ends in a stream "
                  "synchronisation; the merge call includes the fetch of the statuses, the counts and the order; the "
                  "text is not fetched), profiling off; gather bytes: the joined input read once + the output written once",
           "clocks_before": S.clocks()}
    arr, offs = synth.generate_array(RECORDS, SAMPLES, seed=20251226, rec_offsets=True)
    copy = S.device_copy(int(arr.size))
    out["device_copy"] = copy
    eng = engine.Engine(0)
    for k in (2, 8):
        t = time.perf_counter()
        out["k%d" % k] = measure(eng, arr, offs, k, copy["median_ms"])
        out["k%d" % k]["host_seconds_for_this_block"] = round(time.perf_counter() - t, 1)
    out["walk_sites_only_shuffled"] = measure_walk(eng)
    eng.close()
    out["clocks_after"] = S.clocks()
    dst = os.environ.get("MG_TIME_OUT", os.path.join(REPO, "profiles", "mg_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("device_copy", "k2", "k8", "walk_sites_only_shuffled")}, indent=1))


if __name__ == "__main__":
    main()
