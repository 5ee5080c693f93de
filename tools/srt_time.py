"""Diagnostics: VCFX_sorter's device work, device-resident, on three inputs: the bench shard
(427,409 records x 2,504 samples) with its records shuffled in blocks of SHUFFLE records, the same
shard as generated (already in order), and a sites-only file of the same record count (8 columns,
~50-byte lines, the same shuffle).  Yardsticks in the same process on the same resident bytes:
vcfxg_index from offset 0 (line_count, line_compact), vcfxg_count_byte (the read floor) and a
hipMemcpyAsync device-to-device copy of the same byte count (the stand-in for a line copy).
vcfxg_sort: srt_key (the key pass and the class pass), srt_sort (compaction scan, scatter, the radix
sort passes and the word gathers between them), srt_place (the output lines' lengths and their scan);
vcfxg_sort_text block after block: srt_gather.  Device events summed over a call (or over the block
loop), and the host clock around each whole call; two warm-up calls, then the median of five.  The
gather is repeated on the shuffled shard with non-temporal loads, stores and both (VCFXG_SRT_NT, a
context each) and with one text block for the whole output.  Writes profiles/srt_bench.json."""
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vcfx_amd import engine, synth  # noqa: E402

RECORDS = int(os.environ.get("SRT_TIME_RECORDS", 427409))
SAMPLES = int(os.environ.get("SRT_TIME_SAMPLES", 2504))
SHUFFLE = 1024
WARM, REPS = 2, 5
HBM_PEAK_GBS = 8000.0  # bench.py's HBM_PEAK_GBS
IDX_KERNELS = ("line_count", "line_compact", "line_emit")
SORT_KERNELS = ("srt_key", "srt_sort", "srt_place")


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


def stats(v):
    return {"median_ms": round(med(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


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
    return {k: dict(stats(v), launches_per_call=launches[k]) for k, v in per.items() if launches[k]}, stats(wall)


def device_copy(nbytes):
    """hipMemcpyAsync device to device of nbytes, timed by device events (ctypes on libamdhip64)"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")

    def chk(rc, what):
        if rc != 0:
            raise RuntimeError("%s: hipError %d" % (what, rc))
    src, dst, a, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    chk(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(nbytes)), "hipMalloc")
    chk(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(nbytes)), "hipMalloc")
    chk(hip.hipMemset(src, 0x41, ctypes.c_size_t(nbytes)), "hipMemset")
    chk(hip.hipEventCreate(ctypes.byref(a)), "hipEventCreate")
    chk(hip.hipEventCreate(ctypes.byref(b)), "hipEventCreate")
    ev = []
    for i in range(WARM + REPS):
        chk(hip.hipEventRecord(a, None), "hipEventRecord")
        chk(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(nbytes), 3, None), "hipMemcpyAsync")  # 3: device to device
        chk(hip.hipEventRecord(b, None), "hipEventRecord")
        chk(hip.hipEventSynchronize(b), "hipEventSynchronize")
        ms = ctypes.c_float()
        chk(hip.hipEventElapsedTime(ctypes.byref(ms), a, b), "hipEventElapsedTime")
        if i >= WARM:
            ev.append(ms.value)
    hip.hipFree(src)
    hip.hipFree(dst)
    return dict(stats(ev), bytes_each_way=nbytes, GBps=round(2 * nbytes / med(ev) / 1e6, 1),
                what="hipMemcpyAsync device to device of the input's byte count, device events")


def block_shuffled(arr, offs, seed=7):
    """the records in blocks of SHUFFLE, the blocks in random order"""
    offs = offs.astype(np.int64)
    n = len(offs) - 1
    blocks = [(offs[i], offs[min(i + SHUFFLE, n)]) for i in range(0, n, SHUFFLE)]
    np.random.RandomState(seed).shuffle(blocks)
    return np.concatenate([arr[:offs[0]]] + [arr[a:b] for a, b in blocks])


def sites_only(n):
    """a sites-only file of n records in order, and its record offsets"""
    head = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    lines = [b"%d\t%d\trs%d\t%c\t%c\t%d\tPASS\tDP=%d;AF=0.%03d\n" % (1 + i * 22 // n, 10000 + 37 * i, i, b"ACGT"[i & 3], b"CGTA"[i & 3],
                                                                 20 + i % 70, 100 + i % 900, i % 1000) for i in range(n)]
    offs = np.cumsum([len(head)] + [len(x) for x in lines], dtype=np.int64)
    return np.frombuffer(head + b"".join(lines), np.uint8), offs


def gather_loop(eng, rows):
    j = calls = 0
    while j < rows:
        k = engine.ctypes.c_uint64()
        n = engine.ctypes.c_uint64()
        eng._chk(eng.L.vcfxg_sort_text(eng.h, j, engine.ctypes.byref(k), engine.ctypes.byref(n)), "sort_text")
        j += k.value
        calls += 1
    return calls


def measure_gather(eng, arr, natural=False, load=True):
    """the block loop alone, after one sort"""
    if load:
        eng.load(arr)
        eng.index(0)
    s = eng.sort(engine.MODE_FILE, natural)[0]
    calls = [0]

    def loop():
        calls[0] = gather_loop(eng, s.rows)
    k, w = timed(eng, loop, ("srt_gather",))
    ms = k["srt_gather"]["median_ms"]
    return {"kernels": k, "loop": w, "blocks": calls[0], "GBps_read_plus_written": round(2 * arr.size / ms / 1e6, 1),
            "fraction_of_hbm_peak": round(2 * arr.size / ms / 1e6 / HBM_PEAK_GBS, 3)}


def measure(eng, arr, copy_ms):
    eng.load(arr)
    ik, iw = timed(eng, lambda: eng.index(0), IDX_KERNELS)
    cnt = [0]

    def sweep():
        cnt[0] = eng.count_byte(0, 10)
    ck, cw = timed(eng, sweep, ("count_byte",))
    out = {"bytes": int(arr.size), "index": {"kernels": ik, "call": iw}, "count_byte": {"kernels": ck, "call": cw}}
    idx_ms = sum(v["median_ms"] for v in ik.values())
    for name, natural in (("lexicographic", False), ("natural", True)):
        s = [None]

        def call():
            s[0] = eng.sort(engine.MODE_FILE, natural)
        sk, sw = timed(eng, call, SORT_KERNELS)
        summ, st, counts, order = s[0]
        g = measure_gather(eng, arr, natural, load=False)

        def whole():
            eng.index(0)
            x = eng.sort(engine.MODE_FILE, natural)[0]
            gather_loop(eng, x.rows)
        _, ww = timed(eng, whole, ())
        sort_ms = sum(v["median_ms"] for v in sk.values())
        gms = g["kernels"]["srt_gather"]["median_ms"]
        out[name] = {"lines": summ.n_lines, "written": summ.rows, "kept": summ.data_lines, "wave_path_lines": counts[5],
                     "moved_lines": int((order != np.arange(len(order), dtype=order.dtype)).sum()),
                     "sort": {"kernels": sk, "call": sw}, "gather": g, "index_sort_text_call": ww,
                     "derived": {"index_kernels_ms": round(idx_ms, 3), "sort_kernels_ms": round(sort_ms, 3),
                                 "gather_over_device_copy": round(gms / copy_ms, 3),
                                 "gather_over_count_byte": round(gms / ck["count_byte"]["median_ms"], 3),
                                 "sort_plus_gather_kernels_over_index_kernels": round((sort_ms + gms) / idx_ms, 3),
                                 "sort_and_text_calls_over_index_call":
                                     round((sw["median_ms"] + g["loop"]["median_ms"]) / iw["median_ms"], 3)}}
    return out


def main():
    out = {"shape": {"records": RECORDS, "samples": SAMPLES, "shuffle_block_records": SHUFFLE},
           "warmup_calls": WARM, "timed_calls": REPS, "hbm_peak_GBps": HBM_PEAK_GBS,
           "how": "kernel figures: device events around each launch group, summed per call (srt_gather: per block "
                  "loop), median of the timed calls; call figures: host clock around the call (each ends in a stream "
                  "synchronisation; the sort call includes the fetch of the statuses and the order; the text is not "
                  "fetched), profiling off; gather bytes: the input read once + the output written once",
           "clocks_before": clocks()}
    arr, offs = synth.generate_array(RECORDS, SAMPLES, seed=20251226, rec_offsets=True)
    shuffled = block_shuffled(arr, offs)
    sarr, soffs = sites_only(RECORDS)
    sites = block_shuffled(sarr, soffs)
    copy = device_copy(int(arr.size))
    copy_sites = device_copy(int(sites.size))
    out["device_copy"] = {"wide": copy, "sites_only": copy_sites}
    eng = engine.Engine(0)
    out["wide_shuffled"] = measure(eng, shuffled, copy["median_ms"])
    out["wide_in_order"] = measure(eng, arr, copy["median_ms"])
    out["sites_only_shuffled"] = measure(eng, sites, copy_sites["median_ms"])
    eng.close()
    out["in_order_input_is_left_in_place"] = out["wide_in_order"]["lexicographic"]["moved_lines"] == 0
    out["shuffled_input_is_moved"] = out["wide_shuffled"]["lexicographic"]["moved_lines"] > 0
    variants = {}
    for nt, block in ((0, None), (1, None), (2, None), (3, None), (0, 1 << 34)):
        os.environ["VCFXG_SRT_NT"] = str(nt)
        if block:
            os.environ["VCFXG_SRT_BLOCK"] = str(block)
        e = engine.Engine(0)
        g = measure_gather(e, shuffled)
        e.close()
        g["gather_over_device_copy"] = round(g["kernels"]["srt_gather"]["median_ms"] / copy["median_ms"], 3)
        variants["nt%d%s" % (nt, "_one_block" if block else "")] = g
    os.environ.pop("VCFXG_SRT_NT")
    os.environ.pop("VCFXG_SRT_BLOCK")
    out["gather_variants_wide_shuffled"] = dict(
        variants, what="nt bit 0: non-temporal loads, bit 1: non-temporal stores; one_block: the whole output in one "
                       "text block (VCFXG_SRT_BLOCK = 16 GiB) instead of 256 MiB blocks")
    out["clocks_after"] = clocks()
    dst = os.environ.get("SRT_TIME_OUT", os.path.join(REPO, "profiles", "srt_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("device_copy", "wide_shuffled", "wide_in_order", "sites_only_shuffled",
                                          "gather_variants_wide_shuffled")}, indent=1))


if __name__ == "__main__":
    main()
