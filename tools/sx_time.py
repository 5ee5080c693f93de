"""Diagnostics: VCFX_sample_extractor on the bench shard (427,409 records x 2,504 samples,
device-resident, file mode) keeping 1, 25, 626 and all 2,504 samples (evenly spread columns; the
single one is the middle sample): the kernels of a whole pass over the lines (sx_len, sx_scan,
sx_write; device events, summed over the pass's blocks of VCFXG_SX_BLOCK lines), the whole pass by
a host clock (every block's call ends in a synchronisation; the text is not fetched), and the
algorithmic bytes -- the data lines read once plus the output written once -- as GB/s and as a
fraction of the HBM peak bench.py uses.  In the same process: a plain stream of the same input
bytes (vcfxg_count_byte) as the read floor, and for keep-all a device-to-device copy of the same
bytes (hipMemcpyAsync, device events) as the copy yardstick -- the project has no device kernel that copies
lines; its pass-through tools copy kept lines on the host.  Two warm-up passes, then the median of
five.  Writes profiles/sx_bench.json; the "reference_cpu" entry of an existing file (the compiled
reference's wall time on a CPU host, measured by hand: the reference is not part of this
repository) is carried over."""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vcfx_amd import engine, synth  # noqa: E402

RECORDS = int(os.environ.get("SX_TIME_RECORDS", 427409))
SAMPLES = 2504
KEEP = (1, 25, 626, 2504)
WARM, REPS = 2, 5
HBM_PEAK_GBS = 8000.0  # bench.py's HBM_PEAK_GBS
KERNELS = ("sx_len", "sx_scan", "sx_write")


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
    return {k: dict(stats(v), launches_per_call=launches[k]) for k, v in per.items()}, stats(wall)


def walked_fraction(line, lastk):
    """the part of a line one pass loads: whole 1 KiB steps (from the line's 16 B-aligned start)
    up to the one that holds the tab after field lastk -- the walk's stop rule, evaluated on the
    first data line (an estimate from the rule, not a counter)"""
    pos, tabs = -1, 0
    while tabs <= lastk:
        pos = line.find(b"\t", pos + 1)
        if pos < 0:
            return 1.0
        tabs += 1
    return min(1.0, (pos // 1024 + 1) * 1024 / len(line))


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
                what="hipMemcpyAsync device to device of the data bytes, device events")


def main():
    out = {"shape": {"records": RECORDS, "samples": SAMPLES}, "warmup_calls": WARM, "timed_calls": REPS,
           "hbm_peak_GBps": HBM_PEAK_GBS,
           "how": "kernel figures: device events around each launch, summed per pass, median of the timed passes; "
                  "pass figures: host clock around the block loop (each block's call ends in a stream "
                  "synchronisation; the text is not fetched), profiling off; bytes: data lines read once + output "
                  "written once",
           "clocks_before": clocks()}
    arr = synth.generate_array(RECORDS, SAMPLES, seed=20251226)
    head = arr[:1 << 20].tobytes()
    ds = engine.data_start_of(head)
    assert len(head[:ds].split(b"\n")[-2].split(b"\t")) == 9 + SAMPLES
    line0 = head[ds:head.index(b"\n", ds)]
    in_bytes = int(arr.size) - ds
    out["shape"].update(bytes=int(arr.size), data_bytes=in_bytes)
    eng = engine.Engine(0)
    eng.load(arr)
    n = eng.index(ds)
    out["lines"] = int(n)
    k, w = timed(eng, lambda: eng.index(ds), ("line_count",))
    out["index"] = {"kernels": k, "call": w}
    cnt = [0]

    def stream():
        cnt[0] = eng.count_byte(ds, 10)
    k, w = timed(eng, stream, ("count_byte",))
    floor_ms = k["count_byte"]["median_ms"]
    out["read_floor"] = {"kernels": k, "call": w, "GBps": round(in_bytes / floor_ms / 1e6, 1), "newlines": int(cnt[0])}
    res = {}
    for keep in KEEP:
        cols = [9 + SAMPLES // 2] if keep == 1 else [9 + (i * SAMPLES) // keep for i in range(keep)]
        tot = [0, 0, 0]

        def one_pass():
            l0, tb, rows, blocks = 0, 0, 0, 0
            while l0 < n:
                s = eng.sample_extract(l0, n, cols, engine.MODE_FILE, True)
                l0 += s.n_lines
                tb += s.text_bytes
                rows += s.rows
                blocks += 1
            tot[:] = [tb, rows, blocks]
        k, w = timed(eng, one_pass, KERNELS)
        dev_ms = sum(k[x]["median_ms"] for x in KERNELS)
        moved = in_bytes + tot[0]
        frac = walked_fraction(line0, cols[-1])
        res[str(keep)] = {
            "columns": cols if keep <= 25 else "%d evenly spread from field %d to %d" % (keep, cols[0], cols[-1]),
            "kernels": k, "call": w, "text_bytes": tot[0], "rows": tot[1], "blocks_per_pass": tot[2],
            "algorithmic_bytes": moved,
            "kernels_GBps": round(moved / dev_ms / 1e6, 1),
            "kernels_frac_of_hbm_peak": round(moved / dev_ms / 1e6 / HBM_PEAK_GBS, 4),
            "call_GBps": round(moved / w["median_ms"] / 1e6, 1),
            "kernels_over_read_floor": round(dev_ms / floor_ms, 2),
            "input_loaded_per_pass_est": round(frac, 3),
            "input_loads_both_passes_est": round(2 * frac, 3),
        }
    out["sample_extract"] = res
    eng.close()
    # the copy yardstick: the same bytes device to device, on the HIP runtime the engine uses
    try:
        out["copy_yardstick"] = device_copy(in_bytes)
        all_ms = sum(res["2504"]["kernels"][x]["median_ms"] for x in KERNELS)
        out["copy_yardstick"]["keep_all_kernels_over_copy"] = round(all_ms / out["copy_yardstick"]["median_ms"], 2)
    except Exception as e:  # noqa: BLE001
        out["copy_yardstick"] = "not available: %s" % e
    out["clocks_after"] = clocks()
    dst_path = os.environ.get("SX_TIME_OUT", os.path.join(REPO, "profiles", "sx_bench.json"))
    keep_path = os.path.join(REPO, "profiles", "sx_bench.json")
    if os.path.exists(keep_path):
        with open(keep_path) as f:
            old = json.load(f)
        if "reference_cpu" in old:
            out["reference_cpu"] = old["reference_cpu"]
    with open(dst_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("read_floor", "sample_extract", "copy_yardstick", "index")}, indent=1))


if __name__ == "__main__":
    main()
