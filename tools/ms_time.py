"""Diagnostics: VCFX_multiallelic_splitter's device call on an input of the bench width (2,504
samples, FORMAT GT:AD:DP:PL, >= 1 GB, device-resident, file mode) of which 0 %, 10 % and 100 % of the
records are tri-allelic (tests/_multiallelic_splitter_ref.py bench_input: a pool of generated
records repeated under rising POS values -- the synthetic bench shard has no multi-allelic record).
Per share: the passes of a whole run over the lines (ms_scan; ms_number = the two scans and the cut;
ms_len; ms_offsets = the scan of the row lengths; ms_write -- device events, summed over the run's
blocks), the whole run by a host clock (every block's call ends in a synchronisation; the text is
not fetched), bytes read (the data lines) and written (the rows).  In the same process, on the same
bytes: a plain stream (vcfxg_count_byte) as the read floor, and VCFX_sample_extractor keeping every
column (vcfxg_sample_extract) as the existing rewrite.  Two warm-up runs, then the median of five.
Writes profiles/ms_bench.json; the "reference_cpu" entry of an existing file (the compiled
reference's wall time on the same inputs on a CPU host, measured by hand with tools/ms_time.py
--reference BIN: the reference is not part of this repository) is carried over."""
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from sx_time import HBM_PEAK_GBS, REPS, WARM, clocks, med, stats, timed  # noqa: E402
from tests import _multiallelic_splitter_ref as R  # noqa: E402

BYTES = int(os.environ.get("MS_TIME_BYTES", 1 << 30))
SAMPLES = 2504
SHARES = tuple(int(x) for x in os.environ.get("MS_TIME_SHARES", "0,10,100").split(","))
KERNELS = ("ms_scan", "ms_number", "ms_len", "ms_offsets", "ms_write")
SX = ("sx_len", "sx_scan", "sx_write")
PATH = os.path.join(REPO, "profiles", "ms_bench.json")


def reference(binary):
    """the compiled reference on the same inputs, file mode, output to /dev/null: wall seconds"""
    res = {"host": "%s, %d CPUs" % (os.uname().machine, os.cpu_count()), "what": "VCFX_multiallelic_splitter -i FILE > /dev/null, "
           "wall time, median of 3 after 1 warm-up", "bytes": BYTES}
    for share in SHARES:
        with tempfile.NamedTemporaryFile(suffix=".vcf") as f:
            f.write(R.bench_input(share, BYTES, SAMPLES))
            f.flush()
            t = []
            for _ in range(4):
                t0 = time.perf_counter()
                subprocess.check_call([binary, "-i", f.name], stdout=subprocess.DEVNULL)
                t.append(time.perf_counter() - t0)
            res[str(share)] = {"seconds": round(med(t[1:]), 3), "GBps_in": round(os.path.getsize(f.name) / med(t[1:]) / 1e9, 3)}
    old = json.load(open(PATH)) if os.path.exists(PATH) else {}
    old["reference_cpu"] = res
    with open(PATH, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1))


def main():
    from vcfx_amd import engine
    out = {"shape": {"samples": SAMPLES, "format": "GT:AD:DP:PL", "bytes_target": BYTES}, "warmup_calls": WARM,
           "timed_calls": REPS, "hbm_peak_GBps": HBM_PEAK_GBS,
           "how": "kernel figures: device events around each launch, summed per run, median of the timed runs; run "
                  "figures: host clock around the block loop (each block's call ends in stream synchronisations; the "
                  "text is not fetched), profiling off; all figures measured, none estimated",
           "clocks_before": clocks()}
    eng = engine.Engine(0)
    res = {}
    for share in SHARES:
        buf = R.bench_input(share, BYTES, SAMPLES)
        start, decls, _ = R.device_view(buf[:1 << 22], False)
        table = R.table_entries(decls)
        in_bytes = len(buf) - start
        eng.load(buf)
        n = eng.index(start)
        del buf
        cnt = [0]

        def stream():
            cnt[0] = eng.count_byte(start, 10)
        k, w = timed(eng, stream, ("count_byte",))
        floor_ms = k["count_byte"]["median_ms"]
        tot = [0, 0, 0, 0]

        def split_run():
            l0, tb, rows, blocks, gen = 0, 0, 0, 0, 0
            while l0 < n:
                s = engine.Summary()
                p = split_run.params
                eng._chk(eng.L.vcfxg_multiallelic_split(eng.h, l0, n, p[0], s), "multiallelic_split")
                l0 += s.n_lines
                tb += s.text_bytes
                rows += s.rows
                gen += s.general_records
                blocks += 1
            tot[:] = [tb, rows, blocks, gen]
        split_run.params = ms_params(table)
        km, wm = timed(eng, split_run, KERNELS)
        dev_ms = sum(km[x]["median_ms"] for x in KERNELS)
        cols = list(range(9, 9 + SAMPLES))
        sx_tot = [0]

        def sx_run():
            l0, tb = 0, 0
            while l0 < n:
                s = eng.sample_extract(l0, n, cols, engine.MODE_FILE, True)
                l0 += s.n_lines
                tb += s.text_bytes
            sx_tot[0] = tb
        ks, ws = timed(eng, sx_run, SX)
        sx_ms = sum(ks[x]["median_ms"] for x in SX)
        res[str(share)] = {
            "lines": int(n), "bytes_read": in_bytes, "bytes_written": tot[0], "rows": tot[1], "blocks_per_run": tot[2],
            "general_records": tot[3], "kernels": km, "call": wm, "kernels_ms": round(dev_ms, 3),
            "kernels_GBps_read_plus_written": round((in_bytes + tot[0]) / dev_ms / 1e6, 1),
            "call_GBps_read_plus_written": round((in_bytes + tot[0]) / wm["median_ms"] / 1e6, 1),
            "read_floor": {"kernels": k, "call": w, "GBps": round(in_bytes / floor_ms / 1e6, 1), "newlines": int(cnt[0])},
            "kernels_over_read_floor": round(dev_ms / floor_ms, 2),
            "sample_extract_keep_all": {"kernels": ks, "call": ws, "kernels_ms": round(sx_ms, 3), "text_bytes": sx_tot[0],
                                        "GBps_read_plus_written": round((in_bytes + sx_tot[0]) / sx_ms / 1e6, 1)},
            "kernels_over_sample_extract": round(dev_ms / sx_ms, 2),
        }
    out["shares_percent_triallelic"] = res
    eng.close()
    out["clocks_after"] = clocks()
    if os.path.exists(PATH):
        with open(PATH) as f:
            old = json.load(f)
        if "reference_cpu" in old:
            out["reference_cpu"] = old["reference_cpu"]
    with open(os.environ.get("MS_TIME_OUT", PATH), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1))


def ms_params(table):
    """a vcfxg_ms_params for the table, kept alive with what it points to"""
    import ctypes

    from vcfx_amd import engine
    ids = [bytes(t[0]) for t in table]
    ent = (engine.MsEntry * max(len(ids), 1))()
    for e, i, t in zip(ent, ids, table):
        e.id, e.id_len, e.section, e.number = i, len(i), int(t[1]), int(t[2])
    p = engine.MsParams(ctypes.cast(ent, ctypes.c_void_p), len(ids), engine.MODE_FILE)
    return ctypes.byref(p), p, ent, ids


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--reference":
        reference(sys.argv[2])
    else:
        main()
