"""Diagnostics: VCFX_fasta_converter's device calls on an input of the bench width (2,504 samples,
about 1 GB, device-resident, file mode) with FORMAT GT (every record fixed-stride) and GT:AD:DP
(every record on the general path); tests/_fasta_converter_ref.py bench_input: a pool of generated
records repeated under rising POS values.  Per FORMAT: the status pass the drop-in runs first
(fa_scan and fa_number over every block), then the conversion (fa_scan and fa_number again, fa_bases,
fa_transpose -- device events, summed over the run's blocks), each run by a host clock (every block's
call ends in a synchronisation; the text is not fetched), bytes read and written.  In the same
process, on the same bytes: a plain stream (vcfxg_count_byte) as the read floor.  Every pass is
reported against its algorithmic bytes at that measured stream rate and at the 8 TB/s peak:
    fa_bases      reads the data lines, writes S x V bases (rows padded to 16)
    fa_transpose  reads S x V, writes S x V bases and S x ceil(V / 60) newlines
    in all        input + 3 S V + S V / 60
Two warm-up runs, then the median of five.  Writes profiles/fa_bench.json; the "reference_cpu" entry
of an existing file (the compiled reference's wall time on the same inputs on a CPU host, measured
by hand with tools/fa_time.py --reference BIN: the reference is not part of this repository) is
carried over."""
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from sx_time import HBM_PEAK_GBS, REPS, WARM, clocks, med, timed  # noqa: E402
from tests import _fasta_converter_ref as R  # noqa: E402

BYTES = int(os.environ.get("FA_TIME_BYTES", 1 << 30))
SAMPLES = 2504
FORMATS = tuple(os.environ.get("FA_TIME_FORMATS", "GT,GT:AD:DP").split(","))
SCAN = ("fa_scan", "fa_number")
KERNELS = ("fa_scan", "fa_number", "fa_bases", "fa_transpose")
PATH = os.path.join(REPO, "profiles", "fa_bench.json")


def reference(binary):
    """the compiled reference on the same inputs, file mode, output to /dev/null: wall seconds"""
    res = {"host": "%s, %d CPUs" % (os.uname().machine, os.cpu_count()), "what": "VCFX_fasta_converter -i FILE > /dev/null, "
           "wall time, median of 3 after 1 warm-up", "bytes": BYTES}
    for fmt in FORMATS:
        with tempfile.NamedTemporaryFile(suffix=".vcf") as f:
            f.write(R.bench_input(fmt.encode(), BYTES, SAMPLES))
            f.flush()
            t = []
            for _ in range(4):
                t0 = time.perf_counter()
                subprocess.check_call([binary, "-i", f.name], stdout=subprocess.DEVNULL)
                t.append(time.perf_counter() - t0)
            res[fmt] = {"seconds": round(med(t[1:]), 3), "GBps_in": round(os.path.getsize(f.name) / med(t[1:]) / 1e9, 3)}
    old = json.load(open(PATH)) if os.path.exists(PATH) else {}
    old["reference_cpu"] = res
    with open(PATH, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1))


def main():
    import numpy as np

    from vcfx_amd import engine
    out = {"shape": {"samples": SAMPLES, "bytes_target": BYTES}, "warmup_calls": WARM, "timed_calls": REPS,
           "hbm_peak_GBps": HBM_PEAK_GBS,
           "how": "kernel figures: device events around each launch, summed per run, median of the timed runs; run "
                  "figures: host clock around the block loop (each block's call ends in a stream synchronisation; the "
                  "text is not fetched), profiling off; all figures measured, none estimated; the fractions compare a "
                  "pass's time with its algorithmic bytes at the stream rate measured in the same process",
           "clocks_before": clocks()}
    eng = engine.Engine(0)
    res = {}
    for fmt in FORMATS:
        buf = R.bench_input(fmt.encode(), BYTES, SAMPLES)
        start, names, _, _ = R.device_view(buf[:1 << 22], False)
        assert len(names) == SAMPLES
        in_bytes = len(buf) - start
        eng.load(buf)
        n = eng.index(start)
        first = buf[start:buf.index(b"\n", start)]
        del buf
        cnt = [0]

        def stream():
            cnt[0] = eng.count_byte(start, 10)
        k, w = timed(eng, stream, ("count_byte",))
        floor_ms = k["count_byte"]["median_ms"]
        stream_gbps = in_bytes / floor_ms / 1e6
        cols = [0]

        def scan_run():
            l0, c = 0, 0
            while l0 < n:
                s = engine.Summary()
                eng._chk(eng.L.vcfxg_fasta_scan(eng.h, l0, n, engine.MODE_FILE, SAMPLES, s), "fasta_scan")
                l0 += s.n_lines
                c += s.rows
            cols[0] = c
        ks, ws = timed(eng, scan_run, SCAN)
        V = cols[0]
        row = V + (V + R.LINE - 1) // R.LINE
        row_off = (np.arange(SAMPLES + 1, dtype=np.uint64) * np.uint64(row))
        text = SAMPLES * row
        eng.fasta_begin(text)
        tot = [0, 0]

        def fasta_run():
            l0, c, gen, blocks = 0, 0, 0, 0
            while l0 < n:
                s = eng.fasta(l0, n, SAMPLES, c, V, row_off)
                l0 += s.n_lines
                c += s.rows
                gen += s.general_records
                blocks += 1
            tot[:] = [gen, blocks]
        kf, wf = timed(eng, fasta_run, KERNELS)
        dev_ms = sum(kf[x]["median_ms"] for x in KERNELS)
        pitch = (SAMPLES + 15) & ~15
        algo = {"fa_bases": in_bytes + pitch * V, "fa_transpose": pitch * V + text}
        whole = in_bytes + 3 * SAMPLES * V + SAMPLES * V // R.LINE
        sample = eng.text_range(0, min(text, 200))
        res[fmt] = {
            "lines": int(n), "columns": int(V), "record_bytes": len(first) + 1, "bytes_read": in_bytes, "bytes_written": text,
            "bytes_model_input_3SV_SV60": whole, "blocks_per_run": tot[1], "general_records": tot[0],
            "first_row_head": sample[:70].decode("latin-1"),
            "status_pass": {"kernels": ks, "call": ws},
            "conversion": {"kernels": kf, "call": wf, "kernels_ms": round(dev_ms, 3)},
            "read_floor": {"kernels": k, "call": w, "GBps": round(stream_gbps, 1), "newlines": int(cnt[0])},
            "passes": {p: {"bytes": b, "ms": kf[p]["median_ms"], "GBps": round(b / kf[p]["median_ms"] / 1e6, 1),
                           "stream_time_over_time": round((b / stream_gbps / 1e6) / kf[p]["median_ms"], 3),
                           "peak_time_over_time": round((b / HBM_PEAK_GBS / 1e6) / kf[p]["median_ms"], 3)}
                       for p, b in algo.items()},
            "conversion_kernels_GBps_of_model_bytes": round(whole / dev_ms / 1e6, 1),
            "conversion_call_GBps_of_model_bytes": round(whole / wf["median_ms"] / 1e6, 1),
            "model_stream_time_over_kernels": round((whole / stream_gbps / 1e6) / dev_ms, 3),
            "model_peak_time_over_kernels": round((whole / HBM_PEAK_GBS / 1e6) / dev_ms, 3),
        }
    out["formats"] = res
    eng.close()
    out["clocks_after"] = clocks()
    if os.path.exists(PATH):
        with open(PATH) as f:
            old = json.load(f)
        if "reference_cpu" in old:
            out["reference_cpu"] = old["reference_cpu"]
    with open(os.environ.get("FA_TIME_OUT", PATH), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--reference":
        reference(sys.argv[2])
    else:
        main()
