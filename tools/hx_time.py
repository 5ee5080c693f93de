"""Diagnostics: VCFX_haplotype_extractor's device passes on an input of the bench width (2,504 samples,
phased "a|b" records generated here: tests/_haplotype_extractor_ref.py bench_input, a pool of records
repeated under POS values 100 apart), device-resident, file mode.  Three runs: FORMAT GT at the default
block size (neighbours are closer than it: one block), FORMAT GT with -b 5 (one-member blocks), FORMAT GT:AD:DP at the
default (no line is fixed-stride: every member holds a row of the cell matrix).  Per run the passes hx_scan, hx_number, hx_segment, hx_layout, hx_heads, hx_emit by device
events (summed per call, median of five calls after two warm-ups) and the three calls by a host clock.
Beside them, in the same process:
    (a) the read floor: vcfxg_count_byte over the same bytes;
    (b) k_fa_transpose's bytes/s on the same sample count (VCFX_fasta_converter on the GT input): the
        in-project yardstick for a transpose through LDS;
    (c) carried over from an existing profiles/hx_bench.json: the compiled reference's wall time on the
        same file on a CPU host (tools/hx_time.py --reference BIN; the reference is not part of this
        repository).
Algorithmic bytes per pass (M members, G of them with a matrix row, S samples, B blocks, I input bytes,
X text bytes, 8-byte cells; DESIGN "Haplotype extraction"):
    hx_scan    I read, 8 G S written
    hx_layout  16 G S read (the tiles walked twice), 32 (M / 32) S for the tile sums and carries, 32 B S for
               the totals and their scan
    hx_emit    8 G S + the GT bytes (3 M S for "a|b") + 8 B S read, X written
Writes profiles/hx_bench.json."""
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
from tests import _fasta_converter_ref as FA  # noqa: E402
from tests import _haplotype_extractor_ref as R  # noqa: E402

RECORDS = int(os.environ.get("HX_TIME_RECORDS", 100000))
SAMPLES = 2504
RUNS = (("GT_default", b"GT", 100000), ("GT_one_member_blocks", b"GT", 5), ("GT_AD_DP_default", b"GT:AD:DP", 100000))
KERNELS = ("hx_scan", "hx_number", "hx_segment", "hx_layout", "hx_heads", "hx_emit")
PATH = os.path.join(REPO, "profiles", "hx_bench.json")


def reference(binary):
    """the compiled reference on the same inputs, file mode, output to /dev/null: wall seconds"""
    res = {"host": "%s, %d CPUs" % (os.uname().machine, os.cpu_count()),
           "what": "VCFX_haplotype_extractor [-b T] -i FILE > /dev/null, wall time, median of 3 after 1 warm-up",
           "records": RECORDS}
    for name, fmt, T in RUNS:
        with tempfile.NamedTemporaryFile(suffix=".vcf") as f:
            f.write(R.bench_input(fmt, RECORDS, SAMPLES))
            f.flush()
            t = []
            for _ in range(4):
                t0 = time.perf_counter()
                subprocess.check_call([binary, "-b", str(T), "-i", f.name], stdout=subprocess.DEVNULL)
                t.append(time.perf_counter() - t0)
            res[name] = {"seconds": round(med(t[1:]), 3), "GBps_in": round(os.path.getsize(f.name) / med(t[1:]) / 1e9, 3)}
    old = json.load(open(PATH)) if os.path.exists(PATH) else {}
    old["reference_cpu"] = res
    with open(PATH, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1))


def fasta_yardstick(engine_mod, eng, start, n):
    """k_fa_transpose on the same bytes and sample count: (bytes, median ms)"""
    import numpy as np
    cols = [0]

    def scan_run():
        l0, c = 0, 0
        while l0 < n:
            s = engine_mod.Summary()
            eng._chk(eng.L.vcfxg_fasta_scan(eng.h, l0, n, engine_mod.MODE_FILE, SAMPLES, s), "fasta_scan")
            l0 += s.n_lines
            c += s.rows
        cols[0] = c
    scan_run()
    V = cols[0]
    row = V + (V + FA.LINE - 1) // FA.LINE
    row_off = np.arange(SAMPLES + 1, dtype=np.uint64) * np.uint64(row)
    eng.fasta_begin(SAMPLES * row)

    def fasta_run():
        l0, c = 0, 0
        while l0 < n:
            s = eng.fasta(l0, n, SAMPLES, c, V, row_off)
            l0 += s.n_lines
            c += s.rows
    k, _ = timed(eng, fasta_run, ("fa_transpose",))
    pitch = (SAMPLES + 15) & ~15
    return pitch * V + SAMPLES * row, k["fa_transpose"]["median_ms"]


def main():
    import ctypes

    from vcfx_amd import engine as engine_mod
    out = {"shape": {"samples": SAMPLES, "records": RECORDS}, "warmup_calls": WARM, "timed_calls": REPS,
           "hbm_peak_GBps": HBM_PEAK_GBS,
           "how": "kernel figures: device events around each pass, summed per run, median of the timed runs; run "
                  "figures: host clock around scan + blocks + text (three host synchronisations in the scan and the "
                  "layout; the text is not fetched), profiling off; all figures measured, none estimated",
           "clocks_before": clocks()}
    eng = engine_mod.Engine(0)
    res, bufs = {}, {}
    for name, fmt, T in RUNS:
        if fmt not in bufs:
            bufs = {fmt: R.bench_input(fmt, RECORDS, SAMPLES)}
        buf = bufs[fmt]
        start = buf.index(b"\n", buf.index(b"#CHROM")) + 1
        in_bytes = len(buf) - start
        eng.load(buf)
        n = eng.index(start)
        cnt = [0]

        def stream():
            cnt[0] = eng.count_byte(start, 10)
        k, w = timed(eng, stream, ("count_byte",))
        stream_gbps = in_bytes / k["count_byte"]["median_ms"] / 1e6
        tot = [0, 0, 0, 0]

        def run():
            p = engine_mod.HxParams(engine_mod.MODE_FILE, SAMPLES, T, 0)
            s = engine_mod.Summary()
            eng._chk(eng.L.vcfxg_haplotype_scan(eng.h, ctypes.byref(p), s), "haplotype_scan")
            m, g = int(s.rows), int(s.general_records)
            eng._chk(eng.L.vcfxg_haplotype_blocks(eng.h, s), "haplotype_blocks")
            eng._chk(eng.L.vcfxg_haplotype_text(eng.h, s), "haplotype_text")
            tot[:] = [m, int(s.rows), int(s.text_bytes), g]
        kh, wh = timed(eng, run, KERNELS)
        M, B, text, G = tot
        assert M == RECORDS == n
        head = eng.text_range(0, min(text, 60))
        MS, GS, BS = M * SAMPLES, G * SAMPLES, B * SAMPLES
        algo = {"hx_scan": in_bytes + 8 * GS, "hx_layout": 16 * GS + MS + 32 * BS, "hx_emit": 8 * GS + 3 * MS + 8 * BS + text}
        entry = {
            "lines": int(n), "members": M, "matrix_rows": G, "blocks": B, "bytes_read": in_bytes, "text_bytes": text,
            "first_row_head": head.decode("latin-1"), "kernels": kh, "call": wh,
            "kernels_ms": round(sum(kh[x]["median_ms"] for x in KERNELS), 3),
            "read_floor": {"kernels": k, "call": w, "GBps": round(stream_gbps, 1), "newlines": int(cnt[0])},
            "passes": {p: {"bytes": b, "ms": kh[p]["median_ms"], "GBps": round(b / kh[p]["median_ms"] / 1e6, 1),
                           "stream_time_over_time": round((b / stream_gbps / 1e6) / kh[p]["median_ms"], 3),
                           "peak_time_over_time": round((b / HBM_PEAK_GBS / 1e6) / kh[p]["median_ms"], 3)}
                       for p, b in algo.items()},
        }
        if name == "GT_default":
            fb, fms = fasta_yardstick(engine_mod, eng, start, n)
            entry["fa_transpose_yardstick"] = {"bytes": fb, "ms": fms, "GBps": round(fb / fms / 1e6, 1)}
        res[name] = entry
    out["runs"] = res
    eng.close()
    out["clocks_after"] = clocks()
    if os.path.exists(PATH):
        with open(PATH) as f:
            old = json.load(f)
        if "reference_cpu" in old:
            out["reference_cpu"] = old["reference_cpu"]
    with open(os.environ.get("HX_TIME_OUT", PATH), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--reference":
        reference(sys.argv[2])
    else:
        main()
