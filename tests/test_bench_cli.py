"""bench.py's command line: `--steps` sets the timed steps of every workload, a plain run prints
the headline line only, `--full` adds the roofline / check / baseline sections, and
`--dump-outputs DIR` writes the last timed step's outputs (here against the oracle's counts)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._golden import Oracle
from vcfx_amd import REPO, synth

BENCH = os.path.join(REPO, "bench.py")
SMALL = ["--records", "300", "--samples", "2504"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "kernels_ms", "output_check", "e2e", "cpu_baseline")


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_steps_option_sets_timed_steps(monkeypatch):
    assert _parse([], monkeypatch).steps == 20
    assert _parse(["--workload", "ld"], monkeypatch).steps == 3
    assert _parse(["--workload", "ld", "--steps", "20"], monkeypatch).steps == 20
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "2"], monkeypatch)
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(["--full", "--dump-outputs", "d"], monkeypatch)
    assert a.full and a.dump_outputs == "d"


def _run(args):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + args, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_outputs(tmp_path):
    d = str(tmp_path / "dump")
    out = _run(SMALL + ["--steps", "2", "--warmup", "1", "--dump-outputs", d])
    for k in HEADLINE:
        assert k in out, k
    assert not [k for k in FULL_ONLY if k in out]
    assert out["steps"] == 2 and out["unit"] == "records/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(300 / (out["ms_per_step"] * 1e-3), rel=1e-9)
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["alt", "status", "summary", "text", "tot"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    # bench.input_params: the rank-0 shard of these arguments
    buf = synth.generate(300, 2504, 20251226)
    ralt, rtot = Oracle().af_counts(buf)
    rows = got["status"] == 1
    assert rows.sum() == 300 == got["summary"][1]
    assert np.array_equal(got["alt"][rows], ralt) and np.array_equal(got["tot"][rows], rtot)
    assert got["text"].size == got["summary"][4] and got["text"][-1] == 10


@pytest.mark.gpu
def test_full_run_keeps_the_sections():
    out = _run(SMALL + ["--steps", "2", "--warmup", "1", "--full", "--no-e2e", "--cpu-seconds", "0.1"])
    for k in HEADLINE + ("roofline", "kernels_ms", "output_check", "cpu_baseline"):
        assert k in out, k
    assert out["roofline"]["kernel"] in out["kernels_ms"]
