"""The host-only code of VCFX_region_subsampler (vcfx_amd/csrc/tools/rs_host.h: the BED loader and
its own sort_and_merge) without a device: tests/host_rs_test.cpp, a program of its own built under
ASan + UBSan, and the same BED texts through the Python restatement."""
import os
import re
import subprocess

from tests import _region_subsampler_ref as R
from vcfx_amd import BUILD, REPO


def test_host_code_under_asan_and_ubsan():
    exe = os.path.join("build", "san", "host_rs_asan")
    subprocess.check_call(["make", "-s", "-C", REPO, exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, exe)], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    out = r.stdout.decode().split()
    assert out[0] == "ok" and int(out[1]) >= 100
    assert os.path.dirname(os.path.join(REPO, exe)) == os.path.join(BUILD, "san")


def show(bed):
    names, ivs, warn = R.load_bed(bed)
    fmt = lambda rows: b" ".join(b"%s:%d-%d" % (names[i], s, e) for i, s, e in rows)  # noqa: E731
    return fmt(ivs) + b"|" + fmt(R.merged(ivs)), warn.count(b"Warning: skipping invalid bed line ")


def test_the_program_and_the_restatement_load_alike():
    """the program's case table, as the restatement loads and merges it"""
    src = open(os.path.join(REPO, "tests", "host_rs_test.cpp")).read()
    rows = re.findall(r'^        \{"((?:[^"\\]|\\.)*)", "((?:[^"\\]|\\.)*)", (\d+)\},$',
                      src.split("const Case cases[] = {")[1].split("};")[0], re.M)
    assert len(rows) >= 30
    for bed, want, warnings in rows:
        bed, want = (x.encode().decode("unicode_escape").encode("latin-1") for x in (bed, want))
        assert show(bed) == (want, int(warnings)), bed
