"""The host-only code of VCFX_diff_tool (vcfx_amd/csrc/tools/df_host.h: the two files as the one text
the device indexes, the walk over a side's text blocks) without a device: tests/host_df_test.cpp, a
program of its own built under ASan + UBSan, and the same joins through the Python restatement."""
import os
import re
import subprocess

from tests import _diff_tool_ref as R
from vcfx_amd import BUILD, REPO


def test_host_code_under_asan_and_ubsan():
    exe = os.path.join("build", "san", "host_df_asan")
    subprocess.check_call(["make", "-s", "-C", REPO, exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, exe)], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    out = r.stdout.decode().split()
    assert out[0] == "ok" and int(out[1]) >= 100
    assert os.path.dirname(os.path.join(REPO, exe)) == os.path.join(BUILD, "san")


def test_the_program_and_the_restatement_join_alike():
    """the plain cases of the program's table, as the restatement joins them"""
    src = open(os.path.join(REPO, "tests", "host_df_test.cpp")).read()
    rows = re.findall(r'^        \{"((?:[^"\\]|\\.)*)", "((?:[^"\\]|\\.)*)", "((?:[^"\\]|\\.)*)", (\d+), (\d)\},$',
                      src.split("const Case cases[] = {")[1].split("};")[0], re.M)
    assert len(rows) >= 10
    for a, b, text, second, _ in rows:
        a, b, text = (x.encode().decode("unicode_escape").encode("latin-1") for x in (a, b, text))
        assert R.join(a, b) == (text, int(second)), (a, b)
