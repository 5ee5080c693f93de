"""The host-only code of VCFX_merger (vcfx_amd/csrc/tools/mg_host.h: the K files as the one text the
device indexes, the split of -m values, the walk over the text blocks) without a device:
tests/host_mg_test.cpp, a program of its own built under ASan + UBSan, and the same joins and splits
through the Python restatement."""
import os
import re
import subprocess

from tests import _merger_ref as R
from vcfx_amd import BUILD, REPO


def unescape(x):
    return x.encode().decode("unicode_escape").encode("latin-1")


def test_host_code_under_asan_and_ubsan():
    exe = os.path.join("build", "san", "host_mg_asan")
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
    src = open(os.path.join(REPO, "tests", "host_mg_test.cpp")).read()
    rows = re.findall(r'^        \{\{((?:"(?:[^"\\]|\\.)*"(?:, )?)*)\}, "((?:[^"\\]|\\.)*)", \{([\d, ]*)\}, (\d+)\},$',
                      src.split("const Case cases[] = {")[1].split("\n    };")[0], re.M)
    assert len(rows) >= 12
    for files, text, starts, _ in rows:
        files = [unescape(f) for f in re.findall(r'"((?:[^"\\]|\\.)*)"', files)]
        assert R.join(files) == (unescape(text), [int(x) for x in starts.split(",")]), files


def test_the_program_and_the_restatement_split_alike():
    src = open(os.path.join(REPO, "tests", "host_mg_test.cpp")).read()
    rows = re.findall(r'^        \{"([^"]*)", \{((?:"[^"]*"(?:, )?)*)\}\},$', src.split("const Split splits[] = {")[1].split("\n    };")[0], re.M)
    assert len(rows) >= 8
    for value, names in rows:
        assert R.split_names([value]) == re.findall(r'"([^"]*)"', names), value
