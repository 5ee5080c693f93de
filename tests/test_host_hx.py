"""The host-only code of VCFX_haplotype_extractor (vcfx_amd/csrc/tools/hx_host.h: std::stoi for -b, the
header-line rule, the names, the GT spans, the warning and debug texts) without a device:
tests/host_hx_test.cpp, a program of its own built under ASan + UBSan, and its std::stoi table through
the Python restatement."""
import os
import re
import subprocess

from tests import _haplotype_extractor_ref as R
from vcfx_amd import BUILD, REPO


def test_host_code_under_asan_and_ubsan():
    exe = os.path.join("build", "san", "host_hx_asan")
    subprocess.check_call(["make", "-s", "-C", REPO, exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, exe)], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    out = r.stdout.decode().split()
    assert out[0] == "ok" and int(out[1]) >= 50
    assert os.path.dirname(os.path.join(REPO, exe)) == os.path.join(BUILD, "san")


def test_the_program_and_the_restatement_parse_b_alike():
    """the program's std::stoi table, as the restatement parses it"""
    src = open(os.path.join(REPO, "tests", "host_hx_test.cpp")).read()
    rows = re.findall(r'^        \{"((?:[^"\\]|\\.)*)", (\d), (-?\d+)(?: - 1)?\},$',
                      src.split("const Stoi cases[] = {")[1].split("};")[0], re.M)
    assert len(rows) >= 18
    for text, ok, value in rows:
        text = text.encode().decode("unicode_escape")
        got = R.stoi(text)
        assert (got is not None) == (ok == "1"), text
        if got is not None and text != "-2147483648":
            assert got == int(value), text
    assert R.stoi("-2147483648") == -2147483648
