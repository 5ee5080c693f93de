"""The host-only code of VCFX_fasta_converter (vcfx_amd/csrc/tools/fa_host.h: the sample names of a
"#CHROM" line and the row layout of the device text) without a device: tests/host_fa_test.cpp, a
program of its own built under ASan + UBSan, and the same header lines through the Python
restatement."""
import os
import re
import subprocess

from tests import _fasta_converter_ref as R
from vcfx_amd import BUILD, REPO


def test_host_code_under_asan_and_ubsan():
    exe = os.path.join("build", "san", "host_fa_asan")
    subprocess.check_call(["make", "-s", "-C", REPO, exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, exe)], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    out = r.stdout.decode().split()
    assert out[0] == "ok" and int(out[1]) >= 30
    assert os.path.dirname(os.path.join(REPO, exe)) == os.path.join(BUILD, "san")


def test_the_program_and_the_restatement_read_chrom_lines_alike():
    """the cases of the program's table, as the restatement reads them"""
    src = open(os.path.join(REPO, "tests", "host_fa_test.cpp")).read()
    rows = re.findall(r'^        \{"((?:[^"\\]|\\.)*)", \{(.*)\}\},$', src.split("const Case cases[] = {")[1].split("};")[0], re.M)
    assert len(rows) >= 12
    for tail, names in rows:
        line = R.COLS + tail.encode().decode("unicode_escape").encode()
        want = [n.encode().decode("unicode_escape").encode() for n in re.findall(r'"((?:[^"\\]|\\.)*)"', names)]
        assert R.header_names(line) == want, (tail, names)


def test_row_layout_is_the_wrapped_sequence():
    for cols in (0, 1, 59, 60, 61, 120, 121):
        assert len(R.wrap(b"A" * cols)) == cols + (cols + R.LINE - 1) // R.LINE
