"""The host-only code of VCFX_multiallelic_splitter (vcfx_amd/csrc/tools/ms_host.h: the ##INFO /
##FORMAT table of the header and the walk that interleaves the lines the host copies with the rows
the device wrote) without a device: tests/host_ms_test.cpp, a program of its own built under
ASan + UBSan, and the same header lines through the Python restatement."""
import os
import subprocess

from tests import _multiallelic_splitter_ref as R
from vcfx_amd import BUILD, REPO


def test_host_code_under_asan_and_ubsan():
    exe = os.path.join("build", "san", "host_ms_asan")
    subprocess.check_call(["make", "-s", "-C", REPO, exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, exe)], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    out = r.stdout.decode().split()
    assert out[0] == "ok" and int(out[1]) > 150
    assert os.path.dirname(os.path.join(REPO, exe)) == os.path.join(BUILD, "san")


def test_the_program_and_the_restatement_read_header_lines_alike():
    """the cases of the program's table, as the restatement reads them"""
    src = open(os.path.join(REPO, "tests", "host_ms_test.cpp")).read()
    rows = [ln.strip() for ln in src.split("const Case cases[] = {")[1].split("};")[0].splitlines() if ln.strip()]
    assert len(rows) >= 30
    numbers = {"VCFXG_MS_NUM_A": R.NUM_A, "VCFXG_MS_NUM_R": R.NUM_R, "VCFXG_MS_NUM_G": R.NUM_G, "VCFXG_MS_NUM_OTHER": R.NUM_OTHER}
    for row in rows:
        rest = row.rstrip('},').split(', ')
        line = row[2:row.index('", true' if '", true' in row else '", false')]
        line = line.replace('\\"', '"').replace("\\r", "\r").encode()
        got = R.parse_header_line(line)
        if '", false' in row:
            assert got is None, row
        else:
            ident = row.split('", true, "')[1].split('"')[0].encode()
            assert got is not None and got[0] == ident, row
            assert got[1] == (R.FORMAT if "VCFXG_MS_FORMAT" in row else R.INFO), row
            assert R.NUMBERS.get(got[2], R.NUM_OTHER) == numbers[rest[-1].strip()], row
