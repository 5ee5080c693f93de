"""The host-only code of VCFX_field_extractor (vcfx_amd/csrc/tools/fx_host.h: the --fields split, the
field forms of both modes, the S<n> check, the names, the table builder) without a device:
tests/host_fx_test.cpp, a program of its own built under ASan + UBSan, and the tables it prints against
the Python restatement's."""
import os
import re
import subprocess

from tests import _field_extractor_ref as R
from vcfx_amd import BUILD, REPO


def run_program():
    exe = os.path.join("build", "san", "host_fx_asan")
    subprocess.check_call(["make", "-s", "-C", REPO, exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, exe)], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert os.path.dirname(os.path.join(REPO, exe)) == os.path.join(BUILD, "san")
    return r.stdout.decode().split("\n")


def test_host_code_under_asan_and_ubsan():
    out = run_program()
    last = out[-2].split()
    assert last[0] == "ok" and int(last[1]) >= 60


def test_the_program_and_the_restatement_build_the_same_tables():
    src = open(os.path.join(REPO, "tests", "host_fx_test.cpp")).read()
    lst = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', src.split("kList[] =")[1].split(";")[0])).encode().decode("unicode_escape")
    hdr = re.search(r'kHeader\[\] = "((?:[^"\\]|\\.)*)";', src).group(1).encode().decode("unicode_escape").encode()
    fields = lst.split(",")
    assert len(fields) == 27 and "last\r:GT" in fields and R.bad_field(fields) is None
    out = run_program()
    for stdin in (False, True):
        names, _ = R.names_of(hdr + b"\n", True)  # (the program is given the line as it stands, '\r' and all)
        assert names[b"last\r"] == 14 and names[b"dup"] == 13 and names[b""] == 12
        cols, pool = R.table(fields, names, stdin)
        got = [tuple(int(x) for x in ln.split()[2:]) for ln in out if ln.startswith("T %d " % int(stdin))]
        assert got == cols, [(f, g, c) for f, g, c in zip(fields, got, cols) if g != c]
        hexpool = [ln.split()[2] if len(ln.split()) > 2 else "" for ln in out if ln.startswith("P %d" % int(stdin))]
        assert bytes.fromhex(hexpool[0]) == pool
