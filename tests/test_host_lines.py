"""The drop-ins' shared reader (vcfx_amd/csrc/host/emit.h: Lines, LineSource, LineWalk and the
range helpers) without a device: tests/host_lines_test.cpp over the host stand-in for the device
library, built plain and under ASan + UBSan by `make sanitize`, each a process of its own.  Every
line, status and range of every input form (host-resident, shard view, device-only) must equal a
plain split of the bytes on '\\n' -- at a 16-byte and a 1024-byte read-back window (the window
moves within and between lines) and at the default one."""
import os
import subprocess

import pytest

from vcfx_amd import BUILD, REPO

SAN = os.path.join(BUILD, "san")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-j8", "-C", REPO, os.path.join("build", "san", "host_lines"),
                           os.path.join("build", "san", "host_lines_asan")])
    return SAN


@pytest.mark.parametrize("window", ["16", "1024", None])
@pytest.mark.parametrize("kind", ["host_lines", "host_lines_asan"])
def test_shared_reader_against_a_plain_split(built, kind, window):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    env.pop("VCFX_WINDOW_BYTES", None)
    if window:
        env["VCFX_WINDOW_BYTES"] = window
    r = subprocess.run([os.path.join(built, kind)], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    out = r.stdout.decode().split()
    assert out[0] == "ok" and int(out[1]) > 1000000
