"""The context's environment-knob reader (vcfxg_env.h: env_u64, env_i64, env_set) without a device:
tests/env_knobs_test.cpp is a program of its own, built with the header under ASan + UBSan.  Unset gives
the default as it stands (not clamped); a value below lo or above hi clamps; text that is no number
reads as strtoull / atoll read it (0, or the leading digits), and a minus sign wraps in the unsigned
reader as strtoull's does."""
import os
import subprocess

from vcfx_amd import BUILD, REPO

U64_MAX, I64_MIN, I64_MAX = 2 ** 64 - 1, -2 ** 63, 2 ** 63 - 1


def read(cases, env):
    exe = os.path.join("build", "san", "env_knobs_asan")
    subprocess.check_call(["make", "-s", "-C", REPO, exe])
    assert os.path.dirname(os.path.join(REPO, exe)) == os.path.join(BUILD, "san")
    e = {k: v for k, v in os.environ.items() if not k.startswith("KNOB_")}
    e.update(env, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, exe)], input="".join(" ".join(str(x) for x in c) + "\n" for c in cases).encode(),
                       capture_output=True, env=e, timeout=120)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    out = [int(x) for x in r.stdout.split()]
    assert len(out) == len(cases)
    return out


def test_unset_gives_the_default():
    # (the default is not clamped: VCFXG_LD_STAGE_CAP's 0 lies below every other knob's lo)
    assert read([("u64", "KNOB_A", 65536, 1, 1 << 24), ("u64", "KNOB_A", 0, 1, 9), ("i64", "KNOB_A", 16, I64_MIN, I64_MAX),
                 ("i64", "KNOB_A", 131072, 4096, 8 << 20), ("set", "KNOB_A")], {}) == [65536, 0, 16, 131072, 0]


def test_values_clamp_to_lo_and_hi():
    env = {"KNOB_LOW": "0", "KNOB_IN": "7", "KNOB_HIGH": "99999999999", "KNOB_NEG": "-5"}
    assert read([("u64", "KNOB_LOW", 65536, 1, 1 << 24), ("u64", "KNOB_IN", 65536, 1, 1 << 24),
                 ("u64", "KNOB_HIGH", 65536, 1, 1 << 24), ("u64", "KNOB_HIGH", 512 << 20, 1, U64_MAX),
                 ("i64", "KNOB_LOW", 131072, 4096, 8 << 20), ("i64", "KNOB_HIGH", 131072, 4096, 8 << 20),
                 ("i64", "KNOB_NEG", 131072, 4096, 8 << 20), ("i64", "KNOB_NEG", 0, I64_MIN, I64_MAX),
                 ("set", "KNOB_LOW")], env) == [1, 7, 1 << 24, 99999999999, 4096, 8 << 20, 4096, -5, 1]


def test_text_that_is_no_number_reads_as_the_c_library_reads_it():
    env = {"KNOB_TEXT": "fast", "KNOB_EMPTY": "", "KNOB_LEAD": "12abc", "KNOB_NEG": "-1"}
    assert read([("u64", "KNOB_TEXT", 65536, 1, 1 << 24), ("u64", "KNOB_TEXT", 5, 0, U64_MAX),
                 ("u64", "KNOB_EMPTY", 5, 0, U64_MAX), ("u64", "KNOB_LEAD", 5, 0, U64_MAX),
                 ("u64", "KNOB_NEG", 5, 0, U64_MAX), ("u64", "KNOB_NEG", 65536, 1, 1 << 24),
                 ("i64", "KNOB_TEXT", 3, I64_MIN, I64_MAX), ("i64", "KNOB_LEAD", 3, I64_MIN, I64_MAX),
                 ("set", "KNOB_EMPTY")], env) == [1, 0, 0, 12, U64_MAX, 1 << 24, 0, 12, 1]
