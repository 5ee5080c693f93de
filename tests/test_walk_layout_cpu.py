"""The record walk's chunk layout (vcfxg_walk_layout.h, the one function the kernel, the host's plan
and this test share) without a device: tests/walk_layout_test.cpp is a program of its own, built
with the header under ASan + UBSan; for each case it prints the layout and every walker's bytes as
walk_range gives them to the kernel.  Checked here, over a few thousand seeded cases that vary the
region, C, the divisor, K1 and so the grid (grids of 1-9 blocks, K1 = 0, 1 and the last round,
regions shorter than one chunk): the walkers' ranges tile [lo, hi) exactly in file order, no gap and
no overlap; the file order is a bijection of the hardware blocks; short walkers are dispatched in
the rounds from K1 on; the walkers past `nw`, and only they, own nothing; and the one-segment
layout is lo + wk * C."""
import os
import random
import subprocess

from vcfx_amd import BUILD, REPO

WAVES = 4


def run_cases(lines):
    exe = os.path.join("build", "san", "walk_layout_asan")
    subprocess.check_call(["make", "-s", "-C", REPO, exe])
    assert os.path.dirname(os.path.join(REPO, exe)) == os.path.join(BUILD, "san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REPO, exe)], input="".join(s + "\n" for s in lines).encode(),
                       capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    out, cur = [], None
    for ln in r.stdout.decode().splitlines():
        f = ln.split()
        if f[0] == "layout":
            v = [int(x) for x in f[1:]]
            cur = dict(kind=v[0], C=v[1], Cs=v[2], K1=v[3], grid=v[4], nw=v[5], base=v[6:], walkers=[])
        elif f[0] == "end":
            out.append(cur)
        else:
            cur["walkers"].append(tuple(int(x) for x in f))
    assert len(out) == len(lines)
    return out


def check_tiling(case, lay, lo, hi, xcd):
    w = lay["walkers"]
    grid, nw, K1 = lay["grid"], lay["nw"], lay["K1"]
    assert len(w) == grid * WAVES, case
    by_file = sorted(w, key=lambda t: t[2])
    assert [t[2] for t in by_file] == list(range(grid * WAVES)), case  # a bijection
    at = lo
    for blk, wv, wk, cs, ce, size in by_file:
        assert cs == at and cs <= ce <= hi, (case, wk)  # no gap, no overlap
        assert (cs < ce) == (wk < nw), (case, wk)       # exactly the first nw own bytes
        k = blk // 8 if xcd else blk
        assert size == (lay["C"] if K1 < 0 or k < K1 else lay["Cs"]), (case, wk)
        assert ce - cs == size or ce == hi, (case, wk)
        at = ce
    assert at == hi, case
    assert (hi > lo) == (grid > 0) and (grid - 1) * WAVES < nw <= grid * WAVES or grid == 0, case
    if xcd:  # XCD-contiguous: the blocks of one XCD (b mod 8) are one run of the file
        for x in range(8):
            ks = [t[2] // WAVES for t in w if t[0] % 8 == x and t[1] == 0]
            assert ks == list(range(ks[0], ks[0] + len(ks))) if ks else True, case
        firsts = [min(t[2] for t in w if t[0] % 8 == x) for x in range(min(8, grid))]
        assert firsts == sorted(firsts), case


def make_cases():
    rng = random.Random(4245)
    cases = []
    for i in range(3000):
        C = 16 * rng.randint(1, 40)
        div = rng.choice([1, 2, 3, 4, 8])
        Cs = max(C // div & ~15, 16)
        shape = i % 6
        if shape == 0:    # grids of 1-9 blocks
            R = rng.randint(1, 9 * WAVES * C)
        elif shape == 1:  # shorter than one chunk
            R = rng.randint(1, C)
        else:
            R = rng.randint(1, 90 * WAVES * C)
        lo = rng.choice([0, 1, 15, 16, 4097, rng.randint(0, 1 << 20)])
        rounds = -(-R // (8 * WAVES * C))  # of the uniform grid
        K1 = rng.choice([0, 1, max(rounds - 1, 0), rounds, rng.randint(0, rounds + 1), -1])
        xcd = 0 if i % 17 == 0 else 1
        cases.append((lo, lo + R, C, Cs, K1, xcd))
    # the far end of a large region (offsets past 2^32)
    cases.append((5 << 30, (5 << 30) + 33 * WAVES * 131072 + 77, 131072, 32768, 0, 1))
    cases.append((5 << 30, (5 << 30) + 33 * WAVES * 131072 + 77, 131072, 32768, 1, 1))
    return cases


def test_ranges_tile_the_region_in_file_order():
    cases = make_cases()
    lays = run_cases(["make %d %d %d %d %d %d %d" % (lo, hi, C, Cs, K1, WAVES, xcd) for lo, hi, C, Cs, K1, xcd in cases])
    small_grids, last_round, first_round, sub_chunk = set(), 0, 0, 0
    for case, lay in zip(cases, lays):
        lo, hi, C, Cs, K1, xcd = case
        check_tiling(case, lay, lo, hi, xcd)
        assert (lay["C"], lay["Cs"], lay["K1"]) == (C, Cs, K1)
        small_grids.add(lay["grid"])
        rounds = -(-lay["grid"] // 8)
        last_round += xcd and K1 == rounds - 1 and any(t[5] == Cs for t in lay["walkers"]) and Cs < C
        first_round += K1 == 0
        sub_chunk += hi - lo < C
        if K1 < 0 or Cs == C:  # one segment: today's ranges, bit for bit
            for blk, wv, wk, cs, ce, size in lay["walkers"]:
                if wk < lay["nw"]:
                    assert (cs, ce) == (lo + wk * C, min(lo + (wk + 1) * C, hi)), (case, wk)
            assert lay["nw"] == -(-(hi - lo) // C)
    assert set(range(1, 10)) <= small_grids
    assert last_round > 20 and first_round > 100 and sub_chunk > 100


def test_empty_region():
    lay, = run_cases(["make 100 100 4096 1024 1 4 1"])
    assert lay["grid"] == 0 and lay["nw"] == 0 and not lay["walkers"]


def test_plans_fit_whole_generations_and_taper_the_last():
    rng = random.Random(8005)
    cases = []
    for i in range(600):
        C0 = 16 * rng.randint(4, 64)
        S = WAVES * rng.choice([1, 2, 3, 8, 16, 40, 64])
        R = rng.randint(1, 12 * S * C0)
        knob = rng.choice(["uniform", "fit", "taper:2:1", "taper:4:1", "taper:4:2", "taper:3:9", "split:2:1"])
        cases.append((rng.randint(0, 5000), R, C0, S, knob))
    # the bench shard's shape: 20 walkers past eight generations of 4,096
    cases.append((4096, 32788 * 131072 - 5000, 131072, 4096, "fit"))
    lays = run_cases(["plan %d %d %d %d %s %d 1" % (lo, lo + R, C0, S, knob, WAVES) for lo, R, C0, S, knob in cases])
    kinds = {"uniform": 1, "fit": 2, "taper": 3, "split": 4}
    for case, lay in zip(cases, lays):
        lo, R, C0, S, knob = case
        if len(lay["walkers"]) < 5000:
            check_tiling(case, lay, lo, lo + R, 1)
        nw0 = -(-R // C0)
        G = nw0 // S
        name = knob.split(":")[0]
        if name in ("uniform", "split") or G < 1:  # under one generation: uniform
            want = 4 if name == "split" else 1
            assert lay["kind"] == want and lay["C"] == C0, case
            if want == 1:
                assert lay["nw"] == nw0 and lay["K1"] == -1, case
            continue
        assert lay["kind"] == kinds[name], case
        div = int(knob.split(":")[1]) if name == "taper" else 1
        unit = 16 * div
        C = lay["C"]
        # the least C >= C0 (a multiple of 16 * div) with which G generations cover the region
        assert C >= C0 and C % unit == 0 and G * S * C >= R, case
        assert C - unit < C0 or G * S * (C - unit) < R, case
        if name == "fit":
            assert lay["K1"] == -1 and lay["nw"] <= G * S and lay["nw"] > (G - 1) * S, case
        else:
            g = min(int(knob.split(":")[2]), G)
            assert lay["Cs"] == C // div and lay["K1"] == (G - g) * (S // WAVES) // 8, case
    assert lays[-1]["nw"] == 8 * 4096 and lays[-1]["grid"] == 8 * 1024 and lays[-1]["C"] > 131072


def test_knob_spellings_that_do_not_parse_are_the_default():
    bad = ["tape", "taper", "taper:2", "taper:0:1", "taper:2:1:3", "taper:x:1", "fit:2", "uniformly", "split:65:1"]
    lays = run_cases(["plan 0 1000000 4096 16 %s %d 1" % (k, WAVES) for k in bad])
    for lay in lays:  # (kLayoutDefault reaches walk_layout_plan only here: it plans the uniform layout)
        assert lay["kind"] == 1 and lay["C"] == 4096 and lay["K1"] == -1
