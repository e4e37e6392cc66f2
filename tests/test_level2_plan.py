"""The Level-2 range planner (lambda_amd/csrc/lx_level2_plan.h), without a GPU and without the library: tests/native/level2_plan_check.cpp,
built with g++ under AddressSanitizer and UBSan, answers requests on its standard input with what the header's functions give.  This
file restates the rule -- how many ranges a window list is cut into, where the cuts are looked for, where they fall -- and holds the
program against the restatement and, for the named cases, against figures worked out by hand."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

MAX_RANGES = 8       # lx::kFpMaxRanges
PROBE = 512          # lxi::kL2ProbeWindows
GIB = 1 << 30


# ---- the restatement
def ranges_by_size(n):
    return 1 if n < 300_000 else min(4, n // 4_000_000 + 2)


def need_bytes(n, slot_bytes):
    return (n + n // 8) * (slot_bytes // 2 + 1)


def range_count(n, records_on_device, forced, need, have):
    if not records_on_device:
        return 1
    if forced:
        return min(forced, MAX_RANGES)
    return min(MAX_RANGES, max(ranges_by_size(n), -(-need // have)))


def probe_targets(n, R):
    out = []
    for k in range(1, R):
        target = n // 100 * 66 if R == 2 else n * k // R
        lo, hi = max(target - PROBE // 2, 0), min(n, target + PROBE // 2)
        if hi - lo >= 2 and (not out or lo >= out[-1][2]) and len(out) < MAX_RANGES:
            out.append((target, lo, hi))
    return out


def cuts(q, probes, q_frames):
    n, bounds = len(q), [0]
    for target, lo, hi in probes:
        at = next((w for w in range(max(target, lo + 1), hi) if q[w] // q_frames != q[w - 1] // q_frames), 0)
        if at and bounds[-1] < at < n:
            bounds.append(at)
    return bounds + [n]


def runs_of(q):
    runs = []
    for v in q:
        if runs and runs[-1][1] == v:
            runs[-1][0] += 1
        else:
            runs.append([1, v])
    return runs


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = tmp_path_factory.mktemp("level2_plan") / "level2_plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{ROOT / 'lambda_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "level2_plan_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(requests):
        r = subprocess.run([str(exe)], input="".join(q + "\n" for q in requests), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(requests)
        return lines

    return run


def ask_counts(ask, cases):
    got = [int(x) for x in ask([f"count {n} {int(rod)} {forced} {need} {have}" for n, rod, forced, need, have in cases])]
    assert got == [range_count(*c) for c in cases]
    return got


def ask_probes(ask, n, R):
    (line,) = ask([f"probes {n} {R}"])
    got = [] if line == "-" else [tuple(int(x) for x in p.split(":")) for p in line.split()]
    assert got == probe_targets(n, R), (n, R)
    return got


def ask_cuts(ask, q, probes, q_frames=1):
    runs = runs_of(q)
    req = f"cuts {len(q)} {q_frames} {len(probes)} " + " ".join(f"{t} {a} {b}" for t, a, b in probes) + f" {len(runs)} " + " ".join(f"{c} {v}" for c, v in runs)
    got = [int(x) for x in ask([req])[0].split()]
    assert got == cuts(q, probes, q_frames)
    return got


def test_the_constants_are_the_restatements(ask):
    assert ask(["consts"]) == [f"{MAX_RANGES} {PROBE}"]


def test_the_range_count_by_size(ask):
    sizes = (0, 1, 299_999, 300_000, 3_999_999, 4_000_000, 8_000_000, 12_000_000, 2_000_000_000)
    got = ask_counts(ask, [(n, True, 0, 0, 8 * GIB) for n in sizes])
    assert got == [1, 1, 1, 2, 2, 3, 4, 4, 4]


def test_a_forced_count_and_records_on_the_host(ask):
    # forced: taken as it is whatever the size and the memory say, 64 clamped to what the plan kernels take
    got = ask_counts(ask, [(n, True, f, need, GIB) for n in (1000, 5_000_000) for f in (1, 2, 64) for need in (0, 100 * GIB)])
    assert got == [1, 1, 2, 2, 8, 8] * 2
    # records on the host threads: one range always
    got = ask_counts(ask, [(n, False, f, need, GIB) for n in (1000, 300_000, 12_000_000) for f in (0, 3, 64) for need in (0, 100 * GIB)])
    assert set(got) == {1}


def test_the_memory_rule_raises_the_count_and_is_capped(ask):
    n, slot = 1_000_000, 40_000
    (need,) = [int(x) for x in ask([f"need {n} {slot}"])]
    assert need == need_bytes(n, slot) == 1_125_000 * 20_001
    got = ask_counts(ask, [(n, True, 0, need, have) for have in (64 * GIB, 8 * GIB, need // 2, need // 2 - 1, 1 << 28, 1)])
    # 22.5 GB of slots: two ranges by size where they fit, three in 8 GiB, two / three around the half, at most eight
    assert got == [2, 3, 2, 3, 8, 8]
    # a small list that the size rule leaves whole is cut as well where its slots do not fit
    assert ask_counts(ask, [(1000, True, 0, 10 * GIB + 1, 5 * GIB), (1000, True, 0, 10 * GIB, 5 * GIB)]) == [3, 2]
    assert [int(x) for x in ask(["need 0 7", "need 7 0", "need 8 3"])] == [0, 7, 18]


def test_probe_targets(ask):
    assert ask_probes(ask, 1_000_000, 2) == [(660_000, 659_744, 660_256)]  # two ranges: the first one 66 %
    assert ask_probes(ask, 1_234_567, 2) == [(814_770, 814_514, 815_026)]  # (n / 100 * 66: of whole hundredths)
    assert ask_probes(ask, 900_000, 3) == [(300_000, 299_744, 300_256), (600_000, 599_744, 600_256)]
    assert len(ask_probes(ask, 12_000_000, 8)) == 7
    # eight ranges over 600 windows: every probe behind the first would overlap it and is dropped
    assert ask_probes(ask, 600, 8) == [(75, 0, 331)]
    assert ask_probes(ask, 1, 2) == [] and ask_probes(ask, 2, 2) == [(0, 0, 2)] and ask_probes(ask, 0, 2) == []
    assert ask_probes(ask, 1, 8) == [] and ask_probes(ask, 2, 8) == [(0, 0, 2)]
    assert ask_probes(ask, 1_000_000, 1) == [] and ask_probes(ask, 1_000_000, 0) == []
    for n in (3, 511, 512, 513, 1023, 1024, 1025, 4096, 100_000):
        for R in range(2, 9):
            ask_probes(ask, n, R)


def test_cuts_around_the_target(ask):
    n, target = 3000, 1980  # 3000 / 100 * 66
    probes = probe_targets(n, 2)
    assert probes == [(target, target - 256, target + 256)]
    two = lambda at: [0] * at + [1] * (n - at)
    assert ask_cuts(ask, two(target), probes) == [0, target, n]          # a query boundary exactly at the target
    assert ask_cuts(ask, two(target + 1), probes) == [0, target + 1, n]  # one window behind it
    assert ask_cuts(ask, two(target + 255), probes) == [0, target + 255, n]
    assert ask_cuts(ask, two(target + 256), probes) == [0, n]            # (behind the probe)
    assert ask_cuts(ask, two(target - 1), probes) == [0, n]              # only in front of the target: the range merges with the next
    # the nearest of several, and only those at or behind the target
    assert ask_cuts(ask, [w // 100 for w in range(n)], probes) == [0, 2000, n]
    # the probe lies inside one query of more than 512 windows
    assert ask_cuts(ask, [0] * 1700 + [1] * 600 + [2] * 700, probes) == [0, n]
    # two frames per query: 10 -> 11 is a frame change of query 5, 11 -> 12 the next query
    assert ask_cuts(ask, [10] * target + [11] * (n - target), probes, 2) == [0, n]
    assert ask_cuts(ask, [10] * target + [11] * 20 + [12] * (n - target - 20), probes, 2) == [0, target + 20, n]
    assert ask_cuts(ask, [10] * target + [11] * 20 + [12] * (n - target - 20), probes, 1) == [0, target, n]


def test_cuts_of_tiny_lists_and_of_probes_that_agree(ask):
    assert ask_cuts(ask, [0, 1], probe_targets(2, 2)) == [0, 1, 2]
    assert ask_cuts(ask, [0, 0], probe_targets(2, 2)) == [0, 2]
    assert ask_cuts(ask, [0], []) == [0, 1]
    # two probes that find the same cut: the second one's does not lie behind the first one's and is dropped
    q = [0] * 200 + [1] * 400
    assert ask_cuts(ask, q, [(100, 0, 300), (150, 50, 350)]) == [0, 200, 600]
    # three ranges whose middle one lies inside one long query: two ranges come of it
    n = 9000
    probes = probe_targets(n, 3)
    q = [w // 50 for w in range(3300)] + [66] * 3500 + [67 + w // 50 for w in range(n - 6800)]
    assert ask_cuts(ask, q, probes) == [0, 3000, n] and probes[1][0] == 6000
    # a cut at the list's last window is one, at its end none
    assert ask_cuts(ask, [0] * 599 + [1], [(590, 334, 600)]) == [0, 599, 600]


def test_cuts_agree_with_the_restatement_on_generated_lists(ask):
    import numpy as np

    rng = np.random.default_rng(11)
    for _ in range(40):
        n, R, qf = int(rng.integers(2, 6000)), int(rng.integers(2, 9)), int(rng.integers(1, 4))
        lens = rng.integers(1, int(rng.choice([4, 40, 900])) + 1, n)
        q = np.repeat(np.arange(len(lens)), lens)[:n].tolist()
        ask_cuts(ask, q, ask_probes(ask, n, R), qf)


def test_the_strip_geometry(ask):
    # the answer is the strips' columns per lane, 19 / 13 / 11: narrower strips must save 15 %
    got = [int(x) for x in ask(["cfg 100 100 100", "cfg 114 100 100", "cfg 116 100 100", "cfg 116 100 99", "cfg 1000 800 500", "cfg 0 0 0", "cfg 100 86 87", "cfg 100 87 86"])]
    assert got == [19, 19, 13, 11, 11, 19, 13, 11]
