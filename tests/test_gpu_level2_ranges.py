"""The multi-range path of the Level-2 driver (lx_level2_host.cpp) on small lists.  By itself a call cuts its window list into ranges
from 300 000 windows on -- each range planned by itself, swept as one chunk of the pipeline, its records made behind its chunk and
flushed in order (RecordsJob), the per-query cut of lx_iterate_matches_dev_top made range by range.  The library's environment switch
LX_L2_RANGES forces a range count on any list; it is read once per process, so every setting runs tests/level2_ranges_case.py in a
process of its own (the four side by side).  Whatever the count, rows, alignment columns and both statistics structs must be the bytes
that the one range gives which these lists take by themselves."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.level2_ranges_case import LISTS, LONG_QUERY
from tests.test_level2_plan import cuts, probe_targets

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SETTINGS = (None, 2, 3, 8)
KEYS = ("rows", "ops", "stats", "top.rows", "top.ops", "top.stats", "top.record_stats")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("level2_ranges")
    procs = {}
    for setting in SETTINGS:
        env = dict(os.environ, LX_HOST_TIMING="1")
        env.pop("LX_L2_RANGES", None)
        if setting:
            env["LX_L2_RANGES"] = str(setting)
        out = tmp / f"ranges_{setting}.npz"
        procs[setting] = (out, subprocess.Popen([sys.executable, str(ROOT / "tests" / "level2_ranges_case.py"), str(out)], stdout=subprocess.PIPE,
                                                stderr=subprocess.PIPE, text=True, env=env))
    got = {}
    for setting, (out, p) in procs.items():
        _, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-2000:]
        # the ranges of every lx_iterate_matches_dev* call, list by list: the marks between two "list NAME done" lines
        ranges, at = {}, 0
        for name in LISTS:
            end = err.index(f"list {name} done", at)
            ranges[name] = [int(x) for x in re.findall(r"extension \+ records \(range by range\), (\d+) ranges", err[at:end])]
            at = end
        got[setting] = (np.load(out), ranges)
    return got


def expected_ranges(window_query, forced):
    """What the range plan (tests/test_level2_plan.py restates it) makes of this window list."""
    R = min(forced, 8) if forced else 1
    return len(cuts(window_query.tolist(), probe_targets(len(window_query), R), 1)) - 1


@pytest.mark.parametrize("name", LISTS)
def test_forced_ranges_give_the_bytes_of_one_range(runs, name):
    one, one_ranges = runs[None]
    wq = one[f"{name}.window_query"]
    # what the case needs of its list -- from the device's own window list, not from the generator
    assert 5_000 < len(wq) < 30_000 and (np.diff(wq.astype(np.int64)) >= 0).all()
    per_query = np.bincount(wq.astype(np.int64))
    assert "sweep_mq_kernel" in str(one[f"{name}.kernel"])  # (the multi-query sweep over a device plan: the solo packing or the free packing)
    assert len(one[f"{name}.rows"]) > 128 * 1000 and len(one[f"{name}.ops"]) > 0 and 0 < len(one[f"{name}.top.rows"]) <= len(one[f"{name}.rows"])
    if name == "long_query":
        # one query holds more than 600 windows, and the probe around the 66 % mark lies inside them
        first = int(np.searchsorted(wq, LONG_QUERY)), int(np.searchsorted(wq, LONG_QUERY, side="right"))
        ((_, lo, hi),) = probe_targets(len(wq), 2)
        assert per_query[LONG_QUERY] > 600 and first[0] < lo and hi <= first[1]
        assert expected_ranges(wq, 2) == 1  # the forced 2 quietly gives one range
        assert len(one[f"{name}.top.rows"]) < len(one[f"{name}.rows"])  # (the cut has something to cut)
    else:
        assert per_query.max() < 64 and [expected_ranges(wq, f) for f in (2, 3, 8)] == [2, 3, 8]
    assert one_ranges[name] == [1, 1]  # lx_iterate_matches_dev, lx_iterate_matches_dev_top: one range each
    for forced in SETTINGS[1:]:
        got, got_ranges = runs[forced]
        assert (got[f"{name}.window_query"] == wq).all()
        assert got_ranges[name] == [expected_ranges(wq, forced)] * 2, (forced, got_ranges[name])
        for k in KEYS:
            a, b = one[f"{name}.{k}"], got[f"{name}.{k}"]
            assert a.shape == b.shape and (a == b).all(), (forced, k)
