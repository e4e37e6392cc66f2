"""The sliced word-table build without a device: lx_index_plan_slices -- how LX_OPT_INDEX_SLICE_WORDS cuts a prefix table into
slices -- against a restatement of its rule, its invariants and its refusals; and the front end's --table-slice, which is refused
before any file is looked at.

The rule (include/lambda_ext.h): the buckets are walked in order with one running slice; a bucket joins it if the slice still has
no words or if its words plus the bucket's do not exceed N, otherwise the slice closes and the bucket opens the next one.  Empty
buckets need two remarks.  They join a slice that has no words yet, so the empty buckets in front of a bucket larger than N share
its slice: "no slice of two or more buckets exceeds N" can only be meant of buckets that hold words, and is checked so.  And behind
a slice that is full the rule alone would leave the table's last empty buckets as a slice without words; the library joins them to
the slice before, which keeps "every slice has a word"."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi


def plan(pre, n):
    """first bucket of every slice"""
    first, words = [0], 0
    for w in range(len(pre) - 1):
        c = int(pre[w + 1]) - int(pre[w])
        if words and words + c > n:
            first.append(w)
            words = 0
        words += c
    if len(first) > 1 and words == 0:  # empty buckets behind a full slice
        first.pop()
    return first


def _pre(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.uint64))]).astype(np.uint64)


def _check(pre, n):
    got = capi.index_plan_slices(pre, n).astype(int).tolist()
    assert got == plan(pre, n), (pre.tolist()[:20], n)
    ends = got[1:] + [len(pre) - 1]
    # the slices partition the buckets in order
    assert got[0] == 0 and all(a < b for a, b in zip(got, ends)) and ends[-1] == len(pre) - 1
    total = int(pre[-1])
    for k, (a, b) in enumerate(zip(got, ends)):
        words = int(pre[b]) - int(pre[a])
        assert words >= 1 or total == 0, (got, n)  # every slice but an empty table's has a word
        if words > n:  # only a single bucket may exceed N (empty buckets beside it hold nothing)
            assert sum(1 for w in range(a, b) if int(pre[w + 1]) > int(pre[w])) == 1, (got, n)
    return got


def test_plan_on_random_tables(lx_lib):
    rng = np.random.default_rng(7)
    for trial in range(200):
        nb = int(rng.integers(1, 60))
        counts = rng.integers(0, 50, nb) * (rng.random(nb) < 0.7)
        pre = _pre(counts)
        total = int(pre[-1])
        for n in {1, 2, 7, 49, 50, 120, max(1, total - 1), max(1, total), total + 1}:
            _check(pre, n)


def test_plan_on_the_named_tables(lx_lib):
    assert _check(np.zeros(9, np.uint64), 5) == [0]  # an empty table: one slice without words
    assert _check(_pre([1000]), 10) == [0]  # one bucket holds everything
    assert _check(_pre([0, 0, 1000, 0, 0]), 10) == [0]  # ... between empty ones
    assert _check(_pre([3, 4, 100, 2, 5]), 10) == [0, 2, 3]  # a bucket larger than N between small ones
    assert _check(_pre([3, 4, 100, 0, 0, 2, 5]), 10) == [0, 2, 3]  # (empty buckets behind it open the next slice)
    assert _check(_pre([3, 4, 100, 0, 0]), 10) == [0, 2]  # (... unless nothing follows them)
    assert _check(_pre([1, 0, 2, 1]), 1) == [0, 2, 3]  # N = 1
    assert _check(_pre([1, 1, 1]), 1) == [0, 1, 2]
    counts = [5, 0, 7, 3, 0, 9]  # total 24
    assert _check(_pre(counts), 23) == [0, 5]
    assert _check(_pre(counts), 24) == [0]
    assert _check(_pre(counts), 25) == [0]
    assert _check(_pre([0, 0, 0, 4, 4, 4, 0, 0]), 8) == [0, 5]  # leading and trailing empty buckets
    assert _check(_pre([0, 0, 0, 4, 4, 0, 0]), 8) == [0]


def _raw(lx_lib, pre, n_prefix, n, first, cap, count):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return lx_lib.lx_index_plan_slices(p(pre), n_prefix, n, p(first), cap, None if count is None else C.byref(count))


def test_plan_refusals(lx_lib):
    pre, count, first = _pre([3, 4, 5]), C.c_uint64(77), np.zeros(8, np.uint64)
    assert _raw(lx_lib, None, 4, 5, first, 8, count) == capi.LX_EINVAL and count.value == 0
    assert _raw(lx_lib, pre, 4, 5, first, 8, None) == capi.LX_EINVAL
    assert _raw(lx_lib, pre, 4, 5, None, 8, count) == capi.LX_EINVAL
    assert _raw(lx_lib, pre, 4, 0, first, 8, count) == capi.LX_EINVAL  # slices of no words
    assert _raw(lx_lib, pre, 1, 5, first, 8, count) == capi.LX_EINVAL and _raw(lx_lib, pre, 0, 5, first, 8, count) == capi.LX_EINVAL
    assert _raw(lx_lib, np.array([0, 5, 4, 9], np.uint64), 4, 5, first, 8, count) == capi.LX_EINVAL  # descends
    # a bucket of 2^31 words is beyond the sort (two numbers, no memory behind them); 2^31 - 1 is not
    assert _raw(lx_lib, np.array([0, 2 ** 31], np.uint64), 2, 2 ** 40, first, 8, count) == capi.LX_EINVAL and count.value == 0
    assert b"h == NULL" in lx_lib.lx_last_output_error()
    assert _raw(lx_lib, np.array([7, 7 + 2 ** 31], np.uint64), 2, 1, first, 8, count) == capi.LX_EINVAL
    assert _raw(lx_lib, np.array([0, 2 ** 31 - 1], np.uint64), 2, 1, first, 8, count) == capi.LX_OK and count.value == 1
    assert _raw(lx_lib, np.array([0, 2 ** 31 - 1, 2 ** 32 - 2], np.uint64), 3, 2 ** 31 - 1, first, 8, count) == capi.LX_OK and count.value == 2


def test_plan_with_too_little_room_writes_the_count_only(lx_lib):
    pre, count = _pre([3, 4, 100, 2, 5]), C.c_uint64(0)
    first = np.full(8, 99, np.uint64)
    assert _raw(lx_lib, pre, len(pre), 10, first, 2, count) == capi.LX_OK and count.value == 3
    assert (first == 99).all()
    assert _raw(lx_lib, pre, len(pre), 10, None, 0, count) == capi.LX_OK and count.value == 3
    assert _raw(lx_lib, pre, len(pre), 10, first, 3, count) == capi.LX_OK and first.tolist() == [0, 2, 3, 99, 99, 99, 99, 99]


def test_the_option_is_declared():
    assert capi.LX_OPT_INDEX_SLICE_WORDS == 18


@pytest.mark.parametrize("args", [["--table-slice", "0"], ["--table-slice", "x"], ["--table-slice", "-3"], ["--table-slice", "12x"], ["--table-slice"]])
def test_front_end_refuses_a_bad_table_slice_before_any_file(tmp_path, args):
    r = subprocess.run([str(build.build_cli()), "searchp", "-q", "no/such/query.fasta", "-d", "no/such/db.fasta", "-o", str(tmp_path / "o.m8"), *args],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--table-slice" in r.stderr and "no/such" not in r.stderr, r.stderr
