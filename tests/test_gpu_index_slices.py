"""The word table built on the device in slices of the key space (LX_OPT_INDEX_SLICE_WORDS = N): the same table as the host's entry
for entry and byte for byte, with as many timed launches as the rule of tests/test_index_slices.py cuts slices from the host
table's prefix table; the single sort's limits unchanged without the option; the refusals of the sliced build and of a load;
seeding on a sliced table; the front end's --table-slice.  The handle is the session's: every test puts the option back to 0."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests import level3_cases as L3
from tests.test_cli import _fasta
from tests.test_gpu_level3 import SORT_TILE, _both, _case, _params
from tests.test_index_slices import plan

pytestmark = pytest.mark.gpu


def _sliced(handle, n, *args):
    handle.set_option(capi.LX_OPT_INDEX_SLICE_WORDS, n)
    try:
        assert handle.get_option(capi.LX_OPT_INDEX_SLICE_WORDS) == n
        return capi.Index.build(handle, *args)
    finally:
        handle.set_option(capi.LX_OPT_INDEX_SLICE_WORDS, 0)


def _prefix_table(ix):
    info = ix.info()
    return np.frombuffer(ix.save()[-8 * info.n_prefix:], "<u8")


def _sizes(pre, n):
    first = plan(pre, n)
    return [int(pre[b]) - int(pre[a]) for a, b in zip(first, first[1:] + [len(pre) - 1])]


def _same_table(handle, host, n, red, off, lens, alph):
    """the sliced build with slices of n words against the host-made index `host`; returns the number of slices"""
    want = len(plan(_prefix_table(host), n))
    with _sliced(handle, n, red, off, lens, alph) as dev:
        hi, di = host.info(), dev.info()
        assert (di.built_on_device, hi.built_on_device) == (1, 0)
        assert (di.n_entries, di.n_prefix, di.alph, di.key_len, di.prefix_len) == (hi.n_entries, hi.n_prefix, hi.alph, hi.key_len, hi.prefix_len)
        assert dev.entries().tobytes() == host.entries().tobytes()
        assert dev.save() == host.save()  # (the prefix table too)
    ms, launches = handle.last_phase_ms(8)
    assert launches == want and ms > 0, (launches, want, n)
    return want


@pytest.mark.parametrize("alph", [10, 4, 3])
def test_sliced_table_equals_host_table(handle, alph):
    args = (*L3.table_inputs(alph), alph)
    total = int(args[2].sum())
    with capi.Index.build(None, *args) as host:
        for slices in (2, 5, 16):
            got = _same_table(handle, host, -(-total // slices), *args)
            assert slices <= got <= slices + 3, (slices, got)
        assert _same_table(handle, host, total, *args) == 1  # one slice: still the sliced code
        assert _same_table(handle, host, 2 ** 40, *args) == 1


@pytest.mark.parametrize("total", [1, 255, 256, 257, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
def test_sliced_table_at_the_block_and_tile_edges(handle, total):
    rng = np.random.default_rng(total)
    # three sequences (the middle one empty) that hold `total` letters, as one slice (its size on the edge) and as several
    lens = np.array([total // 3, 0, total - total // 3], np.uint64)
    off, lens = L3.offsets(lens)
    args = (rng.integers(0, 10, total).astype(np.uint8), off, lens, 10)
    with capi.Index.build(None, *args) as host:
        assert _same_table(handle, host, total, *args) == 1
        assert _same_table(handle, host, total // 3 + 1, *args) <= 8


@pytest.mark.parametrize("edge,prefix_len", [(256, 2), (SORT_TILE, 3)])
def test_slices_of_exactly_the_block_and_the_sort_tile(handle, edge, prefix_len):
    """Three sequences of one letter each: the words of prefix_len equal letters fill buckets of edge, edge - 1 and edge + 1 words, the
    pads behind them buckets of one.  With N = edge - 1, edge, edge + 1 one slice holds exactly N words (255 / 256 / 257: the block of
    the table's kernels; SORT_TILE - 1 / SORT_TILE / SORT_TILE + 1: a tile of the sort), others one or two, and at N = edge - 1 two exceed N."""
    lens = np.array([edge, edge - 1, edge + 1], np.uint64) + np.uint64(prefix_len - 1)
    off, lens = L3.offsets(lens)
    args = (np.repeat(np.array([0, 1, 2], np.uint8), lens.astype(int)), off, lens, 10)
    with capi.Index.build(None, *args) as host:
        assert host.info().prefix_len == prefix_len
        pre = _prefix_table(host)
        for n in (edge - 1, edge, edge + 1):
            sizes = _sizes(pre, n)
            assert n in sizes, (n, sizes)
            assert _same_table(handle, host, n, *args) == len(sizes) <= 9
        assert max(_sizes(pre, edge - 1)) == edge + 1


def test_a_hot_bucket_far_beyond_the_slice(handle):
    # 100 000 equal letters: one word for all but the last positions -- a wavefront's run is one atomic --, a single slice of 100x N
    lens = np.array([100000], np.uint64)
    args = (np.full(100000, 7, np.uint8), np.zeros(1, np.uint64), lens, 10)
    with capi.Index.build(None, *args) as host:
        sizes = _sizes(_prefix_table(host), 1000)
        assert len(sizes) == 2 and sizes[0] > 99000
        assert _same_table(handle, host, 1000, *args) == 2


def test_equal_words_keep_the_hosts_order_across_a_cut(handle):
    # 64 copies of one sequence: every word occurs 64 times, ordered by sequence; a cut falls directly behind such a bucket
    rng = np.random.default_rng(11)
    one = rng.integers(0, 4, 300).astype(np.uint8)
    off, lens = L3.offsets(np.full(64, 300))
    args = (np.tile(one, 64), off, lens, 4)
    with capi.Index.build(None, *args) as host:
        pre = _prefix_table(host)
        n = int(pre[np.searchsorted(pre, 300 * 64 // 4)])  # the words of whole buckets: the first slice is full to the last word
        sizes = _sizes(pre, n)
        assert sizes[0] == n and n % 64 == 0 and 3 <= len(sizes) <= 8, sizes
        assert _same_table(handle, host, n, *args) == len(sizes)
        rows = host.entries()
        same = rows["key"][1:] == rows["key"][:-1]
        assert same.sum() >= 63 * 280 and (rows["seq"][1:][same] > rows["seq"][:-1][same]).all()


def test_sequences_shorter_than_the_key(handle):
    rng = np.random.default_rng(3)
    lens = rng.integers(1, L3.key_len(10), 50)  # pads in every key
    off, lens = L3.offsets(lens)
    total = int(lens.sum())
    args = (rng.integers(0, 10, total).astype(np.uint8), off, lens, 10)
    with capi.Index.build(None, *args) as host:
        assert 3 <= _same_table(handle, host, total // 4, *args) <= 8


def _build_raw(handle, lens, n_red=16):
    out, red = C.c_void_p(), np.zeros(n_red, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = handle.lib.lx_index_build(handle.h, p(red), p(np.zeros(len(lens), np.uint64)), p(lens), len(lens), 10, 0, C.byref(out))
    assert not out.value
    return rc, handle.lib.lx_last_error(handle.h)


def test_the_single_sort_keeps_its_limit(handle):
    assert handle.get_option(capi.LX_OPT_INDEX_SLICE_WORDS) == 0
    rc, text = _build_raw(handle, np.array([2 ** 30, 2 ** 30, 8], np.uint64))
    assert rc == capi.LX_EINVAL and b"h == NULL" in text and b"2^31" in text


def test_the_sliced_build_refuses_what_a_device_cursor_cannot_name(handle):
    handle.set_option(capi.LX_OPT_INDEX_SLICE_WORDS, 2 ** 30)
    try:
        # 2^32 - 1 words: refused on the lengths alone, before a letter is read (there are 16)
        rc, text = _build_raw(handle, np.array([2 ** 31, 2 ** 31 - 1], np.uint64))
        assert rc == capi.LX_EINVAL and b"32-bit" in text and b"cursor" in text and b"h == NULL" in text
    finally:
        handle.set_option(capi.LX_OPT_INDEX_SLICE_WORDS, 0)


def test_a_load_is_not_held_to_the_sorts_limit(handle):
    # 2^31 + 8 words and the 32 bytes of a table's header: refused as truncated (on the header alone, before a letter is read), no longer
    # as beyond the device
    lens = np.array([2 ** 30, 2 ** 30, 8], np.uint64)
    table = np.array([10, 18, 3, 0], "<i4").tobytes() + np.array([2 ** 31 + 8, 11 ** 3 + 1], "<u8").tobytes()
    buf, red, out = np.frombuffer(table, np.uint8), np.zeros(16, np.uint8), C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = handle.lib.lx_index_load(handle.h, p(buf), len(table), p(red), p(np.zeros(3, np.uint64)), p(lens), 3, C.byref(out))
    text = handle.lib.lx_last_error(handle.h)
    assert rc == capi.LX_EINVAL and not out.value and b"truncated" in text and b"beyond the device" not in text


def test_seeding_on_a_sliced_table_equals_the_host_path(handle):
    c = _case("nucleotide", 200)
    args = (c["s_red"], c["s_off"], c["s_len"], c["alph"])
    with _sliced(handle, int(c["s_len"].sum()) // 5, *args) as dev_ix, capi.Index.build(None, *args) as host_ix:
        assert handle.last_phase_ms(8)[1] >= 5
        total = 0
        for half_exact in (True, False):
            for adaptive in (True, False):
                for pre_scoring in (0, 2):
                    d, st = _both(handle, dev_ix, host_ix, c, _params(c, half_exact=half_exact, adaptive=adaptive, pre_scoring=pre_scoring, pre_scoring_thresh=2.0))
                    assert (st.reads_declined, st.launches_full) == (0, 0), (half_exact, adaptive, pre_scoring)
                    total += st.n_matches
        assert total >= 300


def _run(cwd, *args):
    return subprocess.run([str(build.build_cli()), *map(str, args)], capture_output=True, text=True, cwd=cwd, timeout=120)


def test_front_end_table_slice(tmp_path):
    rng = np.random.default_rng(5)
    genome = ["".join("ACGT"[i] for i in rng.integers(0, 4, 6000)) for _ in range(3)]
    reads = []
    for k in range(60):
        c, a = int(rng.integers(0, 3)), int(rng.integers(0, 5800))
        r = list(genome[c][a:a + 150])
        for p in rng.integers(0, 150, 4):
            r[p] = "ACGT"[int(rng.integers(0, 4))]
        reads.append("".join(r))
    _fasta(tmp_path / "g.fasta", [f"chr{i}" for i in range(3)], genome)
    _fasta(tmp_path / "r.fasta", [f"read{k} x" for k in range(60)], reads)
    base = ["searchn", "-q", "r.fasta", "-d", "g.fasta", "--version-to-outputfile", "0"]
    host = _run(tmp_path, *base, "--table", "host", "-o", "host.m8")
    assert host.returncode == 0 and "slices" not in host.stderr, host.stderr
    gpu = _run(tmp_path, *base, "--table", "gpu", "--table-slice", 5000, "-o", "gpu.m8")
    assert gpu.returncode == 0, gpu.stderr
    want = (tmp_path / "host.m8").read_bytes()
    assert len(want.splitlines()) >= 40 and (tmp_path / "gpu.m8").read_bytes() == want
    m = re.search(r"reduce \+ word table \(on the GPU in (\d+) slices\)", gpu.stderr)
    assert m and 3 <= int(m.group(1)) <= 16, gpu.stderr
    one = _run(tmp_path, *base, "--table", "gpu", "-o", "one.m8")  # without the option: one sort, the line as it was
    assert one.returncode == 0 and "reduce + word table (on the GPU) " in one.stderr and (tmp_path / "one.m8").read_bytes() == want
    host = _run(tmp_path, "mkindexn", "-d", "g.fasta", "-i", "host.lba", "--table", "host")
    gpu = _run(tmp_path, "mkindexn", "-d", "g.fasta", "-i", "gpu.lba", "--table", "gpu", "--table-slice", 5000)
    assert host.returncode == 0 and gpu.returncode == 0, (host.stderr, gpu.stderr)
    assert re.search(r"reduce \+ word table \d+ \(on the GPU in (\d+) slices\)", gpu.stderr), gpu.stderr
    assert (tmp_path / "gpu.lba").read_bytes() == (tmp_path / "host.lba").read_bytes()
