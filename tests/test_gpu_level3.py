"""Level 3 on the device: the word table made by kernels against the host-made one, lx_seed_queries on a handle against the host
path (h == NULL) as sorted match lists with equal counters -- on inputs the kernel serves alone, on inputs it must decline, on a
read with many hits --, the device list handed to lx_iterate_matches_dev_top without a copy, and the lifetimes of indexes and
results.  The host path itself is checked against brute force in tests/test_level3_abi.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import level3_cases as L3
from tests.test_oracle import SCHEMES

pytestmark = pytest.mark.gpu

SORT_TILE = 256 * 16  # lx_level2.h: kL2SortBlock * kL2SortItems keys per tile of the radix sort


def _hip_runtime():
    """the HIP runtime this process already has (the one the library is bound to), for a copy the ABI has no call for"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def _same_table(handle, red, off, lens, alph):
    with capi.Index.build(None, red, off, lens, alph) as host, capi.Index.build(handle, red, off, lens, alph) as dev:
        hi, di = host.info(), dev.info()
        assert (di.built_on_device, hi.built_on_device) == (1 if lens.sum() else 0, 0)
        assert (di.n_entries, di.n_prefix, di.alph, di.key_len, di.prefix_len) == (hi.n_entries, hi.n_prefix, hi.alph, hi.key_len, hi.prefix_len)
        assert dev.entries().tobytes() == host.entries().tobytes()
        assert dev.save() == host.save()  # (the prefix table too)
    if lens.sum():
        ms, launches = handle.last_phase_ms(8)
        assert launches == 1 and ms > 0


@pytest.mark.parametrize("alph", [10, 4, 3])
def test_device_table_equals_host_table(handle, alph):
    _same_table(handle, *L3.table_inputs(alph), alph)


@pytest.mark.parametrize("total", [1, 255, 256, 257, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
def test_device_table_at_the_block_and_tile_edges(handle, total):
    rng = np.random.default_rng(total)
    # three sequences (the middle one empty) that hold `total` letters: 256 is the block of the table's kernels, SORT_TILE a tile of the sort
    lens = np.array([total // 3, 0, total - total // 3], np.uint64)
    off, lens = L3.offsets(lens)
    _same_table(handle, rng.integers(0, 10, total).astype(np.uint8), off, lens, 10)


def test_device_table_limits(handle):
    # 2^31 words are beyond the device build: LX_EINVAL with a text before any device work (the lengths alone say so)
    lens = np.array([2 ** 30, 2 ** 30, 8], np.uint64)
    out = C.c_void_p()
    red = np.zeros(16, np.uint8)
    rc = handle.lib.lx_index_build(handle.h, red.ctypes.data_as(C.c_void_p), np.zeros(3, np.uint64).ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), 3, 10, 0, C.byref(out))
    assert rc == capi.LX_EINVAL and b"h == NULL" in handle.lib.lx_last_error(handle.h)


MODES = {"protein": ("blosum62", None, 10), "translated": ("blosum62", None, 10), "nucleotide": ("nucl", None, 14), "bisulfite": ("bs_fwd", "bs_rev", 17)}
# (rng seeds of the inputs, checked on the CPU with the host path: every mode finds hundreds of promising seeds at 63 reads and more,
# and the most frequent key_len-word of the subjects -- a sequence's last letter and its padding -- occurs 11 times, far from the 32 a
# device cursor holds)
CASE_SEEDS = {"protein": 101, "translated": 102, "nucleotide": 103, "bisulfite": 104}
_cases = {}


def _case(mode, n_reads):
    if (mode, n_reads) not in _cases:
        _cases[(mode, n_reads)] = L3.make_case(mode, n_reads, CASE_SEEDS[mode])
    return _cases[(mode, n_reads)]


def _params(c, **kw):
    fwd, rev, sl = MODES[c["mode"]]
    base = dict(seed_length=sl, seed_offset=max(3, sl // 2), max_seed_dist=1, q_num_frames=c["frames"], unknown_rank=c["unknown"], max_matches=256,
                matrix_rev=None if rev is None else SCHEMES[rev].matrix_np())
    base.update(kw)
    return capi.seed_params(SCHEMES[fwd].matrix_np(), **base)


def _both(handle, dev_ix, host_ix, c, p, reads=None):
    q = (c["q_res"], c["q_red"], c["q_off"], c["q_len"])
    d = capi.seed_queries(handle, dev_ix, c["s_res"], *q, p, reads=reads)
    h = capi.seed_queries(None, host_ix, c["s_res"], *q, p, reads=reads)
    ds, hs = d.stats, h.stats
    assert (ds.n_matches, ds.hits_after_seeding, ds.hits_failed_pre_extend) == (hs.n_matches, hs.hits_after_seeding, hs.hits_failed_pre_extend)
    assert d.dev() is not None and h.dev() is None
    assert np.array_equal(L3.sorted_matches(d.matches()), L3.sorted_matches(h.matches()))
    return d, ds


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("mode", list(MODES))
def test_seeding_on_the_device_equals_the_host_path(handle, mode, n_reads):
    c = _case(mode, n_reads)
    assert L3.max_word_count(c) <= 32  # the inputs must exercise the kernel, not the host completion
    total = 0
    with capi.Index.build(handle, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as dev_ix, capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as host_ix:
        for half_exact in (True, False):
            for adaptive in (True, False):
                for pre_scoring in (0, 2):
                    p = _params(c, half_exact=half_exact, adaptive=adaptive, pre_scoring=pre_scoring, pre_scoring_thresh=2.0)
                    d, st = _both(handle, dev_ix, host_ix, c, p)
                    assert (st.reads_declined, st.launches_full) == (0, 0), (half_exact, adaptive, pre_scoring)
                    total += st.n_matches
        d, st = _both(handle, dev_ix, host_ix, c, _params(c, max_seed_dist=0))  # exact seeds
        assert (st.reads_declined, st.launches_full) == (0, 0)
        ms, launches = handle.last_phase_ms(9)
        assert launches == 1 and ms > 0
        if n_reads >= 63:
            assert total >= 300 and st.n_matches >= 20, (total, st.n_matches)
            _both(handle, dev_ix, host_ix, c, _params(c), reads=np.array([40, 2, 17], np.uint64) * c["frames"])


def test_reads_the_device_declines_are_finished_inside_the_call(handle):
    """40 identical subjects of 60 letters and reads of the same sequence: every key_len-word occurs 40 > 32 times, so a cursor that
    adaptive seeding elongates beyond the key length must decline its read."""
    rng = np.random.default_rng(7)
    one = synth.STD20[rng.integers(0, 20, 60)].astype(np.uint8)
    s_off, s_len = L3.offsets([60] * 40)
    others = [synth.STD20[rng.integers(0, 20, 45)].astype(np.uint8) for _ in range(6)]
    seqs = [one, others[0], one[5:50], *others[1:]]
    q_off, q_len = L3.offsets([len(x) for x in seqs])
    c = dict(mode="protein", alph=10, frames=1, unknown=25, s_res=np.tile(one, 40), s_red=L3.LI10[np.tile(one, 40)], s_off=s_off, s_len=s_len,
             q_res=np.concatenate(seqs), q_red=L3.LI10[np.concatenate(seqs)], q_off=q_off, q_len=q_len)
    assert L3.max_word_count(c) == 40
    with capi.Index.build(handle, c["s_red"], s_off, s_len, 10) as dev_ix, capi.Index.build(None, c["s_red"], s_off, s_len, 10) as host_ix:
        d, st = _both(handle, dev_ix, host_ix, c, _params(c, adaptive=True, max_seed_dist=0, max_matches=10))
        assert st.reads_declined >= 1 and st.n_matches >= 40
        # ... and with the subjects resident on the handle instead of handed in (the host threads fetch them for the declined reads)
        handle.set_subjects(c["s_res"])
        r = capi.seed_queries(handle, dev_ix, None, c["q_res"], c["q_red"], q_off, q_len, _params(c, adaptive=True, max_seed_dist=0, max_matches=10))
        assert r.stats.reads_declined == st.reads_declined and np.array_equal(L3.sorted_matches(r.matches()), L3.sorted_matches(d.matches()))


def _identical_subjects(copies):
    """the construction of the test above with `copies` identical subjects: every key_len-word occurs `copies` times"""
    rng = np.random.default_rng(7)
    one = synth.STD20[rng.integers(0, 20, 60)].astype(np.uint8)
    s_off, s_len = L3.offsets([60] * copies)
    others = [synth.STD20[rng.integers(0, 20, 45)].astype(np.uint8) for _ in range(6)]
    seqs = [one, others[0], one[5:50], *others[1:]]
    q_off, q_len = L3.offsets([len(x) for x in seqs])
    return dict(mode="protein", alph=10, frames=1, unknown=25, s_res=np.tile(one, copies), s_red=L3.LI10[np.tile(one, copies)], s_off=s_off,
                s_len=s_len, q_res=np.concatenate(seqs), q_red=L3.LI10[np.concatenate(seqs)], q_off=q_off, q_len=q_len)


@pytest.mark.parametrize("copies", [32, 33])
def test_a_range_of_32_entries_is_the_last_the_device_keeps(handle, copies):
    """dev_extend (lx_seed.hip) beyond the key length: a range of exactly 32 entries gets the full mask (the shift by 32 is avoided), a
    range of 33 makes the read decline.  Either way the list and the counters are the host path's."""
    c = _identical_subjects(copies)
    assert L3.max_word_count(c) == copies
    with capi.Index.build(handle, c["s_red"], c["s_off"], c["s_len"], 10) as dev_ix, capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], 10) as host_ix:
        d, st = _both(handle, dev_ix, host_ix, c, _params(c, adaptive=True, max_seed_dist=0, max_matches=10))
        m = d.matches()
        # the reads equal to the subject hit every copy, with seeds elongated beyond the key length (where the mask takes over)
        assert st.n_matches >= 2 * copies and int((m["qryEnd"] - m["qryStart"]).max()) > L3.key_len(10)
        assert len(np.unique(m["subjId"][m["qryId"] == 0])) == copies
        if copies == 32:
            assert (st.reads_declined, st.launches_full) == (0, 0)
        else:
            assert st.reads_declined >= 1


K_MAX_SECOND = int(re.search(r"kMaxSecond\s*=\s*(\d+)", (Path(__file__).resolve().parents[1] / "lambda_amd" / "csrc" / "lx_seed.h").read_text()).group(1))


@pytest.mark.parametrize("seed_length", [K_MAX_SECOND, K_MAX_SECOND + 1])
def test_the_depth_first_walk_holds_seeds_of_up_to_kMaxSecond_letters(handle, seed_length):
    """Nucleotide reads of 40 letters, seeds with one error anywhere (no exact half): the walk's stack holds the whole seed.  A seed of
    kMaxSecond letters is the device's, one letter more sends every read that is long enough for a seed to the host."""
    n_reads = 20
    c = dict(L3.make_case("nucleotide", n_reads, CASE_SEEDS["nucleotide"]))
    assert c["frames"] == 2
    seqs = [c["q_res"][int(o):int(o) + 40] for o in c["q_off"]]
    seqs[6], seqs[7] = seqs[6][:20], seqs[7][:20]  # read 3: both frames shorter than a seed
    assert all(len(x) == 40 for k, x in enumerate(seqs) if k not in (6, 7))
    c["q_res"] = np.concatenate(seqs)
    c["q_red"] = L3.DNA4[c["q_res"]]
    c["q_off"], c["q_len"] = L3.offsets([len(x) for x in seqs])
    assert L3.max_word_count(c) <= 32  # (no read declines for the other reason)
    with capi.Index.build(handle, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as dev_ix, capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as host_ix:
        total = 0
        for kw in (dict(pre_scoring=0, pre_scoring_thresh=0.0), dict(), dict(adaptive=False)):
            p = _params(c, seed_length=seed_length, seed_offset=8, half_exact=False, max_seed_dist=1, **kw)
            d, st = _both(handle, dev_ix, host_ix, c, p)
            assert st.launches_full == 0
            assert st.reads_declined == (0 if seed_length <= K_MAX_SECOND else n_reads - 1), kw
            total += st.n_matches
        assert total >= 10, total


def test_a_read_with_more_matches_than_its_share_of_the_buffer(handle):
    """One read whose seeds hit more than 64 places (the room a launch has per read): 30 copies of a subject, the read equal to it."""
    rng = np.random.default_rng(8)
    one = synth.STD20[rng.integers(0, 20, 80)].astype(np.uint8)
    s_off, s_len = L3.offsets([80] * 30)
    q_off, q_len = L3.offsets([80])
    c = dict(mode="protein", alph=10, frames=1, unknown=25, s_res=np.tile(one, 30), s_red=L3.LI10[np.tile(one, 30)], s_off=s_off, s_len=s_len,
             q_res=one, q_red=L3.LI10[one], q_off=q_off, q_len=q_len)
    with capi.Index.build(handle, c["s_red"], s_off, s_len, 10) as dev_ix, capi.Index.build(None, c["s_red"], s_off, s_len, 10) as host_ix:
        d, st = _both(handle, dev_ix, host_ix, c, _params(c, max_seed_dist=0, adaptive=False, pre_scoring=0, pre_scoring_thresh=0.0, max_matches=1 << 30))
        assert st.n_matches > 64
        print("launches_full", st.launches_full, "reads_declined", st.reads_declined, "matches", st.n_matches)  # (recorded, not asserted)


def test_the_device_list_goes_into_the_level2_driver_without_a_copy(handle):
    """lx_seed_result_matches_dev -> lx_iterate_matches_dev_top against the host path's list -> lx_iterate_matches ->
    lx_postprocess_records: the same records bit for bit (but where their columns stand) and the same counters.  The device entry
    points take a list of any length -- 131 072 matches is where lx_iterate_matches hands ITS list to them --, so this list is a
    few thousand matches, the smallest that still gives queries more than one record."""
    c = L3.make_case("protein", 300, seed=55, n_subjects=40)
    handle.set_scoring(SCHEMES["blosum62"], 0)
    params = capi.SearchParams(10.0, -1, 0, int(c["s_len"].sum()), 0, 1, 1, 0, capi.LX_FRAMES_NONE, capi.LX_FRAMES_NONE, capi.karlin_params(62), 0, capi.LX_ITERATE_NO_OPS)
    handle.set_subjects(c["s_res"])
    handle.set_subject_seqs(c["s_off"], c["s_len"])
    handle.set_queries(c["q_res"], c["q_off"], c["q_len"], c["q_len"], 1)
    p = _params(c, max_seed_dist=0, seed_offset=3)
    with capi.Index.build(handle, c["s_red"], c["s_off"], c["s_len"], 10) as dev_ix:
        d = capi.seed_queries(handle, dev_ix, None, c["q_res"], c["q_red"], c["q_off"], c["q_len"], p)  # (the resident subjects)
        h = capi.seed_queries(None, dev_ix, c["s_res"], c["q_res"], c["q_red"], c["q_off"], c["q_len"], p)
        n = int(d.stats.n_matches)
        assert n >= 1000 and n == h.stats.n_matches and (d.stats.reads_declined, d.stats.launches_full) == (0, 0)
        # the device pointer's list, copied down by hand, is lx_seed_result_matches' copy
        down = np.zeros(n, capi.MATCH_DTYPE)
        assert _hip_runtime().hipMemcpy(C.c_void_p(down.ctypes.data), C.c_void_p(d.dev().data_ptr()), C.c_size_t(n * 48), 2) == 0  # 2 = hipMemcpyDeviceToHost
        assert down.tobytes() == d.matches().tobytes()
        got, _, gst, rst = handle.iterate_matches_dev_top(d.dev(), n, params, 5)
        plain, _, pst = handle.iterate_matches(c["q_res"], c["q_off"], c["q_len"], c["q_len"], c["s_res"], c["s_off"], c["s_len"], h.matches(), params)
        want, wst = capi.postprocess_records(plain, 5)
    assert len(want) >= 100 and len(got) == len(want)
    for f in got.dtype.names:
        if f != "ops_off":
            assert got[f].tobytes() == want[f].tobytes(), f
    for f in ("hits_duplicate", "failed_bitscore", "failed_evalue", "failed_identity", "num_ext_score", "num_ext_ali"):
        assert getattr(gst, f) == getattr(pst, f), f
    for f in ("qrys_with_hit", "hits_duplicate2", "hits_abundant", "hits_final", "pairs"):
        assert getattr(rst, f) == getattr(wst, f), f


def test_lifetimes_of_indexes_and_results(lx_lib):
    a, b = L3.make_case("protein", 64, seed=61), L3.make_case("nucleotide", 64, seed=62)
    h = capi.Handle(0)
    try:
        ia = capi.Index.build(h, a["s_red"], a["s_off"], a["s_len"], a["alph"])
        ib = capi.Index.build(h, b["s_red"], b["s_off"], b["s_len"], b["alph"])
        host_b = capi.Index.build(None, b["s_red"], b["s_off"], b["s_len"], b["alph"])
        qa, qb = (a["q_res"], a["q_red"], a["q_off"], a["q_len"]), (b["q_res"], b["q_red"], b["q_off"], b["q_len"])
        r1 = capi.seed_queries(h, ia, a["s_res"], *qa, _params(a))
        r2 = capi.seed_queries(h, ib, b["s_res"], *qb, _params(b))
        m1 = r1.matches().copy()
        ia.close()  # seed from an index after another was destroyed
        r3 = capi.seed_queries(h, ib, b["s_res"], *qb, _params(b))
        want = L3.sorted_matches(capi.seed_queries(None, host_b, b["s_res"], *qb, _params(b)).matches())
        assert len(want) >= 50 and np.array_equal(L3.sorted_matches(r3.matches()), want) and np.array_equal(L3.sorted_matches(r2.matches()), want)
        assert np.array_equal(r1.matches(), m1)  # a result outlives its index
        # an index attached to a second handle shares the table; either goes first
        h2 = capi.Handle(0)
        ic = ib.attach(h2)
        with pytest.raises(capi.LambdaExtError) as e:  # a handle that is not the index's
            capi.seed_queries(h2, ib, b["s_res"], *qb, _params(b))
        assert e.value.code == capi.LX_EINVAL and "this handle" in str(e.value)
        with pytest.raises(capi.LambdaExtError):
            capi.seed_queries(h2, host_b, b["s_res"], *qb, _params(b))
        ib.close()
        r4 = capi.seed_queries(h2, ic, b["s_res"], *qb, _params(b))
        assert np.array_equal(L3.sorted_matches(r4.matches()), want)
        for r in (r2, r4, r1, r3):  # results go in any order
            r.close()
        r5 = capi.seed_queries(h2, ic, b["s_res"], *qb, _params(b))  # (takes the block a freed result left with the handle)
        assert np.array_equal(L3.sorted_matches(r5.matches()), want)
        r5.close()
        ic.close()
        host_b.close()
        h2.close()
    finally:
        h.close()
