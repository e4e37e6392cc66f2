"""The host path of lx_seed_queries (h == NULL: seedQueries, host/lx_seeding.hpp) against tests/seed_model.py's restatement of the
reference's search() -- sorted match lists and both counters, exactly -- over the table of edge cases there, with the real scoring
schemes.  Every case asserts the events it names, so that it tests what it says.  No GPU.

That the model catches what it is for was tried by hand, one mutation of seedQueries at a time (not committed); each made this
file fail:
  * `count > 10 * maxMatches` as `>=`: C-30-copies-are-kept-at-max_matches-3 and C-10-copies-max_matches-1-offset-1 (exactly ten
    times max_matches occurrences are kept);
  * desiredOccs' factor 10 as 9: E-frames-max_matches-2-offset-5 and E-frames-max_matches-5-offset-3 (another elongation);
  * the elongation's `&&` as `||`: 87 cases, every adaptive one that finds something;
  * the cursors of a seed visited in reverse order: the two C-order-of-the-cursors-of-a-seed cases, made for it (no other case
    of the table depends on the order, in the model either);
  * the per-read reset behind the length test: five of the six E cases (their first read's first frame is shorter than a seed)."""
import numpy as np
import pytest

from lambda_amd import capi
from tests import seed_model as SM

_indexes = {}


def host_index(key):
    """the host-made word table of a case's subjects, and its geometry"""
    if key not in _indexes:
        c = SM.inputs(key)
        ix = capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"])
        info = ix.info()
        _indexes[key] = (ix, int(info.key_len), int(info.prefix_len))
    return _indexes[key]


def host_against_model(entry, reads=None):
    c = SM.inputs(entry.inputs)
    ix, key_len, prefix_len = host_index(entry.inputs)
    p, _, _ = SM.params_of(entry, key_len, prefix_len)
    want, after, failed, ev = SM.expected(entry, key_len, prefix_len, reads=reads)
    r = capi.seed_queries(None, ix, c["s_res"], c["q_res"], c["q_red"], c["q_off"], c["q_len"], p, reads=reads)
    st = r.stats
    print(entry.name, "seed_length", p.seed_length, "matches", len(want), "hits", after, "failed", failed, dict(ev))
    assert (st.n_matches, st.hits_after_seeding, st.hits_failed_pre_extend) == (len(want), after, failed)
    assert SM.sorted_rows(r.matches()) == want
    return want, after, failed, ev


@pytest.mark.parametrize("name", [e.name for e in SM.TABLE])
def test_the_host_path_equals_the_model(lx_lib, name):
    entry = SM.BY_NAME[name]
    want, after, failed, ev = host_against_model(entry)
    SM.check_entry(entry, ev, len(want), after, failed)


def test_the_geometry_the_table_is_written_against(lx_lib):
    """Group B's seed lengths end on the table's regimes only if the indexes have the geometry the model assumes"""
    for key in ("protein", "nucleotide"):
        _, key_len, prefix_len = host_index(key)
        assert key_len == SM.L3.key_len(SM.inputs(key)["alph"]) and 2 < prefix_len + 1 < key_len - 1
    assert 2 * SM.k_max_second() + 1 < 63 <= 70


def test_the_reads_the_device_would_decline(lx_lib):
    """the case of tests/test_gpu_seed_edges.py's launch test, on the host: 33 occurrences beyond key_len"""
    want, _, _, ev = host_against_model(SM.DECLINING)
    assert len(want) > 100 and SM.DECLINING_LATE_READ in ev.wide_reads and 0 < len(ev.wide_reads) < len(SM.inputs("declining")["q_len"])


def test_reads_in_any_order_and_twice(lx_lib):
    """reads = [40, 2, 17, 2] (first frames): unsorted, one of them twice"""
    for mode in ("protein", "translated"):
        entry = SM._entry("reads-" + mode, mode, dict())
        reads = np.array([40, 2, 17, 2], np.uint64) * SM.inputs(mode)["frames"]
        want, _, _, _ = host_against_model(entry, reads=reads)
        once, _, _, _ = host_against_model(entry, reads=reads[:3])
        assert len(want) > len(once) > 0  # (read 2 has matches, and they are there twice)
