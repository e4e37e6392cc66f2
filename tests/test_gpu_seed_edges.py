"""seed_reads_kernel (lx_seed.hip) and its driver seed_on_device (lx_seed_host.cpp) against tests/seed_model.py's restatement of the
reference's search(): lx_seed_queries on a handle, sorted match lists and both counters, exactly -- never against the host path,
which tests/test_seed_model.py holds against the same model.  The table of edge cases is the one of that file; where a case is
meant for the kernel it asserts that no read was declined and no launch was full (otherwise the host completion would be what is
tested), where it is meant to decline, how many reads.  Then the buffer and launch paths of the driver, through the two
environment variables the library reads on every call."""
import numpy as np
import pytest

from lambda_amd import capi
from tests import level3_cases as L3
from tests import seed_model as SM

pytestmark = pytest.mark.gpu

_indexes = {}


def device_index(handle, key):
    """the device-made word table of a case's subjects (kept for the session: its handle is the session's), and its geometry"""
    if key not in _indexes:
        c = SM.inputs(key)
        ix = capi.Index.build(handle, c["s_red"], c["s_off"], c["s_len"], c["alph"])
        info = ix.info()
        _indexes[key] = (ix, int(info.key_len), int(info.prefix_len))
    return _indexes[key]


@pytest.fixture(scope="module", autouse=True)
def _indexes_go_before_the_handle(handle):
    yield
    for ix, _, _ in _indexes.values():
        ix.close()
    _indexes.clear()


def device_against_model(handle, entry, reads=None):
    c = SM.inputs(entry.inputs)
    ix, key_len, prefix_len = device_index(handle, entry.inputs)
    p, _, _ = SM.params_of(entry, key_len, prefix_len)
    want, after, failed, ev = SM.expected(entry, key_len, prefix_len, reads=reads)
    r = capi.seed_queries(handle, ix, c["s_res"], c["q_res"], c["q_red"], c["q_off"], c["q_len"], p, reads=reads)
    st = r.stats
    print(entry.name, "seed_length", p.seed_length, "matches", len(want), "hits", after, "failed", failed, "declined", st.reads_declined, "full", st.launches_full)
    assert r.dev() is not None
    assert (st.n_matches, st.hits_after_seeding, st.hits_failed_pre_extend) == (len(want), after, failed)
    assert SM.sorted_rows(r.matches()) == want
    r.close()
    return st, p, (want, after, failed, ev)


@pytest.mark.parametrize("name", [e.name for e in SM.TABLE])
def test_the_kernel_equals_the_model(handle, name):
    entry = SM.BY_NAME[name]
    c = SM.inputs(entry.inputs)
    st, p, (want, after, failed, ev) = device_against_model(handle, entry)
    SM.check_entry(entry, ev, len(want), after, failed)
    if entry.on_device:
        assert L3.max_word_count(c) <= 32 and not ev.wide_reads
        assert (st.reads_declined, st.launches_full) == (0, 0)
        ms, launches = handle.last_phase_ms(9)
        assert launches == 1 and ms > 0
    else:
        assert entry.declines == "long_enough" and L3.max_word_count(c) <= 32  # (no read declines for the other reason)
        n = SM.long_enough(c, p.seed_length)
        assert 0 < n < len(c["q_len"]) // c["frames"]  # (a read without a frame that holds a seed stays with the kernel)
        assert (st.reads_declined, st.launches_full) == (n, 0)


BUFFER_CASE = SM._entry("buffer-protein", "protein", dict())  # 65 reads, one launch, the defaults of tests/test_gpu_level3.py


def test_the_match_buffer_at_its_capacity(handle, monkeypatch):
    """LAMBDA3_SEED_CAP around the number of matches of the call: one record short the launch is full and its reads are the host's,
    with exactly enough room it is the kernel's -- the list and the counters are the model's either way"""
    _, key_len, prefix_len = device_index(handle, BUFFER_CASE.inputs)
    total = len(SM.expected(BUFFER_CASE, key_len, prefix_len)[0])
    n_reads = len(SM.inputs("protein")["q_len"])
    assert total > 100 and n_reads == 65
    for cap in (1, total - 1, total, total + 1):
        monkeypatch.setenv("LAMBDA3_SEED_CAP", str(cap))
        st, _, _ = device_against_model(handle, BUFFER_CASE)
        assert (st.launches_full, st.reads_declined) == ((1, n_reads) if cap < total else (0, 0)), cap


@pytest.mark.parametrize("launch", [1, 7, 64])
def test_several_launches(handle, monkeypatch, launch):
    monkeypatch.setenv("LAMBDA3_SEED_LAUNCH", str(launch))
    st, _, _ = device_against_model(handle, BUFFER_CASE)
    assert (st.reads_declined, st.launches_full) == (0, 0)
    assert handle.last_phase_ms(9)[1] == -(-65 // launch)


def test_a_full_launch_among_others(handle, monkeypatch):
    """seven reads a launch and room for 20 matches: some launches fill up and go to the host, the records of the others stay where
    the kernel wrote them, behind those of the launches before"""
    _, key_len, prefix_len = device_index(handle, BUFFER_CASE.inputs)
    want = SM.expected(BUFFER_CASE, key_len, prefix_len)[0]
    per_launch = [sum(1 for m in want if a <= m[0] < a + 7) for a in range(0, 65, 7)]
    full = sum(1 for n in per_launch if n > 20)
    assert 0 < full < len(per_launch) and any(0 < n <= 20 for n in per_launch), per_launch
    monkeypatch.setenv("LAMBDA3_SEED_LAUNCH", "7")
    monkeypatch.setenv("LAMBDA3_SEED_CAP", "20")
    st, _, _ = device_against_model(handle, BUFFER_CASE)
    assert st.launches_full == full and st.reads_declined == sum(min(7, 65 - 7 * k) for k, n in enumerate(per_launch) if n > 20)


def test_declined_and_kept_reads_in_one_launch(handle, monkeypatch):
    """LAMBDA3_SEED_LAUNCH=3 on seed_model.declining_case: launches that hold declined reads next to reads with matches, behind launches
    that left matches -- the declined reads' records are taken out of the launch's, the others move up, the host's are appended"""
    entry, c = SM.DECLINING, SM.inputs("declining")
    assert L3.max_word_count(c) == 33
    monkeypatch.setenv("LAMBDA3_SEED_LAUNCH", "3")
    st, _, (want, _, _, ev) = device_against_model(handle, entry)
    n_reads, wide = len(c["q_len"]), ev.wide_reads
    by_read = [sum(1 for m in want if m[0] == r) for r in range(n_reads)]
    kept_with_matches = [r for r in range(n_reads) if r not in wide and by_read[r] > 0]
    # a launch with both kinds behind a launch that left matches; in it the read that wrote matches before it declined
    both = [a for a in range(0, n_reads, 3) if any(r in wide for r in range(a, a + 3)) and any(r in kept_with_matches for r in range(a, a + 3))]
    late = SM.DECLINING_LATE_READ
    assert late in wide and late // 3 * 3 in both and late >= 3 and any(r in kept_with_matches for r in range(0, late // 3 * 3)), (sorted(wide), kept_with_matches)
    assert any(m[0] == late and m[2] == 0 and m[3] == 14 for m in want)
    assert (st.reads_declined, st.launches_full) == (len(wide), 0)
    assert handle.last_phase_ms(9)[1] == -(-n_reads // 3)


def test_reads_in_any_order_and_twice(handle):
    for mode in ("protein", "translated"):
        entry = SM._entry("reads-" + mode, mode, dict())
        reads = np.array([40, 2, 17, 2], np.uint64) * SM.inputs(mode)["frames"]
        st, _, (want, _, _, _) = device_against_model(handle, entry, reads=reads)
        assert (st.reads_declined, st.launches_full) == (0, 0) and len(want) > 0
