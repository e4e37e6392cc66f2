"""GPU tests of the pre-extension filter (lx_prefilter_batch, lx_prefilter.hip) against tests/prefilter_cases.py: an independent
restatement of the reference's seedLooksPromising and a table of cases aimed at the kernel's clips, its dword tail, its threshold and
the ends of its buffers.  Every comparison is exact (one byte per seed)."""
import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import prefilter_cases as pc
from tests.test_oracle import SCHEMES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    cs = pc.cases()
    return cs, np.array([pc.expected(c) for c in cs], dtype=np.uint8)


def _calls(cs):
    """the cases grouped by what one lx_prefilter_batch call fixes: scheme, slot, seed_length, pre_scoring, thresh"""
    groups = {}
    for i, c in enumerate(cs):
        groups.setdefault((c.scheme, c.slot, c.seed_length, c.pre_scoring, c.thresh), []).append(i)
    return groups


def _run(handle, cs, idx, resident=False, last=None):
    c0 = cs[idx[0]]
    handle.set_scoring(SCHEMES[c0.scheme], c0.slot)
    q, s, seeds = pc.buffers([cs[i] for i in idx], capi.SEED_DTYPE, last=last)
    if resident:
        handle.set_subjects(s)
        try:
            return handle.prefilter_batch(q, None, seeds, c0.seed_length, c0.pre_scoring, c0.thresh, c0.slot)
        finally:
            handle.set_subjects(None)
    return handle.prefilter_batch(q, s, seeds, c0.seed_length, c0.pre_scoring, c0.thresh, c0.slot)


def test_prefilter_case_table(handle, table):
    cs, want = table
    groups = _calls(cs)
    assert len(groups) >= 15
    seen = {}
    for idx in groups.values():
        got = _run(handle, cs, idx)
        for i, g in zip(idx, got):
            assert g == want[i], (cs[i].group, cs[i].name, int(g))
            seen.setdefault(cs[i].group, set()).add(int(g))
    assert len(seen) == 8 and all(v == {0, 1} for v in seen.values()), seen  # both answers in every group
    # bs_rev really went through slot 1 (prefilter_kernel reads p.sc = sc_dev[slot])
    assert any(k[1] == 1 for k in groups)
    handle.set_scoring(SCHEMES["blosum62"], 0)


@pytest.mark.parametrize("resident", [False, True])
def test_prefilter_region_ends_on_the_buffers_last_bytes(handle, table, resident):
    """The decisive seed's sequences close q_res and s_res, so its region's last cell is the buffers' last byte and the last dword of
    lx_prefilter.hip:59 reaches 1, 2 or 3 bytes into the slack behind them (kSlack); with s_res = None the subject is the resident copy
    (lx_set_subjects), which has a slack of its own."""
    cs, want = table
    ends = [i for i, c in enumerate(cs) if c.group == "buffer ends"]
    assert len(ends) == 6
    key = (cs[ends[0]].scheme, cs[ends[0]].slot, cs[ends[0]].seed_length, cs[ends[0]].pre_scoring, cs[ends[0]].thresh)
    idx = _calls(cs)[key]
    assert set(ends) <= set(idx) and len(idx) > 20
    for e in ends:
        c = cs[e]
        assert c.qry_end == len(c.q) and c.subj_start + (c.qry_end - c.qry_start) == len(c.s)  # ends on the last byte of both
        got = _run(handle, cs, idx, resident=resident, last=c)
        assert (got == want[idx]).all(), (c.name, np.nonzero(got != want[idx])[0])
        # alone in the buffers: the region is all there is before the slack
        assert _run(handle, cs, [e], resident=resident)[0] == want[e], c.name


@pytest.mark.parametrize("n", [255, 256, 257])
def test_prefilter_block_edge(handle, table, n):
    """n around one workgroup of 256 lanes (`x >= p.n`, lx_prefilter.hip:22; the second block of launch_prefilter)."""
    cs, want = table
    idx = max(_calls(cs).values(), key=len)
    rep = [idx[k % len(idx)] for k in range(n)]
    c0 = cs[idx[0]]
    handle.set_scoring(SCHEMES[c0.scheme], c0.slot)
    q, s, seeds = pc.buffers([cs[i] for i in idx], capi.SEED_DTYPE)
    got = handle.prefilter_batch(q, s, seeds[[k % len(idx) for k in range(n)]], c0.seed_length, c0.pre_scoring, c0.thresh, c0.slot)
    assert len(got) == n and (got == want[rep]).all()
    assert 0 < got.sum() < n


def test_prefilter_random_seeds_equal_the_model(handle, oracle):
    """tests/test_gpu_trace.py::test_prefilter's input (4000 random protein seeds, half of them on a planted diagonal): a 200-seed
    sample of the kernel's and the oracle's answers against the model."""
    from tests import oracle_lib

    sc_p = SCHEMES["blosum62"]
    handle.set_scoring(sc_p, 0)
    osc = oracle_lib.scoring_from(sc_p)
    mat = sc_p.matrix_np()
    rng = np.random.default_rng(5)
    nq, ns = 50, 20
    qlen = rng.integers(30, 200, nq)
    slen = rng.integers(200, 1500, ns)
    qoff = np.concatenate([[0], np.cumsum(qlen)[:-1]])
    soff = np.concatenate([[0], np.cumsum(slen)[:-1]])
    q = synth.STD20[rng.integers(0, 20, int(qlen.sum()))].astype(np.uint8)
    s = synth.STD20[rng.integers(0, 20, int(slen.sum()))].astype(np.uint8)
    n = 4000
    seeds = np.zeros(n, dtype=capi.SEED_DTYPE)
    for i in range(n):
        a, b = int(rng.integers(0, nq)), int(rng.integers(0, ns))
        L = int(rng.integers(8, 14))
        qs = int(rng.integers(0, qlen[a] - L + 1))
        ss = int(rng.integers(0, slen[b] - L + 1))
        if rng.random() < 0.5:
            lo = min(qs, ss, 15)
            hi = min(qlen[a] - qs, slen[b] - ss, 25)
            s[soff[b] + ss - lo: soff[b] + ss + hi] = q[qoff[a] + qs - lo: qoff[a] + qs + hi]
        seeds[i] = (qoff[a], soff[b], qlen[a], slen[b], qs, qs + L, ss, 0)
    sample = np.random.default_rng(6).choice(n, 200, replace=False)
    for seed_length, pre, thr in ((10, 2, 2.0), (11, 2, 2.0), (10, 1, 2.0), (14, 2, 1.4)):
        got = handle.prefilter_batch(q, s, seeds, seed_length, pre, thr)
        for i in sample:
            x = seeds[i]
            qq = q[int(x["q_off"]): int(x["q_off"]) + int(x["q_len"])]
            ss_ = s[int(x["s_off"]): int(x["s_off"]) + int(x["s_len"])]
            m = pc.model(qq, ss_, int(x["qry_start"]), int(x["qry_end"]), int(x["subj_start"]), seed_length, pre, thr, mat)
            want = oracle.seed_looks_promising(qq, ss_, int(x["qry_start"]), int(x["qry_end"]), int(x["subj_start"]), seed_length, pre, thr, osc)
            assert bool(got[i]) == m == want, (i, seed_length, pre, thr)
        assert 0.05 < got[sample].mean() < 0.95


def test_prefilter_refusals_leave_the_handle_usable(lx_lib, handle, table):
    """What lx_prefilter_batch checks before it launches (lx_host_batch.cpp): each is LX_EINVAL, and the next call on the handle is right."""
    cs, want = table
    idx = max(_calls(cs).values(), key=len)
    c0 = cs[idx[0]]
    handle.set_scoring(SCHEMES[c0.scheme], c0.slot)
    q, s, seeds = pc.buffers([cs[i] for i in idx], capi.SEED_DTYPE)

    def call(h, q_, s_, sd, slot=c0.slot):
        return h.prefilter_batch(q_, s_, sd, c0.seed_length, c0.pre_scoring, c0.thresh, slot)

    def broken(field, value, at=3):
        b = seeds.copy()
        b[field][at] = value
        return b

    at = 3
    x = seeds[at]
    refusals = [
        ("qry_end > q_len", q, broken("qry_end", int(x["q_len"]) + 1)),
        ("qry_end < qry_start", q, broken("qry_end", int(x["qry_start"]) - 1) if x["qry_start"] else broken("qry_start", int(x["qry_end"]) + 1)),
        ("subj_start + actual > s_len", q, broken("subj_start", int(x["s_len"]) - (int(x["qry_end"]) - int(x["qry_start"])) + 1)),
        ("a slice beyond q_bytes", q[:-1], seeds),  # (the last case's query ends at q_bytes)
        ("a query offset beyond q_bytes", q, broken("q_off", len(q))),
        ("a slice beyond s_bytes", q, broken("s_off", len(s) - int(x["s_len"]) + 1)),
    ]
    for name, q_, sd in refusals:
        with pytest.raises(capi.LambdaExtError) as e:
            call(handle, q_, s, sd)
        assert e.value.code == capi.LX_EINVAL, (name, str(e.value))
        assert (call(handle, q, s, seeds) == want[idx]).all(), name
    # a scoring slot that was never set, and one that does not exist: on a handle of its own (the shared one's slots are all in use)
    with capi.Handle(0) as h2:
        h2.set_scoring(SCHEMES[c0.scheme], 0)
        for slot in (1, 2, -1):
            with pytest.raises(capi.LambdaExtError) as e:
                call(h2, q, s, seeds, slot=slot)
            assert e.value.code == capi.LX_EINVAL, (slot, str(e.value))
            assert (call(h2, q, s, seeds, slot=0) == want[idx]).all(), slot
    handle.set_scoring(SCHEMES["blosum62"], 0)
