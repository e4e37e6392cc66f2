"""Query masking on the device: the kernels' mask (lx_query_mask_create_seg on a handle) byte for byte against the Python restatement
of tests/qmask_cases.py -- on the hand-made cases, at the kernels' own edges (the 64-window word, the 256-window workgroup, the
carry scan's tile) and on a read set --, and lx_seed_queries_masked on a handle against the host seeder with the host mask."""
import re
from pathlib import Path

import numpy as np
import pytest

from lambda_amd import capi
from tests import level3_cases as L3
from tests import qmask_cases as QC
from tests.test_gpu_level3 import MODES, _params

pytestmark = pytest.mark.gpu

_HEADER = (Path(__file__).resolve().parent.parent / "lambda_amd" / "csrc" / "lx_qmask.h").read_text()
TILE = int(re.search(r"kTileWords = (\d+)", _HEADER).group(1)) * 64  # kQmaskTile: letters per workgroup of the carry scan
W = 12


def _device_equals_restatement(handle, seqs, cache=None, **seg):
    res, off, ln = QC.as_set(seqs)
    if cache is None:
        want = QC.seg_mask_set(res, off, ln, **seg)
    else:  # (a set drawn from few distinct sequences: the restatement runs once per distinct one)
        for s in seqs:
            if s.tobytes() not in cache:
                cache[s.tobytes()] = QC.seg_mask(s, **seg)
        want = np.concatenate([cache[s.tobytes()] for s in seqs])
    p = capi.SegParams(seg.get("W", 12), seg.get("k1", 2.2), seg.get("k2", 2.5))
    with capi.QueryMask.seg(handle, res, off, ln, p) as m:
        ms, launches = handle.last_phase_ms(15)
        assert launches == 1 and ms >= 0
        got = m.copy()
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert m.info() == QC.counts(want, off, ln)
    return want


@pytest.mark.parametrize("name", sorted(QC.named_cases()))
def test_named_cases(handle, name):
    _device_equals_restatement(handle, QC.named_cases()[name])


def test_compositions_other_windows_and_random_sets(handle):
    _device_equals_restatement(handle, QC.composition_windows(12))
    for seg in (dict(W=7, k1=1.6, k2=1.6), dict(W=4, k1=1.0, k2=1.5), dict(W=64, k1=3.0, k2=3.4)):
        for seed in range(10):
            _device_equals_restatement(handle, QC.random_frames(seed) + [QC.repeat("GGS", 150)], **seg)
    # the 300 sets of the host test, laid end to end in groups of 30
    for g in range(10):
        _device_equals_restatement(handle, [s for seed in range(30 * g, 30 * g + 30) for s in QC.random_frames(seed)])


def _mixed(rng, n):
    """n letters: random stretches and repeats of 1 to 3 letters, 5 to 60 letters each"""
    parts, have = [], 0
    while have < n:
        k = int(rng.integers(5, 61))
        parts.append(QC.random_protein(rng, k) if rng.random() < 0.5 else np.resize(rng.integers(0, 20, int(rng.integers(1, 4))).astype(np.uint8), k))
        have += k
    return np.concatenate(parts)[:n]


@pytest.mark.parametrize("edge", [64, 256, TILE])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_window_counts_at_the_edges(handle, edge, delta):
    rng = np.random.default_rng(edge + delta)
    n = edge + delta + W - 1  # edge + delta windows
    want = _device_equals_restatement(handle, [_mixed(rng, n), QC.repeat("SP", 30)])
    assert want.any() and not want.all()
    # ... and one run over all of them
    assert _device_equals_restatement(handle, [QC.repeat("SP", n)]).all()


@pytest.mark.parametrize("trigger_last", [True, False])
def test_a_run_over_three_tiles_with_one_trigger(handle, trigger_last):
    """windows that only reach thr2 over more than two tiles; the only windows that reach thr1 at one end"""
    weak, strong = QC.repeat("SPACD", 2 * TILE + 500), QC.repeat("SP", 40)
    rng = np.random.default_rng(1)
    body = np.concatenate([weak, strong] if trigger_last else [strong[::-1], weak])
    seq = np.concatenate([QC.random_protein(rng, 100), body, QC.random_protein(rng, 100)])
    want = _device_equals_restatement(handle, [QC.random_protein(rng, 37), seq])
    assert want[37 + 100:37 + 100 + len(body)].all()
    # without the trigger nothing of it is masked
    assert not _device_equals_restatement(handle, [np.concatenate([QC.random_protein(rng, 100), weak, QC.random_protein(rng, 100)])]).any()


def test_a_long_sequence_that_is_one_run(handle):
    assert _device_equals_restatement(handle, [QC.repeat("SPA", 40000)]).all()


def test_a_read_set(handle):
    """20 000 reads x 6 frames of 50 letters, about every tenth frame repetitive; first and last sequences shorter than W"""
    rng = np.random.default_rng(77)
    pool = [QC.random_protein(rng, 50) for _ in range(180)] + [_mixed(rng, 50) for _ in range(10)] + \
           [np.resize(rng.integers(0, 20, int(rng.integers(1, 4))).astype(np.uint8), 50) for _ in range(10)]
    pick = rng.integers(0, len(pool), 120000)
    seqs = [QC.random_protein(rng, 5)] + [pool[k] for k in pick] + [QC.repeat("S", 11)]
    want = _device_equals_restatement(handle, seqs, cache={})
    frac = want.mean()
    assert 0.03 < frac < 0.2


def test_gaps_between_sequences_and_errors(handle):
    rng = np.random.default_rng(3)
    seqs = [QC.repeat("SP", 40), QC.random_protein(rng, 30), QC.repeat("K", 20), QC.random_protein(rng, 70)]
    res, off, ln = QC.as_set(seqs)
    # the same sequences with gaps of repeats between them (letters of no sequence)
    gaps = [7, 0, 20, 3]
    res2, off2, at = [], [], 0
    for s, g in zip(seqs, gaps):
        res2.append(QC.repeat("SP", g)), res2.append(s)
        off2.append(at + g)
        at += g + len(s)
    res2, off2 = np.concatenate(res2), np.array(off2, np.uint64)
    want = QC.seg_mask_set(res2, off2, ln)
    with capi.QueryMask.seg(handle, res2, off2, ln) as m:
        assert np.array_equal(m.copy(), want) and m.info() == QC.counts(want, off2, ln)
    with pytest.raises(capi.LambdaExtError) as e:
        capi.QueryMask.seg(handle, res, off[::-1].copy(), ln[::-1].copy())
    assert e.value.code == capi.LX_EINVAL and "ascending order" in str(e.value)
    with pytest.raises(capi.LambdaExtError) as e:
        capi.QueryMask.seg(handle, res, off, ln, capi.SegParams(3, 1.0, 1.5))
    assert e.value.code == capi.LX_EINVAL


def _case_with_repeat(mode):
    """level3_cases.make_case with a 30-letter SP stretch shared by subject 0 and every third read's first frame"""
    c = L3.make_case(mode, 64, seed=31)
    if mode in ("protein", "translated"):
        sp = QC.repeat("SP", 30)
        o = int(c["s_off"][0])
        c["s_res"][o + 10:o + 40] = sp
        c["s_red"][o + 10:o + 40] = L3.LI10[sp]
        for r in range(0, 64, 3):
            if r in (5, 9):
                continue
            o = int(c["q_off"][r * c["frames"]])
            c["q_res"][o + 8:o + 38] = sp
            c["q_red"][o + 8:o + 38] = L3.LI10[sp]
    return c


@pytest.mark.parametrize("mode", list(MODES))
def test_masked_seeding_on_the_device_equals_the_host_path(handle, mode):
    c = _case_with_repeat(mode)
    q = (c["q_res"], c["q_red"], c["q_off"], c["q_len"])
    want_mask = QC.seg_mask_set(c["q_res"], c["q_off"], c["q_len"])
    assert want_mask.any()
    sl = MODES[mode][2]
    with capi.Index.build(handle, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as dev_ix, \
            capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as host_ix, \
            capi.QueryMask.seg(handle, c["q_res"], c["q_off"], c["q_len"]) as dev_m, \
            capi.QueryMask.seg(None, c["q_res"], c["q_off"], c["q_len"]) as host_m:
        assert np.array_equal(dev_m.copy(), want_mask) and np.array_equal(host_m.copy(), want_mask)
        for kw in (dict(max_seed_dist=0, adaptive=False), dict(max_seed_dist=0), dict(), dict(half_exact=False)):
            p = _params(c, **kw)
            plain_h = L3.sorted_matches(capi.seed_queries(None, host_ix, c["s_res"], *q, p).matches())
            plain_d = L3.sorted_matches(capi.seed_queries(handle, dev_ix, c["s_res"], *q, p, mask=None).matches())
            assert np.array_equal(plain_d, plain_h)  # mask=None: the list of today
            h = capi.seed_queries(None, host_ix, c["s_res"], *q, p, mask=host_m)
            d = capi.seed_queries(handle, dev_ix, c["s_res"], *q, p, mask=dev_m)
            assert d.dev() is not None
            got = L3.sorted_matches(d.matches())
            assert np.array_equal(got, L3.sorted_matches(h.matches()))
            assert (d.stats.hits_after_seeding, d.stats.hits_failed_pre_extend) == (h.stats.hits_after_seeding, h.stats.hits_failed_pre_extend)
            for r in got:
                o = int(c["q_off"][r["qryId"]]) + int(r["qryStart"])
                assert not want_mask[o:o + sl].any()
            assert len(got) < len(plain_h)
        # a host-only mask, and a mask of another sequence table, are refused on the device
        for bad, text in ((host_m, "host only"), (None, "another sequence table")):
            with pytest.raises(capi.LambdaExtError) as e:
                if bad is None:
                    with capi.QueryMask.seg(handle, c["q_res"], c["q_off"][:-1], c["q_len"][:-1]) as other:
                        capi.seed_queries(handle, dev_ix, c["s_res"], *q, _params(c), mask=other)
                else:
                    capi.seed_queries(handle, dev_ix, c["s_res"], *q, _params(c), mask=bad)
            assert e.value.code == capi.LX_EINVAL and text in str(e.value)


def test_a_given_mask_on_the_device(handle):
    c = _case_with_repeat("protein")
    q = (c["q_res"], c["q_red"], c["q_off"], c["q_len"])
    rng = np.random.default_rng(6)
    bytes_ = (rng.random(len(c["q_res"])) < 0.04).astype(np.uint8)
    p = _params(c, max_seed_dist=0, adaptive=False, pre_scoring=0, pre_scoring_thresh=0.0)
    want = L3.sorted_matches(QC.brute_exact_matches_masked(c, bytes_, 10, 5))
    with capi.Index.build(handle, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as ix, \
            capi.QueryMask.from_bytes(handle, bytes_, c["q_off"], c["q_len"]) as m:
        assert np.array_equal(m.copy(), bytes_) and m.info()[1] == int(bytes_.sum())
        got = L3.sorted_matches(capi.seed_queries(handle, ix, c["s_res"], *q, p, mask=m).matches())
    assert len(want) > 20 and np.array_equal(got, want.astype(capi.MATCH_DTYPE))
