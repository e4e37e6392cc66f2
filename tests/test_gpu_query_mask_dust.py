"""The nucleotide query masking on the device: the kernels' mask (lx_query_mask_create_dust on a handle) byte for byte against the
Python restatement of tests/dust_cases.py and against the host function's -- on the stated cases, at the sweep kernel's own edges (a
workgroup's run of starts and its halo, the 64-lane wavefront, the 64-bit word), on a repeat over several workgroups and on a read
set --, and lx_seed_queries_masked on a handle with the device mask against the host seeder with the host mask."""
import re
from pathlib import Path

import numpy as np
import pytest

from lambda_amd import capi
from tests import dust_cases as DC
from tests import level3_cases as L3
from tests.test_gpu_level3 import _params
from tests.test_query_mask_dust import for_the_rule, nucleotide_case

pytestmark = pytest.mark.gpu

_HEADER = (Path(__file__).resolve().parent.parent / "lambda_amd" / "csrc" / "lx_dust.h").read_text()
BLOCK = int(re.search(r"kDustBlock = (\d+)", _HEADER).group(1))


def run_of(window):
    """dust_run: the starts a workgroup of the sweep answers for; the window - 3 behind them are its halo"""
    return BLOCK - (window - 3)


def _device_equals_restatement(handle, seqs, window=64, level=20, table=None, cache=None):
    res, off, ln = DC.as_set(seqs) if table is None else table
    if cache is None:
        want = DC.dust_mask_set(res, off, ln, window, level)
    else:  # (a set drawn from few distinct sequences: the restatement runs once per distinct one)
        for s in seqs:
            if s.tobytes() not in cache:
                cache[s.tobytes()] = DC.dust_mask(s, window, level)
        want = np.concatenate([cache[s.tobytes()] for s in seqs])
    p = capi.DustParams(window, level)
    with capi.QueryMask.dust(handle, res, off, ln, p) as m, capi.QueryMask.dust(None, res, off, ln, p) as host:
        ms, launches = handle.last_phase_ms(15)
        assert launches == 1 and ms >= 0
        got = m.copy()
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert np.array_equal(got, host.copy())
        assert m.info() == DC.counts(want, off, ln) == host.info()
    return want


@pytest.mark.parametrize("name", sorted(DC.named_cases()))
def test_named_cases(handle, name):
    seqs, window, _ = DC.named_cases()[name]
    _device_equals_restatement(handle, seqs, window)


@pytest.mark.parametrize("window", [8, 16, 64])
def test_random_sets(handle, window):
    masked = free = untouched = 0
    for level in (10, 20, 30):
        # thirty seeded sets laid end to end: some 150 sequences over a few dozen workgroups
        seqs = [s for seed in range(30) for s in DC.random_reads(1000 * level + seed)]
        want = _device_equals_restatement(handle, seqs, window, level)
        res, off, ln = DC.as_set(seqs)
        masked, free = masked + int(want.sum()), free + int((want == 0).sum())
        untouched += int((ln > 0).sum()) - DC.counts(want, off, ln)[2]
    assert masked > 1000 and free > 1000 and untouched


def _edges(window):
    run = run_of(window)
    return sorted({run, 2 * run, 64, 128, 192, BLOCK})


@pytest.mark.parametrize("window", [16, 64])
def test_a_perfect_interval_over_every_edge(handle, window):
    """an AC repeat of window + 8 letters in random flanks, its first letter placed so that its perfect intervals start in the last
    window - 3 starts of a workgroup's run (and at a wavefront's and a word's last lanes) and end behind the edge"""
    rng = np.random.default_rng(window)
    for edge in _edges(window):
        for back in (window - 3, window // 2, 2):
            for delta in (-1, 0, 1):
                lead = edge - back + delta
                if lead < 0:
                    continue
                seq = np.concatenate([DC.random_dna(rng, lead), DC.repeat("AC", window + 8), DC.random_dna(rng, 30)])
                want = _device_equals_restatement(handle, [seq], window)
                assert want[lead + 2:lead + window + 6].all() and not want.all()


@pytest.mark.parametrize("window", [16, 64])
def test_a_stretch_that_ends_at_an_edge(handle, window):
    """a repeat that an N, or the sequence's end, cuts one letter before, at and after each edge -- and goes on behind it"""
    rng = np.random.default_rng(100 + window)
    for edge in _edges(window):
        for delta in (-1, 0, 1):
            cut = edge + delta
            lead = max(0, cut - 40)
            head = np.concatenate([DC.random_dna(rng, lead), DC.repeat("AC", cut - lead)])
            with_n = np.concatenate([head, [4], DC.repeat("AC", 40), DC.random_dna(rng, 20)])
            want = _device_equals_restatement(handle, [with_n], window)
            assert not want[cut] and want[cut - 12:cut].all() and want[cut + 1:cut + 41].all()
            # the same with a border: two sequences, the second begins with the repeat
            want = _device_equals_restatement(handle, [head, np.concatenate([DC.repeat("AC", 40), DC.random_dna(rng, 20)])], window)
            assert want[cut - 12:cut + 40].all()


def test_a_repeat_over_several_workgroups(handle):
    assert _device_equals_restatement(handle, [DC.repeat("AC", 700)]).all()
    assert _device_equals_restatement(handle, [DC.repeat("AC", 700)], 13, 20).all()
    assert not _device_equals_restatement(handle, [DC.repeat("ACGTAGCTT", 700)], 16).any()


def test_empty_sequences_gaps_and_errors(handle):
    rng = np.random.default_rng(3)
    seqs = [DC.repeat("AC", 40), np.zeros(0, np.uint8), DC.random_dna(rng, 30), DC.repeat("T", 20), np.zeros(0, np.uint8), DC.random_dna(rng, 70)]
    _device_equals_restatement(handle, seqs)
    res, off, ln = DC.as_set(seqs)
    # the same sequences with gaps of repeats between them (letters of no sequence): a repeat never runs on into a gap or out of one
    gaps = [7, 0, 0, 20, 3, 1]
    res2, off2, at = [], [], 0
    for s, g in zip(seqs, gaps):
        res2.append(DC.repeat("AC", g)), res2.append(s)
        off2.append(at + g)
        at += g + len(s)
    res2, off2 = np.concatenate(res2), np.array(off2, np.uint64)
    want = _device_equals_restatement(handle, None, table=(res2, off2, ln))
    assert want[:7].sum() == 0 and want[7:47].all()
    with pytest.raises(capi.LambdaExtError) as e:
        capi.QueryMask.dust(handle, res, off[::-1].copy(), ln[::-1].copy())
    assert e.value.code == capi.LX_EINVAL and "ascending order" in str(e.value)
    for bad in ((3, 20), (64, 0), (65, 20), (64, 1001)):
        with pytest.raises(capi.LambdaExtError) as e:
            capi.QueryMask.dust(handle, res, off, ln, capi.DustParams(*bad))
        assert e.value.code == capi.LX_EINVAL
        assert handle.last_phase_ms(15)[1] == 0  # (refused before any device work)


def test_a_read_set(handle):
    """3 000 reads x 2 frames of 150 letters, one read in ten with a microsatellite of 20 to 60 letters; the second frame is the
    first one's reverse complement, and so is its mask"""
    rng = np.random.default_rng(77)
    pool = []
    for k in range(100):
        x = DC.random_dna(rng, 150)
        if k % 10 == 0:
            n, a = int(rng.integers(20, 61)), int(rng.integers(0, 90))
            x[a:a + n] = np.resize(rng.integers(0, 4, int(rng.integers(1, 5))).astype(np.uint8), n)
        if k % 25 == 3:
            x[rng.integers(0, 150, 2)] = 4
        pool.append(x)
    pick = rng.integers(0, len(pool), 3000)
    seqs = [DC.random_dna(rng, 2)] + [f for k in pick for f in (pool[k], DC.revcomp(pool[k]))] + [DC.repeat("A", 6)]
    want = _device_equals_restatement(handle, seqs, cache={})
    assert 0.01 < want.mean() < 0.1
    body = want[2:-6].reshape(3000, 2, 150)
    assert np.array_equal(body[:, 1, :], body[:, 0, ::-1])


def test_masked_seeding_on_the_device_equals_the_host_path(handle):
    c = nucleotide_case()
    q = (c["q_res"], c["q_red"], c["q_off"], c["q_len"])
    letters = for_the_rule(c["q_res"])
    want_mask = DC.dust_mask_set(letters, c["q_off"], c["q_len"])
    assert want_mask.any()
    with capi.Index.build(handle, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as dev_ix, \
            capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as host_ix, \
            capi.QueryMask.dust(handle, letters, c["q_off"], c["q_len"]) as dev_m, \
            capi.QueryMask.dust(None, letters, c["q_off"], c["q_len"]) as host_m:
        assert np.array_equal(dev_m.copy(), want_mask) and np.array_equal(host_m.copy(), want_mask)
        for kw in (dict(max_seed_dist=0, adaptive=False), dict(max_seed_dist=0), dict(), dict(half_exact=False)):
            p = _params(c, **kw)
            plain = L3.sorted_matches(capi.seed_queries(None, host_ix, c["s_res"], *q, p).matches())
            h = capi.seed_queries(None, host_ix, c["s_res"], *q, p, mask=host_m)
            d = capi.seed_queries(handle, dev_ix, c["s_res"], *q, p, mask=dev_m)
            assert d.dev() is not None
            got = L3.sorted_matches(d.matches())
            assert np.array_equal(got, L3.sorted_matches(h.matches()))
            assert (d.stats.hits_after_seeding, d.stats.hits_failed_pre_extend) == (h.stats.hits_after_seeding, h.stats.hits_failed_pre_extend)
            for r in got:
                o = int(c["q_off"][r["qryId"]]) + int(r["qryStart"])
                assert not want_mask[o:o + 14].any()
            assert 0 < len(got) < len(plain)
