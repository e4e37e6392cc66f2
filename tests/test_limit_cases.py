"""CPU tests of tests/limit_cases.py (no GPU): the GPU tests of the number-range gates trust two things, and both are shown here.

1. Every input they run with a known true score has exactly that score: the int32 oracle's score_batch returns the target, and the
   columns of the oracle's alignment add up to it.  Nothing but the oracle decides whether a case sits on its gate.
2. Under the extreme scoring schemes of tests/test_gpu_schemes_edges.py the oracle agrees with the O(n^3) general-gap Smith-Waterman
   of tests/brute.py, which shares no recurrence with it."""
import numpy as np
import pytest

from tests import brute, limit_cases, oracle_lib


@pytest.fixture(scope="module")
def cases():
    return limit_cases.all_cases()


@pytest.mark.parametrize("name", sorted(limit_cases.CASE_NAMES))
def test_targets_are_the_true_scores(oracle, cases, name):
    sc, (q, s, ext, target) = cases[name]
    osc = oracle_lib.scoring_from(sc)
    got = oracle.score_batch(q, s, ext, osc, threads=8)
    known = np.nonzero(target >= 0)[0]
    assert len(known) > 0 and (got[known] == target[known]).all(), (name, known[got[known] != target[known]][:8])
    # the alignment's columns add up to the target (the longest windows: two of them -- the oracle keeps a full matrix per window)
    M = sc.matrix_np()
    live = known[target[known] > 0]
    pick = live if int(ext["s_len"][live].max()) < 5000 else live[:2]
    pick = pick[:: max(1, len(pick) // 24)]
    for i, (hsp, ops) in zip(pick, oracle.align_batch(q, s, ext[pick], osc)):
        x = ext[i]
        qq = q[int(x["q_off"]): int(x["q_off"]) + int(x["q_len"])]
        ss = s[int(x["s_off"]): int(x["s_off"]) + int(x["s_len"])]
        total, qe, se = brute.score_of_ops(qq, ss, hsp.q_begin, hsp.s_begin, ops, M, sc.gap_open, sc.gap_extend)
        assert (hsp.score, total, qe, se) == (target[i], target[i], hsp.q_end, hsp.s_end), (name, i)


def test_the_cases_sit_on_their_gates(cases):
    """What the case names promise: one target on either side of 2046 / 29695, the host gate's products on either side of 32000."""
    CASES = cases
    t = CASES["one_panel_16"][1][3]
    assert {2046, 2047} <= set(t.tolist()) and set(limit_cases.TARGETS_2046) <= set(t.tolist())
    t = CASES["i16_pairs"][1][3]
    assert {0x7BFF - 2048, 0x7BFF - 2047} <= set(t.tolist())
    assert CASES["gate_1066"][1][3].max() == 31980 < 32000 <= 32010 == CASES["gate_1067"][1][3].max()
    assert CASES["largest"][1][3].max() == 31999
    assert CASES["rows_65535"][1][2]["s_len"].max() == 65535 and CASES["rows_65536"][1][2]["s_len"].max() == 65536


SCHEME_NAMES = limit_cases.EXTREME_NAMES + ["v_minus_ge_32"]


@pytest.mark.parametrize("name", SCHEME_NAMES)
def test_oracle_vs_general_gap_sw_under_extreme_schemes(oracle, name):
    SCHEMES = dict(limit_cases.extreme_schemes(), v_minus_ge_32=None)
    assert sorted(SCHEMES) == sorted(SCHEME_NAMES)
    sc_p = limit_cases.refused_v_minus_ge_32() if SCHEMES[name] is None else limit_cases.make_scoring(*SCHEMES[name])
    sc = oracle_lib.scoring_from(sc_p)
    M = sc_p.matrix_np()
    na = sc_p.alphabet_size
    rng = np.random.default_rng(len(name))
    hits = 0
    for it in range(80):
        lq, ls = int(rng.integers(1, 24)), int(rng.integers(1, 28))
        q = rng.integers(0, na, lq).astype(np.uint8)
        if rng.random() < 0.7 and lq > 3:  # a copy of the query with a piece cut out or put in: gaps worth their price
            cut = int(rng.integers(1, lq))
            s = np.concatenate([q[:cut], rng.integers(0, na, int(rng.integers(0, 3))), q[cut + int(rng.integers(0, 3)):]]).astype(np.uint8)
            if len(s) == 0:
                s = q[:1].copy()
        else:
            s = rng.integers(0, na, ls).astype(np.uint8)
        H = brute.sw_general(q, s, M, sc_p.gap_open, sc_p.gap_extend)
        want = brute.best_cell_column_major(H)
        assert oracle.score(q, s, sc) == want, (name, it)
        hsp, ops = oracle.align(q, s, sc)
        assert hsp.score == want[0]
        if hsp.score > 0:
            total, qe, se = brute.score_of_ops(q, s, hsp.q_begin, hsp.s_begin, ops, M, sc_p.gap_open, sc_p.gap_extend)
            assert (total, qe, se) == (hsp.score, hsp.q_end, hsp.s_end) == (want[0], want[1], want[2])
            hits += 1
    assert hits > 20
