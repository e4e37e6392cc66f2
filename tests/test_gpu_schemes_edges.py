"""The scoring schemes lx_set_scoring says it accepts, at their extremes, through the kernels -- and the ones it must refuse.

Accepted: entries of +100 and -100, gap_open -120 with gap_extend -27, gap_open == gap_extend at -1 and -27, alphabets of 1 and 31
letters (pass 1, ragged lengths 1 - 700 and windows on both sides of the 1100 rows where 27 x rows alone passes the 16-bit sweeps'
29695); matrix - gap_extend at -31 and +31, matrix - gap_open at 0 (the multi-query sweep's byte profiles) and at -1 (no byte
profiles) through the fused step.  (matrix - gap_open = 255 cannot be reached: entries end at 100, gap_open at -120.)
Refused: entries of +-101, gap_open -121, gap_extend -28 and 0, gap_open > gap_extend, alphabets of 0 and 32 letters -- LX_EINVAL, the
scheme in force stays; matrix - gap_extend = 32 scores in pass 1 and is refused by pass 2."""
import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import limit_cases, oracle_lib
from tests.limit_gpu import check_rows, dev_scores, oracle_results, pack_runs, run_dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["entries_pm100", "gaps_120_27", "open_eq_extend_1", "open_eq_extend_27", "alphabet_1", "alphabet_31"])
def test_accepted_extremes_score_pass(handle, oracle, name):
    sc = limit_cases.make_scoring(*limit_cases.extreme_schemes()[name])
    na = sc.alphabet_size
    q, s, ext = synth.make_ragged_np(500, seed=11, alphabet=np.arange(na, dtype=np.uint8), lq_range=(1, 700), ls_extra=(0, 90))
    # windows of 1000 - 1200 rows for a few wide queries: |ge| x rows on both sides of the 16-bit sweeps' limit when ge = -27
    wide = np.nonzero(ext["q_len"] > 300)[0][:12]
    extra = ext[wide].copy()
    rng = np.random.default_rng(5)
    long_s = rng.integers(0, na, 12 * 1200).astype(np.uint8)
    for k, i in enumerate(wide):
        ql = int(ext["q_len"][i])
        long_s[k * 1200 + 100: k * 1200 + 100 + ql] = q[int(ext["q_off"][i]): int(ext["q_off"][i]) + ql]
    extra["s_off"] = len(s) + 1200 * np.arange(12)
    extra["s_len"] = np.linspace(1000, 1200, 12).astype(np.uint32)
    s, ext = np.concatenate([s, long_s]), np.concatenate([ext, extra])
    want = oracle.score_batch(q, s, ext, oracle_lib.scoring_from(sc), threads=8)
    handle.set_scoring(sc, 0)
    try:
        got = handle.score_batch(q, s, ext)
        uni = ext[-12:].copy()  # runs of 16 of one width: the packed kernels (or their refusal) see the long windows too
        uni = np.repeat(uni, 16)
        got16, name16 = dev_scores(handle, q, s, uni, 16, 1)
    finally:
        handle.set_scoring(limit_cases.blosum62(), 0)
    assert (got == want).all(), (name, np.nonzero(got != want)[0][:8])
    assert (got16 == np.repeat(want[-12:], 16)).all(), (name, name16)
    assert want.max() > (50 if na > 1 else 0)


@pytest.mark.parametrize("name,mq_expected", [("adj_pm31", False), ("b8_0", True), ("b8_m1", False)])
def test_accepted_extremes_fused_step(handle, oracle, name, mq_expected):
    """matrix - gap_extend exactly -31 and +31 (what pass 2's int8 table holds), matrix - gap_open exactly 0 (the byte profiles' lowest
    entry) and -1 (no byte profiles: the multi-query sweep must not run, the results stay exact)."""
    sc = limit_cases.make_scoring(*limit_cases.extreme_schemes()[name])
    M = sc.matrix_np()[:4, :4].astype(int)
    if name == "adj_pm31":
        assert (M - sc.gap_extend).min() == -31 and (M - sc.gap_extend).max() == 31
    else:
        assert (M - sc.gap_open).min() == (0 if name == "b8_0" else -1) and (M - sc.gap_extend).max() == 31
    handle.set_scoring(sc, 0)
    try:
        osc = oracle_lib.scoring_from(sc)
        q, s, ext = synth.make_ragged_lists_np(40, seed=12, alphabet=np.arange(4, dtype=np.uint8), lq_range=(60, 260), mean_windows=5.0,
                                               merged_frac=0.15, sub_rate=0.1)
        slots = pack_runs(ext, 4)
        score, fhsp, off, fops, kernel = run_dev(handle, q, s, slots, 4, 40, 2, mq=2)
        assert ("sweep_mq_kernel" in kernel) == mq_expected, kernel
        check_rows(oracle_results(oracle, "edge_" + name, sc, q, s, slots, 40), score, fhsp, off, fops, kernel)
        hsp, ops = handle.align_batch(q, s, ext[:64])
        for g, o, (oh, oops) in zip(hsp, ops, oracle.align_batch(q, s, ext[:64], osc)):
            assert (g["score"], g["q_begin"], g["q_end"], g["s_begin"], g["s_end"], g["n_ops"]) == (oh.score, oh.q_begin, oh.q_end, oh.s_begin, oh.s_end, oh.n_ops)
            assert o == oops
    finally:
        handle.set_scoring(limit_cases.blosum62(), 0)


def _m4(d, off):
    m = np.full((4, 4), off, dtype=np.int64)
    m[np.arange(4), np.arange(4)] = d
    return m


REFUSED = {"entry_101": (_m4(101, -4), -12, -1, None), "entry_m101": (_m4(5, -101), -12, -1, None), "gap_open_m121": (_m4(5, -4), -121, -1, None),
           "gap_extend_m28": (_m4(5, -4), -30, -28, None), "gap_extend_0": (_m4(5, -4), -5, 0, None), "open_above_extend": (_m4(5, -4), -1, -2, None),
           "alphabet_0": (_m4(5, -4), -12, -1, 0), "alphabet_32": (_m4(5, -4), -12, -1, 32)}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_schemes_leave_the_scheme_in_force(handle, oracle, name):
    b62 = limit_cases.blosum62()
    handle.set_scoring(b62, 0)
    m, go, ge, alph = REFUSED[name]
    with pytest.raises(capi.LambdaExtError) as e:
        handle.set_scoring(limit_cases.make_scoring(m, go, ge, alphabet_size=alph), 0)
    assert e.value.code == capi.LX_EINVAL
    q, s, ext = synth.make_batch_np(8, 150, 16, seed=3)
    assert (handle.score_batch(q, s, ext) == oracle.score_batch(q, s, ext, oracle_lib.scoring_from(b62), threads=4)).all()


def test_the_last_accepted_neighbours_of_the_refused_schemes(handle):
    """The other side of each refusal: 100 / -100, -120, -27, gap_open == gap_extend, alphabets of 1 and 31 letters are taken."""
    try:
        for m, go, ge, alph in ((_m4(100, -100), -12, -1, None), (_m4(5, -4), -120, -1, None), (_m4(5, -4), -30, -27, None), (_m4(5, -4), -2, -2, None),
                                (_m4(5, -4), -12, -1, 1), (np.zeros((31, 31), dtype=np.int64) - 1, -12, -1, 31)):
            handle.set_scoring(limit_cases.make_scoring(m, go, ge, alphabet_size=alph), 0)
    finally:
        handle.set_scoring(limit_cases.blosum62(), 0)


def test_matrix_minus_gap_extend_32_scores_but_is_not_traced(handle, oracle):
    sc = limit_cases.refused_v_minus_ge_32()
    assert (sc.matrix_np()[:4, :4].astype(int) - sc.gap_extend).max() == 32
    q, s, ext = synth.make_batch_np(8, 150, 16, seed=4, alphabet=np.arange(4, dtype=np.uint8), sub_rate=0.1)
    want = oracle.score_batch(q, s, ext, oracle_lib.scoring_from(sc), threads=4)
    handle.set_scoring(sc, 0)
    try:
        assert (handle.score_batch(q, s, ext) == want).all() and want.max() > 1000
        with pytest.raises(capi.LambdaExtError, match="gap_extend") as e:
            handle.align_batch(q, s, ext)
        assert e.value.code == capi.LX_EINVAL
        for mode in (2, 1, 0):
            handle.set_option(capi.LX_OPT_PASS2_MODE, mode)
            with pytest.raises(capi.LambdaExtError) as e:
                handle.extend_batch(q, s, ext, 60)
            assert e.value.code == capi.LX_EINVAL
    finally:
        handle.set_option(capi.LX_OPT_PASS2_MODE, 1)
        handle.set_scoring(limit_cases.blosum62(), 0)
    # the handle still works
    b62 = limit_cases.blosum62()
    q, s, ext = synth.make_batch_np(8, 150, 16, seed=3)
    want = oracle.score_batch(q, s, ext, oracle_lib.scoring_from(b62), threads=4)
    score, hsp, off, ops = handle.extend_batch(q, s, ext, 60)
    assert (score == want).all() and (hsp["n_ops"][want >= 60] > 0).all()
