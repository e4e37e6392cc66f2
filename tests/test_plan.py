"""The ONE selection function of the fused step (plan_step, lambda_amd/csrc/lx_step_plan.cpp) walked on the CPU through lx_plan_step:
query widths 1 ... 1 300 x query runs {0, 2, 4, 7, 8, 16, 24, 32} x the four scoring schemes of the reference's programs.  Every
choice must be the documented one for its (width, run, alphabet) and must satisfy its own preconditions: the panels hold the
query, the wavefront's LDS fits, compact codes only with gap costs they can hold, an int32 fix-up launch exactly where the
a-priori bound of the widest admitted query exceeds the codes' 2046 (or the sweep tests the codes after the fact).  A wrong
condition in the table sends a shape to a kernel half as fast without any parity test noticing -- this one does."""
import math

import pytest

from lambda_amd import capi
from tests.test_oracle import SCHEMES

RUNS = (0, 2, 4, 7, 8, 16, 24, 32)


def _expected(name, q, run, nrows):
    small = nrows <= 8  # nucleotide / bisulfite alphabets: two packed-half profiles cost no occupancy
    if run == 2:  # the free packing: pairs of one query, up to four queries per wavefront -- only the multi-query sweep serves it
        return capi.PLAN_MQ, 4
    if run == 0 or run % 4 != 0:
        return capi.PLAN_NO_SWEEP, None
    if run == 4:
        return capi.PLAN_MQ, 4
    if run % 16 != 0:  # 8, 24
        if not small or q > 208:
            return capi.PLAN_MQ, 2
        return capi.PLAN_HALF, (2 if q <= 152 else 1)
    if q <= 208:
        return capi.PLAN_HALF, 1
    return capi.PLAN_I16_COMPACT_WIDE, 1


@pytest.mark.parametrize("name", ["blosum62", "nucl", "bs_fwd", "bs_rev"])
def test_plan_table(name):
    sc = SCHEMES[name]
    nrows = (sc.alphabet_size + 1 + 3) // 4 * 4
    seen = set()
    for run in RUNS:
        for q in range(1, 1301):
            ls = q + 2 * (int(math.sqrt(q)) + 1)
            p = capi.plan_step(sc, q, ls, run, 1000)
            fam, qpw = _expected(name, q, run, nrows)
            assert p.family == fam, (name, q, run, p.family, p.name)
            if fam == capi.PLAN_NO_SWEEP:
                continue
            seen.add((p.family, p.group_lanes, p.strip_cols))
            assert p.queries_per_wavefront == qpw, (name, q, run, p.queries_per_wavefront, p.name)
            # preconditions of the choice
            assert p.group_lanes * p.strip_cols * p.panels >= q and p.group_lanes * p.strip_cols * (p.panels - 1) < q, (q, run, p.name)
            assert p.lds_bytes <= 64 * 1024, (q, run, p.lds_bytes)
            if fam == capi.PLAN_MQ:
                assert p.group_lanes == 8 and p.strip_cols in (11, 13, 19) and p.compact_codes == 1
                assert p.lds_bytes <= 20480  # four protein profiles + staging at two wavefronts per SIMD (eight per CU)
            if fam == capi.PLAN_HALF:
                assert p.panels == 1 and p.compact_codes == 1
                want_geo = (8, 13) if q <= 104 else (8, 19) if q <= 152 else (8, 25) if (q <= 200 and run % 16 == 0) else (16, 13)
                assert (p.group_lanes, p.strip_cols) == want_geo, (q, run, p.name)
            if fam == capi.PLAN_I16_COMPACT_WIDE:
                assert (p.group_lanes, p.strip_cols) == (8, 19) and p.panels == -(-q // 152) and p.compact_codes == 1
            if p.compact_codes:
                assert -sc.gap_open <= 31
            # a fix-up launch exactly where the widest admitted query can exceed what the codes hold, or the panels are several
            assert bool(p.may_decline) == (p.score_bound > 2046 or p.panels > 1), (q, run, p.score_bound, p.panels, p.name)
            assert p.slot_bytes > 0 and p.name.decode().startswith("lx::")
    assert len(seen) >= 7


def test_plan_follows_budget_survivors_and_switches():
    sc = SCHEMES["blosum62"]
    # a batch whose checkpoints do not fit the budget: no sweep
    assert capi.plan_step(sc, 150, 176, 32, 3_200_000, trace_bytes=1 << 30).family == capi.PLAN_NO_SWEEP
    assert capi.plan_step(sc, 150, 176, 32, 3_200_000).family == capi.PLAN_HALF
    # few survivors last time: the one-query-per-wavefront sweep gives way to mode 1, the multi-query plan keeps its sweep
    p = capi.plan_step(sc, 150, 176, 32, 3_200_000, survivor_share=0.01)
    assert p.family == capi.PLAN_NO_SWEEP and p.adapted == 1
    assert capi.plan_step(sc, 150, 176, 32, 3_200_000, survivor_share=0.01, adapt_permille=0).family == capi.PLAN_HALF
    assert capi.plan_step(sc, 150, 176, 32, 3_200_000, survivor_share=0.2).family == capi.PLAN_HALF
    assert capi.plan_step(sc, 150, 176, 4, 100_000, survivor_share=0.01).family == capi.PLAN_MQ
    # the options: LX_OPT_MQ_SWEEP = 0 / 2, LX_OPT_PACKED_HALF = 0, LX_OPT_PASS2_MODE
    assert capi.plan_step(sc, 150, 176, 8, 1000, mq_sweep=0).family == capi.PLAN_HALF  # two profiles per wavefront at reduced occupancy
    assert capi.plan_step(sc, 150, 176, 2, 1000, mq_sweep=0).family == capi.PLAN_NO_SWEEP  # pairs have no other sweep
    assert b"free packing" in capi.plan_step(sc, 150, 176, 2, 1000).name
    assert capi.plan_step(sc, 150, 176, 32, 1000, mq_sweep=2).family == capi.PLAN_MQ
    assert capi.plan_step(sc, 150, 176, 32, 1000, packed_half=0).family == capi.PLAN_INT32
    assert capi.plan_step(sc, 150, 176, 32, 1000, pass2_mode=1).family == capi.PLAN_NO_SWEEP
    # gap costs beyond the compact codes (first character dearer than 31): int16-pair slots
    wide_gap = capi.builtin_scoring(62, gap_open=-35, gap_extend=-1)
    p = capi.plan_step(wide_gap, 150, 176, 32, 1000)
    assert p.family in (capi.PLAN_I16_PAIRS, capi.PLAN_INT32) and p.compact_codes == 0
    assert capi.plan_step(wide_gap, 150, 176, 4, 1000).family == capi.PLAN_NO_SWEEP


# one scheme per alphabet size: proteins (27 letters) and nucleotides (5).  The nucleotide one has an odd match score: with +2 / -2 the
# a-priori bound is always even and never IS 2047.
EDGE_SCHEMES = {
    "protein": dict(method=62, gap_open=-11, gap_extend=-1),
    "nucleotide": dict(method=0, match=3, mismatch=-3, gap_open=-5, gap_extend=-2),
}


@pytest.mark.parametrize("alphabet", list(EDGE_SCHEMES))
@pytest.mark.parametrize("run", [32, 4])  # the packed-half sweep; the multi-query sweep
def test_may_decline_flips_between_bounds_2046_and_2047(alphabet, run):
    """score_bound (lx_step_plan.cpp), the a-priori bound of the widest admitted query: a one-panel packed sweep needs no int32 fix-up
    launch up to 2046 -- what the compact codes hold -- and needs one from 2047 on.  Widths x window lengths are walked until both
    values have turned up, so the flip is shown between neighbours and not merely somewhere."""
    sc = capi.builtin_scoring(**EDGE_SCHEMES[alphabet])
    want_family = capi.PLAN_HALF if run == 32 else capi.PLAN_MQ
    seen = {}
    for q in range(20, 153):
        for k in range(8, 128):
            p = capi.plan_step(sc, q, 16 * k - 7, run, 1000)  # (16 k steps of 8-lane groups)
            if p.score_bound not in (2045, 2046, 2047, 2048) or p.panels != 1:
                continue
            assert p.family == want_family and p.compact_codes == 1, (q, k, p.name)
            assert bool(p.may_decline) == (p.score_bound > 2046), (q, k, p.score_bound, p.may_decline)
            assert (b"int32 fix-up" in p.name) == (p.score_bound > 2046), (q, k, p.name)
            seen[p.score_bound] = seen.get(p.score_bound, 0) + 1
    assert seen.get(2046, 0) > 0 and seen.get(2047, 0) > 0, seen


@pytest.mark.parametrize("alphabet", list(EDGE_SCHEMES))
def test_compact_codes_flip_between_gap_open_31_and_32(alphabet):
    """compact_gaps_ok (lx_step_plan.cpp): the 5-bit gap field of the compact checkpoint codes holds a first gap character of up to 31.
    At -31 the packed-half and the multi-query sweep run with compact codes; at -32 the one-query sweep writes int16 pairs and the
    multi-query sweep, which has no other slots for one panel, does not apply."""
    kw = dict(EDGE_SCHEMES[alphabet])
    fits = capi.builtin_scoring(**dict(kw, gap_open=-31 - kw["gap_extend"]))
    beyond = capi.builtin_scoring(**dict(kw, gap_open=-32 - kw["gap_extend"]))
    assert (fits.gap_open, beyond.gap_open) == (-31, -32)  # (the scheme's gap_open is the cost of a gap's first character)
    for q, ls in ((100, 122), (150, 176), (200, 230), (400, 442)):
        p = capi.plan_step(fits, q, ls, 32, 1000)
        assert p.family in (capi.PLAN_HALF, capi.PLAN_I16_COMPACT_WIDE) and p.compact_codes == 1, (q, p.name)
        p = capi.plan_step(beyond, q, ls, 32, 1000)
        assert p.family in (capi.PLAN_I16_PAIRS, capi.PLAN_INT32) and p.compact_codes == 0, (q, p.name)
        assert capi.plan_step(fits, q, ls, 4, 1000).family == capi.PLAN_MQ
        assert capi.plan_step(beyond, q, ls, 4, 1000).family == capi.PLAN_NO_SWEEP


def test_solo_packing_only_where_sixteen_profiles_fit():
    """LX_OPT_QUERY_RUN = 1 -- no promise, a byte profile per window (lx_sweep_mq.hip's solo packing) -- is served where 16 profiles
    fit a wavefront's share of the LDS: nucleotide and bisulfite schemes (5 letters + pad), one to several panels; 16 protein
    profiles (27 letters) do not fit, and there 1 is what 0 is: no promise, no sweep."""
    prot = capi.builtin_scoring(62, gap_open=-11, gap_extend=-1)
    for lq in (100, 150, 300, 900):
        pl = capi.plan_step(prot, lq, lq + 30, 1, 10_000)
        assert "sweep_mq_kernel" not in pl.name.decode()
    for method in (0, -1, -2):
        sc = capi.builtin_scoring(method, match=2, mismatch=-3, gap_open=-5, gap_extend=-2)
        for lq, slen in ((100, 130), (150, 176), (150, 2000), (400, 450), (1000, 1100)):
            pl = capi.plan_step(sc, lq, slen, 1, 10_000)
            name = pl.name.decode()
            assert "solo packing: up to 16 queries per wavefront" in name, (method, lq, name)
            assert pl.queries_per_wavefront == 16 and pl.lds_bytes <= 20 * 1024 and pl.compact_codes == 1
            assert pl.panels * pl.group_lanes * pl.strip_cols >= lq
            # a fix-up launch exactly where the a-priori bound exceeds the codes or the panels are several
            assert bool(pl.may_decline) == (pl.score_bound > 2046 or pl.panels > 1), (lq, slen, pl.score_bound)
            assert ("int32 fix-up" in name) == bool(pl.may_decline)
