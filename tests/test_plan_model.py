"""The sequential model of the free-packing plan (tests/plan_model.py) on its own, without a GPU: the model's plan keeps every promise
the sweep kernel relies on (tests.test_gpu_plan.check_plan, the same function the device's plan is held against), every case list
meets the condition it was made for -- asserted on the model, as tests/test_gpu_pair_slots.py asserts its conditions on the oracle --,
and the plan's bound holds.  tests/test_gpu_plan_edges.py then compares the device's plan with this model word for word."""
import numpy as np
import pytest

from lambda_amd import capi
from tests import plan_model as pm
from tests.test_gpu_plan import check_plan
from tests.test_gpu_plan import cols_per_lane as cols_per_lane_of_the_promises

CASE_C = [(name, C) for name in pm.CASES for C in pm.get_case(name).Cs]


def test_the_model_reads_the_records_the_library_reads():
    assert pm.EXT_DTYPE == capi.EXT_DTYPE


@pytest.mark.parametrize("C", (19, 13, 11))
def test_columns_per_lane_two_statements_agree(C):
    assert all(pm.cols_per_lane(lq, C) == cols_per_lane_of_the_promises(lq, C) for lq in range(0, 5000))


def test_key16_regions():
    lc = lambda l: 255 - (pm.key16(0, l) & 0xff)
    assert [lc(l) for l in (0, 7, 8, 1016, 1023, 1024, 1087, 1088, 9151, 9152, 20000, 0x7fffffff)] == [0, 0, 1, 127, 127, 128, 128, 129, 254, 255, 255, 255]
    assert all(lc(l) <= lc(l + 1) for l in range(0, 10000))  # (coarse, never out of order)
    assert [pm.key16(p, 0) >> 8 for p in (0, 1, 254, 255, 256, 0xfff)] == [255, 254, 1, 0, 0, 0]


@pytest.mark.parametrize("name,C", CASE_C)
def test_the_models_plan_keeps_the_promises(name, C):
    c = pm.get_case(name)
    m = pm.model_of(name, C)
    rep = np.zeros(16, np.uint32)
    rep[: 5 + len(c.cuts) - 1] = pm.report_of(m, len(c.cuts) - 1)
    check_plan(c.ext, m.plan, m.wf_pan, m.wf_maxs, rep, c.cuts, C)


@pytest.mark.parametrize("name", list(pm.CASES))
def test_the_case_meets_its_condition(name):
    c = pm.get_case(name)
    c.expect(pm.model_of(name, c.Cs[0]))


@pytest.mark.parametrize("name,C", CASE_C)
def test_the_plan_stays_within_its_bound(name, C):
    c = pm.get_case(name)
    m = pm.model_of(name, C)
    assert m.nwf <= capi.load().lx_plan_free_packing_bound(c.n, c.n_qseq, len(c.cuts) - 1)
    assert m.nruns <= min(c.n, c.n_qseq) + c.n // pm.RUN_CUT + 2  # (fp_run_bound: what the run-sized arrays are made for)


def test_facts_of_the_triage():
    """A run of 400/176/176/176/60: two quads, the short one of a single window, no pairs.  513 equal windows of one query: two runs in
    33 wavefronts.  65 one-window queries: 17 wavefronts."""
    m = pm.plan_model(pm.make_ext([(150, [400, 176, 176, 176, 60])]), [0, 5])
    assert [len(q) for _, q in m.quads] == [4, 1] and not m.runs[0].pairs and m.nwf == 1
    assert (m.plan[0] == [0, 1, 2, 3, 4] + [4 | pm.FILLER] * 11).all()
    m = pm.model_of("run_cut_513_equal", 19)
    assert (m.nruns, m.nwf) == (2, 33)
    assert pm.model_of("closing_65_one_window_queries", 19).nwf == 17
