"""The free-packing plan made on the device (lambda_amd/csrc/lx_plan_free.hip) against the sequential model of its rules
(tests/plan_model.py), EXACTLY: every plan word with its filler bit, every wavefront's columns per lane and longest window, and the
report's wavefronts, runs, quads and ranges.  tests/test_gpu_plan.py checks that a plan is valid; this file checks that it is the plan
the rules describe -- the rank, the thresholds, the sort keys, the closing rule and the tie-breaks change no promise when they are
wrong, only what the sweep costs.  The lists (plan_model.CASES) sit on the kernels' own constants; tests/test_plan_model.py asserts on
the model that each meets its condition.  Integers throughout: no tolerance."""
import numpy as np
import pytest

from lambda_amd import capi
from tests import plan_model as pm
from tests.test_gpu_plan import check_plan, on_device

pytestmark = pytest.mark.gpu

CASE_C = [(name, C) for name in pm.CASES for C in pm.get_case(name).Cs]


def assert_equals_model(got, m, nranges):
    plan, pan, maxs, rep = got
    want = pm.report_of(m, nranges)
    assert rep[: len(want)].tolist() == want, (rep[: len(want)].tolist(), want)
    assert plan.shape == m.plan.shape
    bad = np.nonzero((plan != m.plan).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} wavefronts differ, the first is {bad[0]} ({m.kind[bad[0]]}): device {[hex(x) for x in plan[bad[0]]]}, model {[hex(x) for x in m.plan[bad[0]]]}"
    assert (pan == m.wf_pan).all() and (maxs == m.wf_maxs).all()


@pytest.mark.parametrize("name,C", CASE_C)
def test_the_device_plan_is_the_models(handle, name, C):
    c = pm.get_case(name)
    got = handle.plan_free_packing_dev(on_device(c.ext), c.n, c.n_qseq, strip_cols=C, cuts=c.cuts)
    check_plan(c.ext, *got, c.cuts, C)
    assert_equals_model(got, pm.model_of(name, C), len(c.cuts) - 1)


def test_more_runs_than_the_run_bound_is_an_error_not_a_plan(handle):
    """40 one-window queries planned as 36: 40 runs against run-sized arrays made for fp_run_bound(40, 36) = 38.  The plan refuses
    (LX_ESTATE, the message names the run bound); the handle then plans the same list, stated rightly, as the model does."""
    c = pm.get_case("closing_65_one_window_queries")
    ext = c.ext[:40].copy()
    d_ext = on_device(ext)
    with pytest.raises(capi.LambdaExtError) as e:
        handle.plan_free_packing_dev(d_ext, 40, 36)
    assert e.value.code == capi.LX_ESTATE and "run bound 38" in str(e.value), str(e.value)
    got = handle.plan_free_packing_dev(d_ext, 40, 40)
    check_plan(ext, *got, [0, 40])
    assert_equals_model(got, pm.plan_model(ext, [0, 40]), 1)
