"""GPU tests of the LCA on the device (lx_lca.hip through lx_compute_lca_dev): the pairs of lx_compute_lca_ex in order and count on
the crafted lists of tests/lca_cases.py at every top percent, on a random list of 20 000 rows and under three settings of
LX_OPT_LCA_RANGE_ROWS; the refusals before any device work (no launch of phase 13), the reference's text for a query whose taxa
have no common ancestor, and lx_tax_dev_create's refusal of every tree lx_check_tax_tree refuses -- no kernel is given such a tree."""
import numpy as np
import pytest

from lambda_amd import capi
from tests.lca_cases import NO_ROOT, TOP_PERCENTS, crafted_lists, mixed_component_list, model_pairs, random_list, random_world, small_world

pytestmark = pytest.mark.gpu

RANGES = (0, 64, 1)  # LX_OPT_LCA_RANGE_ROWS: the default, and ranges so small that every cut of the lists is exercised


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


@pytest.fixture(scope="module")
def trees(handle):
    """the two trees resident on the handle's device, by world"""
    with capi.TaxDev(handle, *random_world().tree()) as big, capi.TaxDev(handle, *small_world().tree()) as small:
        yield {id(random_world()): big, id(small_world()): small}


@pytest.fixture(scope="module")
def expected():
    """lx_compute_lca_ex on every list at every top percent, computed once"""
    lists = dict(crafted_lists())
    lists["random, 20 000 rows"] = random_list()
    return lists, {(name, top): capi.compute_lca_ex(rows, *w.tree(), top_percent=top) for name, (w, rows) in lists.items() for top in TOP_PERCENTS}


def set_range(handle, rows):
    handle.set_option(capi.LX_OPT_LCA_RANGE_ROWS, rows)
    assert handle.get_option(capi.LX_OPT_LCA_RANGE_ROWS) == rows


@pytest.mark.parametrize("range_rows", RANGES)
def test_device_equals_host(handle, trees, expected, range_rows):
    lists, want = expected
    set_range(handle, range_rows)
    try:
        for name, (w, rows) in lists.items():
            for top in TOP_PERCENTS:
                q, l = handle.compute_lca_dev(trees[id(w)], rows, top_percent=top)
                wq, wl = want[(name, top)]
                assert len(q) == len(wq) == len(l) and np.array_equal(q, wq), (name, top, range_rows)
                assert np.array_equal(l, wl), (name, top, range_rows, np.nonzero(l != wl)[0][:10])
                ms, launches = handle.last_phase_ms(13)
                if len(rows):
                    assert launches >= 1 and ms > 0, (name, top)
                    if range_rows == 1:  # every query is a range of its own (a call keeps the events of its first 512 phase brackets)
                        assert launches == min(len(wq), 512)
                else:
                    assert launches == 0
    finally:
        set_range(handle, 0)


def test_random_list_means_something(expected):
    """asserted on the model, so that a pass of the comparison above says something"""
    w, rows = random_list()
    l100, l10 = model_pairs(rows, w, 100.0)[1], model_pairs(rows, w, 10.0)[1]
    assert np.mean((l100 != 0) & (l100 != 1)) >= 0.25
    assert np.mean(l100 != l10) >= 0.1
    lists, want = expected
    for top in (100.0, 10.0):
        assert np.array_equal(want[("random, 20 000 rows", top)][1], model_pairs(rows, w, top)[1])


def test_mixed_components(handle, trees):
    w, rows = mixed_component_list()
    for top in (100.0, 50.0):
        with pytest.raises(capi.LambdaExtError) as e:
            handle.compute_lca_dev(trees[id(w)], rows, top_percent=top)
        assert e.value.code == capi.LX_EINVAL and NO_ROOT in str(e.value)
        assert handle.last_phase_ms(13)[1] == 1  # (the fold ran: the verdict is the kernel's)
    q, l = handle.compute_lca_dev(trees[id(w)], rows, top_percent=0.0)
    assert l.tolist() == [500, 500, 505]


def test_refused_before_device_work(handle, trees):
    w, rows = random_list()
    tax = trees[id(w)]
    handle.compute_lca_dev(tax, rows[:100])
    assert handle.last_phase_ms(13)[1] == 1

    def refused(text, *a, **kw):
        with pytest.raises(capi.LambdaExtError) as e:
            handle.compute_lca_dev(*a, **kw)
        assert e.value.code == capi.LX_EINVAL and text in str(e.value), str(e.value)
        assert handle.last_phase_ms(13) == (0.0, 0)

    r = rows[:5000].copy()
    r["n_sid"][4321] = len(w.lists)
    refused("row 4321", tax, r)
    handle.compute_lca_dev(tax, rows[:100])
    for bad in (-1.0, 100.5, float("nan")):
        refused("top_percent", tax, rows, top_percent=bad)
    r = rows[:5000].copy()
    r["bit_score"][77] = float("inf")
    refused("not finite", tax, r, top_percent=50.0)
    q, l = handle.compute_lca_dev(tax, r, top_percent=100.0)  # (at 100 the bit scores are not looked at)
    assert np.array_equal(l, capi.compute_lca(r, *w.tree())[1])
    refused("NULL", None, rows)
    with capi.Handle(0) as other:
        with pytest.raises(capi.LambdaExtError) as e:
            other.compute_lca_dev(tax, rows)
        assert e.value.code == capi.LX_EINVAL and "another handle" in str(e.value)
        assert other.last_phase_ms(13) == (0.0, 0)


def test_create_refuses_what_the_check_refuses(handle):
    w = random_world()
    par, hgt, off, ids = (a.copy() for a in w.tree())
    n = len(par)
    broken = []
    p = par.copy()
    p[1000] = n
    broken.append((p, hgt, off, ids))
    h = hgt.copy()
    h[2000] += 1
    broken.append((par, h, off, ids))
    h = hgt.copy()
    h[2] = 1
    broken.append((par, h, off, ids))
    i = ids.copy()
    i[17] = n
    broken.append((par, hgt, off, i))
    o = off.copy()
    o[41] = o[40] - 1
    broken.append((par, hgt, o, ids))
    for tree in broken:
        with pytest.raises(capi.LambdaExtError) as eh:
            capi.check_tax_tree(*tree)
        with pytest.raises(capi.LambdaExtError) as ed:
            capi.TaxDev(handle, *tree)
        assert ed.value.code == capi.LX_EINVAL and str(eh.value).split(": ", 1)[1] in str(ed.value)
