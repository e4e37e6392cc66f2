"""CPU tests of the LCA rule with a top-percent cut (lx_compute_lca_ex) and of the tree check (lx_check_tax_tree): against
lx_compute_lca at top_percent 100, against the independent model of tests/lca_cases.py at every top percent, the refusals, and the
check on the trees lx_taxonomy_build makes and on trees with one rule broken at a time."""
import ctypes as C

import numpy as np
import pytest

from lambda_amd import capi
from tests import lca_cases
from tests.lca_cases import TOP_PERCENTS, crafted_lists, mixed_component_list, model_pairs, random_list, random_world, small_world
from tests.test_taxonomy import model_lca, taxdump


def all_lists():
    lists = dict(crafted_lists())
    lists["random, 20 000 rows"] = random_list()
    return lists


def test_abi_version_stays():
    assert capi.load().lx_abi_version() == 3
    o = capi.lca_options()
    assert o.top_percent == 100.0 and o.reserved == 0


def test_ex_at_100_is_compute_lca():
    for name, (w, rows) in all_lists().items():
        q0, l0 = capi.compute_lca(rows, *w.tree())
        q1, l1 = capi.compute_lca_ex(rows, *w.tree(), top_percent=100.0)
        assert np.array_equal(q0, q1) and np.array_equal(l0, l1), name
    # NULL options are the defaults
    w, rows = random_list()
    tree, keep = capi._tax_tree(*w.tree())
    qid, lca, cnt = np.zeros(len(rows), np.uint64), np.zeros(len(rows), np.uint32), C.c_uint64()
    assert capi.load().lx_compute_lca_ex(capi._ptr(rows), len(rows), C.byref(tree), None, capi._ptr(qid), capi._ptr(lca), C.byref(cnt)) == capi.LX_OK
    q0, l0 = capi.compute_lca(rows, *w.tree())
    assert np.array_equal(qid[:cnt.value], q0) and np.array_equal(lca[:cnt.value], l0)


@pytest.mark.parametrize("top", TOP_PERCENTS)
def test_ex_equals_model(top):
    for name, (w, rows) in all_lists().items():
        q, l = capi.compute_lca_ex(rows, *w.tree(), top_percent=top)
        mq, ml = model_pairs(rows, w, top)
        assert np.array_equal(q, mq), (name, top)
        assert np.array_equal(l, ml), (name, top, l[:20], ml[:20])


def test_crafted_lists_are_what_they_claim():
    lists, w = crafted_lists(), random_world()
    lca = lambda name, top: model_pairs(lists[name][1], lists[name][0], top)[1].tolist()
    assert lca("no starter at all", 100.0) == [0]
    assert lca("starter is the third record", 100.0)[0] not in (0, 1)
    # (the first subject's second taxon, 300, is folded in although its first one kept it from starting the fold)
    assert lca("starter: first taxon unassigned, a later one assigned", 100.0) == [model_lca(w.par_list, w.hgt_list, [[300], [500]])] != [500]
    deep = lca("deep against shallow, both orders", 100.0)
    assert deep[0] == deep[1] == 1 and w.heights[62] == 60
    # at the cut: the record at best * f is kept, the one below it is not; P = 100 takes in the far subject
    top = "top percent: at the cut, just below it, two best records"
    near = int(model_pairs(lca_cases.make_rows([(1, w.named["plain"], 1.0), (1, w.named["near"], 1.0)]), w, 100.0)[1][0])
    assert lca(top, 50.0)[0] == near and lca(top, 10.0)[1] == near and lca(top, 100.0)[0] != near
    assert lca(top, 0.0) == [500, 500, near, 500]
    ends = np.nonzero(np.diff(lists["wavefront and scan tile edges"][1]["n_qid"]))[0] + 1
    assert ends.tolist() == [63, 64, 65, 2047, 2048, 2049]
    # the random list means something: enough queries with an LCA below the root, enough that the cut changes
    rw, rows = random_list()
    l100, l10 = model_pairs(rows, rw, 100.0)[1], model_pairs(rows, rw, 10.0)[1]
    assert np.mean((l100 != 0) & (l100 != 1)) >= 0.25 and np.mean(l100 != l10) >= 0.1


def test_option_refusals():
    w, rows = random_list()
    for bad in (-1.0, 100.5, float("nan")):
        with pytest.raises(capi.LambdaExtError) as e:
            capi.compute_lca_ex(rows, *w.tree(), top_percent=bad)
        assert e.value.code == capi.LX_EINVAL and "top_percent" in str(e.value)
    for bits in (float("inf"), float("-inf"), float("nan")):
        r = rows[:200].copy()
        r["bit_score"][57] = bits
        with pytest.raises(capi.LambdaExtError) as e:
            capi.compute_lca_ex(r, *w.tree(), top_percent=99.0)
        assert e.value.code == capi.LX_EINVAL and "not finite" in str(e.value)
        q, l = capi.compute_lca_ex(r, *w.tree(), top_percent=100.0)  # bit scores are not looked at
        q0, l0 = capi.compute_lca(r, *w.tree())
        assert np.array_equal(l, l0)
    r = rows[:10].copy()
    r["n_sid"][3] = len(w.lists)
    for top in (100.0, 10.0):
        with pytest.raises(capi.LambdaExtError):
            capi.compute_lca_ex(r, *w.tree(), top_percent=top)


def test_mixed_components_are_einval():
    w, rows = mixed_component_list()
    for top in (100.0, 50.0):
        with pytest.raises(capi.LambdaExtError) as e:
            capi.compute_lca_ex(rows, *w.tree(), top_percent=top)
        assert e.value.code == capi.LX_EINVAL
    with pytest.raises(capi.LambdaExtError):
        capi.compute_lca(rows, *w.tree())
    # the cut takes the foreign record out
    q, l = capi.compute_lca_ex(rows, *w.tree(), top_percent=0.0)
    assert l.tolist() == [500, 500, 505]


def random_nodes_dmp(n, seed):
    rng = np.random.default_rng(seed)
    edges = [(1, 1)] + [(t, int(rng.integers(1, t))) for t in range(2, n + 1)]
    nodes = "".join(f"{a}\t|\t{b}\t|\tno rank\t|\t\t|\n" for a, b in edges).encode()
    names = "".join(f"{a}\t|\tn{a}\t|\t\t|\tscientific name\t|\n" for a, _ in edges).encode()
    return nodes, names


def test_check_admits_built_trees():
    nodes, names = taxdump()
    for present in ([5, 6], [9, 12, 5], [3, 9], [11], [5, 30], [12, 10, 8]):
        t = capi.taxonomy_build(nodes, names, present)
        capi.check_tax_tree(t["parents"], t["heights"], [0, len(present)], [p for p in present])
    nodes, names = random_nodes_dmp(10_000, 3)
    present = np.random.default_rng(4).integers(2, 10_001, 700)
    t = capi.taxonomy_build(nodes, names, present)
    assert t["max_height"] >= 5
    capi.check_tax_tree(t["parents"], t["heights"], np.arange(len(present) + 1), present)
    for w in (random_world(), small_world()):
        capi.check_tax_tree(*w.tree())
    assert random_world().parents[random_world().second_root] == 0 and (random_world().parents == random_world().second_root).sum() >= 1


def test_check_refuses_each_broken_rule():
    w = random_world()
    par, hgt, off, ids = (a.copy() for a in w.tree())
    n = len(par)

    def refused(p, h, o, i, text):
        with pytest.raises(capi.LambdaExtError) as e:
            capi.check_tax_tree(p, h, o, i)
        assert e.value.code == capi.LX_EINVAL and text in str(e.value), str(e.value)

    p = par.copy()
    p[1000] = n
    refused(p, hgt, off, ids, "parent of taxon 1000")
    h = hgt.copy()
    assert par[2000] > 1
    h[2000] += 1
    refused(par, h, off, ids, "height of taxon 2000")
    h = hgt.copy()
    assert par[2] == 1
    h[2] = 1
    refused(par, h, off, ids, "taxon 2 ")
    h = hgt.copy()
    h[n - 1] = 3  # (a disconnected taxon: parent 0)
    refused(par, h, off, ids, f"taxon {n - 1} ")
    i = ids.copy()
    i[17] = n
    refused(par, hgt, off, i, f"taxon {n} of a subject")
    o = off.copy()
    assert o[40] > 0
    o[41] = o[40] - 1
    refused(par, hgt, o, ids, "s_tax_off descends at subject 40")
    o = off.copy()
    o[0] = 1
    refused(par, hgt, o, ids, "does not start at 0")
    tree = capi.TaxTree(None, None, 0, None, None, 0)
    assert capi.load().lx_check_tax_tree(C.byref(tree)) == capi.LX_EINVAL and "NULL" in capi.last_output_error()
    assert capi.load().lx_check_tax_tree(None) == capi.LX_EINVAL
