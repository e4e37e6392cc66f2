"""What the LCA tests share (tests/test_lca_abi.py, tests/test_gpu_lca.py, tests/test_gpu_lca_cli.py): the trees, an independent
model of the rule of lx_compute_lca_ex -- tests/test_taxonomy.py's model_lca over the hits a small function keeps under the
top-percent rule, written from include/lambda_ext.h, not from the library --, and the crafted and random record lists."""
import functools

import numpy as np

from lambda_amd import capi
from tests.test_taxonomy import model_lca, model_tree, taxdump

TOP_PERCENTS = (100.0, 50.0, 10.0, 0.0)
NO_ROOT = "LCA-computation error: One of the paths didn't lead to root."
SCAN_TILE = 2048  # kL2ScanTile


# ---- the trees ----------------------------------------------------------------------------------------------------------------
def heights_of(par):
    """lx_taxonomy_build's step 4: the heights counted from the final parents"""
    hgt = []
    for i in range(len(par)):
        h, cur = 0, int(par[i])
        while cur > 1:
            cur = int(par[cur])
            h += 1
        hgt.append(h)
    return np.array(hgt, np.uint32)


@functools.lru_cache(maxsize=None)
def small_world():
    """the tree of tests/test_taxonomy.py::taxdump() through model_tree, and subjects over it"""
    nodes, names = taxdump()
    mt = model_tree(nodes, names, [5, 6, 9, 12, 10, 11])
    lists = [[5], [6], [9], [12], [10], [11], [], [5, 9], [1], [6, 5, 4]]
    return World(mt["parents"], mt["heights"], lists)


class World:
    """a tree and the subjects' taxon lists; names for subjects the crafted lists need"""

    def __init__(self, parents, heights, lists, **named):
        self.parents, self.heights, self.lists = np.asarray(parents, np.uint32), np.asarray(heights, np.uint32), [list(x) for x in lists]
        self.off = np.cumsum([0] + [len(x) for x in self.lists]).astype(np.uint64)
        self.ids = np.array([t for x in self.lists for t in x], np.uint32)
        self.named = named
        self.par_list, self.hgt_list = self.parents.tolist(), self.heights.tolist()  # (the model walks them entry by entry)

    def tree(self):
        return self.parents, self.heights, self.off, self.ids


@functools.lru_cache(maxsize=None)
def random_world(seed=11, n=5000, n_s=600):
    """About 5 000 taxa: a chain of 60 below the root, clades of near-by ids with heights of at most 60, a second root (a taxon
    without a parent that has descendants) and a few disconnected taxa (parent 0).  Subject s's taxa lie near 63 + s * step, so
    that neighbouring subjects have neighbouring taxa; some subjects have none, some two or three, some an unassigned one."""
    rng = np.random.default_rng(seed)
    par = np.zeros(n, np.int64)
    par[1] = 1
    for t in range(2, 63):  # 2 <- 1, 3 <- 2, ...: taxon 62 has height 60
        par[t] = t - 1
    main_end, second_root = n - 220, n - 220
    hgt = np.zeros(n, np.int64)
    for t in range(2, 63):
        hgt[t] = 0 if par[t] <= 1 else hgt[par[t]] + 1
    for t in range(63, main_end):
        p = 1 if rng.random() < 0.004 else int(rng.integers(max(63, t - 40), t)) if t > 63 else 1
        if p > 1 and hgt[p] >= 59:  # (a clade that has reached 60 levels goes on 40 levels further up)
            for _ in range(40):
                p = int(par[p])
        par[t] = p
        hgt[t] = 0 if p <= 1 else hgt[p] + 1
    par[second_root] = 0
    for t in range(second_root + 1, n - 20):
        par[t] = int(rng.integers(second_root, t))
    # (the last 20 taxa keep parent 0: disconnected)
    heights = heights_of(par)
    assert heights.max() == 60 and heights[62] == 60
    disconnected = n - 5
    lists = []
    step = (main_end - 63 - 10) / n_s
    for s in range(n_s):
        c = 63 + int(s * step)
        r = rng.random()
        k = 0 if r < 0.08 else 1 if r < 0.8 else 2 if r < 0.92 else 3
        taxa = [c + int(x) for x in rng.integers(0, 8, k)]
        if k and rng.random() < 0.05:
            taxa[int(rng.integers(0, k))] = disconnected
        lists.append(taxa)
    shallow = next(t for t in range(63, main_end) if heights[t] == 1)
    named = {}
    for name, taxa in [("none", []), ("root", [1]), ("unassigned_first", [disconnected, 300]), ("three", [400, 410, 395]), ("deep", [62]),
                       ("shallow", [shallow]), ("other", [second_root + 7]), ("disconnected", [disconnected]), ("plain", [500]),
                       ("near", [505]), ("far", [3000])]:
        named[name] = len(lists)
        lists.append(taxa)
    w = World(par, heights, lists, **named)
    w.second_root = second_root
    return w


# ---- the model ----------------------------------------------------------------------------------------------------------------
def kept_under(bits, top_percent):
    """which records of one query enter its LCA (lx_lca_options)"""
    if top_percent == 100.0:
        return [True] * len(bits)
    best = max(bits)
    f = 1.0 - top_percent / 100.0
    cut = best * f
    return [b >= cut or b == best for b in bits]


def model_pairs(rows, world, top_percent):
    """(n_qid, lca) per maximal run of equal n_qid"""
    qids, lcas = [], []
    lo = 0
    while lo < len(rows):
        hi = lo + 1
        while hi < len(rows) and rows["n_qid"][hi] == rows["n_qid"][lo]:
            hi += 1
        keep = kept_under([float(b) for b in rows["bit_score"][lo:hi]], top_percent)
        hits = [world.lists[int(s)] for s, k in zip(rows["n_sid"][lo:hi], keep) if k]
        qids.append(int(rows["n_qid"][lo]))
        lcas.append(int(model_lca(world.par_list, world.hgt_list, hits)))
        lo = hi
    return np.array(qids, np.uint64), np.array(lcas, np.uint32)


# ---- the lists ----------------------------------------------------------------------------------------------------------------
def make_rows(triples):
    """(n_qid, n_sid, bit_score) triples as lx_blast_match rows"""
    m = np.zeros(len(triples), capi.BLAST_MATCH_DTYPE)
    if len(triples):
        q, s, b = zip(*triples)
        m["n_qid"], m["n_sid"], m["bit_score"] = q, s, b
    return m


def crafted_lists():
    """name -> (world, rows): every list is folded at every top percent"""
    w, sw = random_world(), small_world()
    N = w.named
    rng = np.random.default_rng(5)
    out = {}

    def near(base, k, qid, top=200.0):
        """k records on subjects around `base`, bit scores descending"""
        return [(qid, int(min(599, max(0, base + int(o)))), top - 7.0 * i) for i, o in enumerate(rng.integers(-3, 4, k))]

    out["n = 0"] = (w, make_rows([]))
    out["one record"] = (w, make_rows([(7, 100, 50.0)]))
    out["a query of one record between two others"] = (w, make_rows(near(50, 3, 1) + near(300, 1, 2) + near(420, 4, 3)))
    out["a repeated n_qid later in the list"] = (w, make_rows(near(50, 2, 1) + near(300, 2, 2) + near(400, 2, 1)))
    out["all taxa equal"] = (w, make_rows([(4, N["plain"], 90.0 - i) for i in range(5)]))
    # rows end at 63, 64, 65, 2047, 2048, 2049; then a query across the scan tile edge at 4096
    t, q, at = [], 0, 0
    for end in (63, 64, 65, 2047, 2048, 2049, 5049):
        t += near(int(rng.integers(5, 590)), end - at, q, top=3000.0)
        q, at = q + 1, end
    assert len(t) == 5049 and 2049 < 2 * SCAN_TILE < 5049
    out["wavefront and scan tile edges"] = (w, make_rows(t))
    out["one query of 10 000 records"] = (w, make_rows([(9, int(s), 20000.0 - i) for i, s in enumerate(rng.integers(200, 260, 10000))]))
    out["subjects with no taxon, one taxon, three taxa"] = (w, make_rows([(1, N["none"], 80.0), (1, N["plain"], 70.0), (1, N["three"], 60.0),
                                                                         (2, N["none"], 50.0), (3, N["three"], 40.0)]))
    out["starter: first taxon unassigned, a later one assigned"] = (w, make_rows([(1, N["unassigned_first"], 90.0), (1, N["plain"], 80.0)]))
    out["starter is the third record"] = (w, make_rows([(1, N["none"], 90.0), (1, N["disconnected"], 85.0), (1, N["plain"], 80.0), (1, N["near"], 70.0)]))
    out["no starter at all"] = (w, make_rows([(1, N["none"], 90.0), (1, N["disconnected"], 85.0), (1, N["unassigned_first"], 80.0)]))
    out["the root itself as a taxon"] = (w, make_rows([(1, N["root"], 90.0), (1, N["plain"], 80.0), (2, N["root"], 70.0), (3, N["plain"], 60.0), (3, N["root"], 50.0)]))
    out["deep against shallow, both orders"] = (w, make_rows([(1, N["deep"], 90.0), (1, N["shallow"], 50.0), (2, N["shallow"], 90.0), (2, N["deep"], 50.0)]))
    # the top-percent rule: a record exactly at best * f (kept) and one just below it (dropped), for P = 50 and P = 10; two records
    # with the same best score and a far weak one
    t = []
    for q, P in ((1, 50.0), (2, 10.0)):
        best = 137.0
        at = best * (1.0 - P / 100.0)
        t += [(q, N["plain"], best), (q, N["near"], at), (q, N["far"], float(np.nextafter(at, 0.0)))]
    t += [(3, N["plain"], 77.5), (3, N["near"], 77.5), (3, N["far"], 20.0)]
    t += [(4, N["far"], 10.0), (4, N["plain"], 99.0), (4, N["near"], 98.0)]  # (the best is not the first record)
    out["top percent: at the cut, just below it, two best records"] = (w, make_rows(t))
    # the small tree of tests/test_taxonomy.py
    out["the taxdump tree"] = (sw, make_rows([(0, 0, 90.0), (0, 1, 80.0), (1, 2, 90.0), (1, 3, 50.0), (1, 4, 45.0), (2, 6, 70.0), (3, 0, 60.0), (3, 2, 30.0),
                                              (4, 7, 60.0), (4, 9, 55.0), (5, 8, 50.0), (5, 5, 49.0), (6, 5, 10.0)]))
    return out


def random_list(n_rows=20000, seed=21):
    """(world, rows): queries of 1 .. 25 records; a query's subjects are neighbours of one subject -- the closer, the better the bit
    score -- and about one in 25 of its records lies anywhere, with weak scores"""
    w = random_world()
    rng = np.random.default_rng(seed)
    t, q = [], 0
    while len(t) < n_rows:
        k = min(int(rng.integers(1, 26)), n_rows - len(t))
        base = int(rng.integers(0, 600))
        for i in range(k):
            if rng.random() < 0.04:
                t.append((q, int(rng.integers(0, 600)), float(rng.integers(30, 80))))
            else:
                o = int(rng.integers(-6, 7))
                t.append((q, min(599, max(0, base + o)), 300.0 - 12.0 * abs(o) - float(rng.integers(0, 5))))
        q += 1
    return w, make_rows(t)


def mixed_component_list():
    """a query whose taxa have no common ancestor: one below the root, one below the second root"""
    w = random_world()
    return w, make_rows([(1, w.named["plain"], 90.0), (2, w.named["plain"], 80.0), (2, w.named["other"], 70.0), (3, w.named["near"], 60.0)])
