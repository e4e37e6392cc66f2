"""The per-query LCA on the host (lx_compute_lca_ex; at top percent 100 that is lx_compute_lca) against the device
(lx_compute_lca_dev, uploads and downloads included), over a seeded synthetic tree of NCBI size and lists of 25 records per query.

The tree: --taxa taxa (default 2.5 M) on 40 levels below the root's children, level sizes growing by a third per level up to
level 24 and level from there on; the taxa of a level are consecutive ids and the k-th of them hangs below the taxon at the same
relative place one level up, so that a clade is a run of ids on every level.  The heights are counted from the parents as
lx_taxonomy_build counts them (step 4), and lx_check_tax_tree must admit the result.  --subjects subjects (default 1 M) carry one
taxon (95 %), none (2 %) or two (3 %) from level 8 downwards and are ordered by their taxon's place in its level: neighbouring
subjects lie in neighbouring clades.  A query's 25 subjects are drawn within +-200 of one subject, one in 25 from anywhere; its bit
scores descend.

Both sides are timed as the bare library call on arrays made beforehand: one warm-up call each, then --runs runs each, alternating in
the same process, at top percent 100 and 10.  Printed: every run, the medians, the host's max - min, the kernels' device time
(lx_last_phase_ms phase 13) and the bytes that go up and come down.  `auto` takes the device only if its median lies below the
host's by more than the host's max - min at every size.

    python tools/lca_bench.py --queries 100000 1000000 > profiles/lca_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi  # noqa: E402

LEVELS = 40
PER_QUERY = 25


def synthetic_tree(n_taxa: int, n_subjects: int, seed: int):
    rng = np.random.default_rng(seed)
    w = np.array([1.33 ** min(l, 24) for l in range(LEVELS + 1)])
    sizes = np.maximum(1, (w / w.sum() * (n_taxa - 2)).astype(np.int64))
    start = 2 + np.concatenate([[0], np.cumsum(sizes)])
    n = int(start[-1])
    par = np.zeros(n, np.uint32)
    par[1] = 1
    place = np.zeros(n, np.float64)  # a taxon's relative place in its level
    par[start[0]:start[1]] = 1
    place[start[0]:start[1]] = (np.arange(sizes[0]) + 0.5) / sizes[0]
    for l in range(1, LEVELS + 1):
        k = np.arange(sizes[l])
        jitter = rng.integers(-1, 2, sizes[l])
        up = np.clip(k * sizes[l - 1] // sizes[l] + jitter, 0, sizes[l - 1] - 1)
        par[start[l]:start[l + 1]] = start[l - 1] + up
        place[start[l]:start[l + 1]] = (k + 0.5) / sizes[l]
    # lx_taxonomy_build's step 4: the heights counted from the final parents
    hgt = np.zeros(n, np.uint32)
    cur = par.copy()
    while True:
        climbing = cur > 1
        if not climbing.any():
            break
        hgt += climbing
        cur = par[cur]
    assert int(hgt.max()) == LEVELS
    taxon = rng.integers(start[8], n, n_subjects)
    taxon = taxon[np.argsort(place[taxon], kind="stable")]
    r = rng.random(n_subjects)
    count = np.where(r < 0.02, 0, np.where(r < 0.05, 2, 1))
    off = np.concatenate([[0], np.cumsum(count)]).astype(np.uint64)
    ids = np.zeros(int(off[-1]), np.uint32)
    first = off[:-1][count > 0].astype(np.int64)
    ids[first] = taxon[count > 0]
    second = off[:-1][count == 2].astype(np.int64) + 1
    ids[second] = np.clip(taxon[count == 2] + rng.integers(-50, 51, int((count == 2).sum())), start[8], n - 1)
    return par, hgt, off, ids


def synthetic_list(n_queries: int, n_subjects: int, seed: int):
    rng = np.random.default_rng(seed)
    n = n_queries * PER_QUERY
    base = np.repeat(rng.integers(0, n_subjects, n_queries), PER_QUERY)
    sid = np.clip(base + rng.integers(-200, 201, n), 0, n_subjects - 1)
    far = rng.random(n) < 0.04
    sid[far] = rng.integers(0, n_subjects, int(far.sum()))
    bits = np.sort(rng.uniform(40.0, 400.0, (n_queries, PER_QUERY)), axis=1)[:, ::-1].reshape(-1)
    m = np.zeros(n, capi.BLAST_MATCH_DTYPE)
    m["n_qid"] = np.repeat(np.arange(n_queries), PER_QUERY)
    m["n_sid"] = sid
    m["bit_score"] = bits
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--taxa", type=int, default=2_500_000)
    ap.add_argument("--subjects", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    lib = capi.load()
    t0 = time.perf_counter()
    par, hgt, off, ids = synthetic_tree(a.taxa, a.subjects, a.seed)
    capi.check_tax_tree(par, hgt, off, ids)
    tree, keep = capi._tax_tree(par, hgt, off, ids)
    print(f"tree: {len(par)} taxa, {(par > 0).sum()} with a parent, largest height {int(hgt.max())}, {a.subjects} subjects with {len(ids)} taxon ids "
          f"({(par.nbytes + hgt.nbytes) / 1e6:.1f} MB of parents and heights; made in {time.perf_counter() - t0:.1f} s)", flush=True)
    wins, same_all = [], True
    with capi.Handle(0) as h, capi.TaxDev(h, par, hgt, off, ids) as tax:
        for nq in a.queries:
            m = synthetic_list(nq, a.subjects, a.seed + nq)
            n = len(m)
            out = {side: (np.zeros(n, np.uint64), np.zeros(n, np.uint32), C.c_uint64()) for side in "ab"}

            def host(opt):
                q, l, c = out["a"]
                return lib.lx_compute_lca_ex(capi._ptr(m), n, C.byref(tree), C.byref(opt), capi._ptr(q), capi._ptr(l), C.byref(c))

            def device(opt):
                q, l, c = out["b"]
                return lib.lx_compute_lca_dev(h.h, tax.t, capi._ptr(m), n, C.byref(opt), capi._ptr(q), capi._ptr(l), C.byref(c))

            for top in (100.0, 10.0):
                opt = capi.lca_options(top)
                times = {"a": [], "b": []}
                kernel = []
                for run in range(-1, a.runs):  # (run -1: the warm-up call of either side)
                    for side, f in (("a", host), ("b", device)):
                        t1 = time.perf_counter()
                        rc = f(opt)
                        dt = (time.perf_counter() - t1) * 1e3
                        if rc != capi.LX_OK:
                            raise SystemExit(f"side ({side}) failed: {rc}")
                        if run >= 0:
                            times[side].append(dt)
                            if side == "b":
                                kernel.append(h.last_phase_ms(13)[0])
                            print(f"queries {nq} top {top:g} run {run} ({side}) {'host  ' if side == 'a' else 'device'} {dt:9.2f} ms"
                                  + (f"  kernels {kernel[-1]:7.2f} ms" if side == "b" else ""), flush=True)
                (qa, la, ca), (qb, lb, cb) = out["a"], out["b"]
                same = ca.value == cb.value == nq and np.array_equal(qa[:nq], qb[:nq]) and np.array_equal(la[:nq], lb[:nq])
                same_all = same_all and same
                med = {s: statistics.median(times[s]) for s in "ab"}
                spread = max(times["a"]) - min(times["a"])
                up = n * (12 if top == 100.0 else 20)
                down = nq * 4 + 4 * h.last_phase_ms(13)[1]
                win = med["b"] < med["a"] - spread
                wins.append(win)
                print(f"queries {nq} rows {n} top {top:g}: host median {med['a']:.2f} ms (max - min {spread:.2f}), device median {med['b']:.2f} ms "
                      f"(kernels median {statistics.median(kernel):.2f} ms, {up} bytes up, {down} bytes down), host / device {med['a'] / med['b']:.2f}, "
                      f"same pairs: {same}, LCA below the root: {np.mean(la[:nq] > 1):.2f}, device wins by the rule: {win}", flush=True)
            del m, out
    print(f"auto = {'gpu' if all(wins) else 'host'} by the rule (the device's median below the host's by more than the host's max - min, every size and top percent)")
    return 0 if same_all else 1


if __name__ == "__main__":
    sys.exit(main())
