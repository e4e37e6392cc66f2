"""_writeRecord's sort / unique / sort / cut (src/search_algo.hpp:820-882) behind a Level-2 call: on the host after everything came
down, or on the device before anything comes down.  Per result list, wall clock of

    (a) lx_iterate_matches_dev + lx_postprocess_records (in place, on the rows of the result)   -- the path without the device step
    (b) lx_iterate_matches_dev_top

with every run listed (--warmup untimed calls, then --runs timed ones of each, alternating), the medians, the spread of (a)'s runs
(max - min), the host function's time alone (its share of (a)), the device time of the step's kernels alone (lx_last_phase_ms phase 7),
and the bytes of rows + alignment columns that came down.  The lists: the protein list of bench.py --iterate --config 1 (configs[1]),
the read list of configs[2] (bench.py --iterate), and an ABUNDANT protein list (lambda_amd/synth.py: families of --abundant-family
members, so that every query has a few hundred surviving windows) -- all cut to --max-matches records per query.

With --max-hsps K and / or --culling-limit L (lx_cull_options; 0 = off, the default) the step has the two rules between its unique
and its cut: (a) ends in lx_postprocess_records_ex, (b) is lx_iterate_matches_dev_top_ex, and a further line names what each rule
dropped.  --lists picks the lists (1, 2, abundant).  With both options off the tool calls what it always called, so that an older
library (LX_LIB_PATH) can be timed with it.

    python tools/records_bench.py > profiles/records_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi, synth, workloads  # noqa: E402


def lists(a):
    w1, w2 = workloads.WORKLOADS[1], workloads.WORKLOADS[2]
    yield "configs[1] protein list", w1, lambda: synth.make_protein_seed_list_np(a.queries, seed=w1.seed, lq=w1.lq, homologs=w1.windows // 2, spurious=w1.windows // 2), 1
    yield "configs[2] read list", w2, lambda: synth.make_seed_list_np(a.reads, a.mbp, seed=0x1A3BDA03), 2
    yield (f"abundant protein list ({a.abundant_family} homologs per query)", w1,
           lambda: synth.make_protein_seed_list_np(a.abundant_queries, seed=w1.seed + 7, lq=w1.lq, homologs=a.abundant_family, spurious=0), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--mbp", type=float, default=100.0)
    ap.add_argument("--abundant-queries", type=int, default=3000)
    ap.add_argument("--abundant-family", type=int, default=300)
    ap.add_argument("--max-matches", type=int, default=25)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-hsps", type=int, default=0)
    ap.add_argument("--culling-limit", type=int, default=0)
    ap.add_argument("--lists", default="1,2,abundant", help="comma-separated: 1 (configs[1]), 2 (configs[2]), abundant")
    a = ap.parse_args()
    import torch

    lib = capi.load()
    cull = a.max_hsps > 0 or a.culling_limit > 0
    wanted = {"1": "configs[1]", "2": "configs[2]", "abundant": "abundant"}
    picked = [wanted[x] for x in a.lists.split(",") if x]
    print(f"# records_bench: max_matches {a.max_matches}, {a.warmup} warm-ups + {a.runs} runs of each path per list; times in ms"
          + (f"; max_hsps {a.max_hsps}, culling_limit {a.culling_limit}" if cull else "") + f"; library build {lib.lx_build_id().decode()}" + (" (LX_LIB_PATH)" if os.environ.get("LX_LIB_PATH") else ""))
    for name, w, make, frames in lists(a):
        if not any(name.startswith(x) for x in picked):
            continue
        q, qoff, qlen, qorig, s, soff, slen, m = make()
        d = w.directions[0]
        m_, ma, mi, go, ge = d.scoring
        with capi.Handle(0) as h:
            h.set_scoring(capi.builtin_scoring(m_, match=ma, mismatch=mi, gap_open=go, gap_extend=ge), 0)
            h.set_option(capi.LX_OPT_TRACE_BYTES, 160 << 30)
            ka = capi.karlin_params(*w.karlin)
            if frames == 1:
                params = capi.SearchParams(w.max_evalue, -1, 0, w.db_length, 0, 1, 1, 0, capi.LX_FRAMES_NONE, capi.LX_FRAMES_NONE, ka)
            else:
                params = capi.SearchParams(w.max_evalue, -1, 0, int(slen.sum()), 0, 2, 1, 0, capi.LX_FRAMES_REVCOMP, capi.LX_FRAMES_NONE, ka)
            h.set_subjects(s)
            h.set_subject_seqs(soff, slen)
            h.set_queries(q, qoff, qlen, qorig, frames)
            d_m = torch.from_numpy(m.view(np.uint8).copy()).to("cuda:0")
            torch.cuda.synchronize()
            # (the untranslated lengths: what lx_set_queries keeps resident for the Level-2 form)
            copt, _lens = capi.cull_options(a.max_hsps, a.culling_limit, qorig) if cull else (None, None)

            def size_of(r):
                n = int(lib.lx_iterate_result_count(r))
                if n == 0:
                    return 0, 0
                rows = np.frombuffer((C.c_char * (n * 128)).from_address(lib.lx_iterate_result_matches(r)), dtype=capi.BLAST_MATCH_DTYPE)
                return n, int((rows["ops_off"] + rows["n_ops"].astype(np.uint64)).max()) if lib.lx_iterate_result_ops(r) else 0

            def path_a():
                r, st = C.c_void_p(), capi.RecordStats()
                t0 = time.perf_counter()
                h._check(lib.lx_iterate_matches_dev(h.h, 0, d_m.data_ptr(), len(m), C.byref(params), C.byref(r)))
                t1 = time.perf_counter()
                n, cols = size_of(r)  # (not timed)
                t2 = time.perf_counter()
                cst = capi.CullStats()
                if cull:
                    kept = lib.lx_postprocess_records_ex(lib.lx_iterate_result_matches(r), n, a.max_matches, C.byref(copt), C.byref(st), C.byref(cst))
                    assert kept >= 0, capi.last_output_error()
                else:
                    kept = lib.lx_postprocess_records(lib.lx_iterate_result_matches(r), n, a.max_matches, C.byref(st))
                t3 = time.perf_counter()
                lib.lx_iterate_result_free(r)
                return (t1 - t0 + t3 - t2) * 1e3, (t3 - t2) * 1e3, n, cols, int(kept), st, cst

            def path_b():
                r, st = C.c_void_p(), capi.RecordStats()
                t0 = time.perf_counter()
                cst = capi.CullStats()
                if cull:
                    h._check(lib.lx_iterate_matches_dev_top_ex(h.h, 0, d_m.data_ptr(), len(m), C.byref(params), a.max_matches, C.byref(copt), C.byref(st),
                                                               C.byref(cst), C.byref(r)))
                else:
                    h._check(lib.lx_iterate_matches_dev_top(h.h, 0, d_m.data_ptr(), len(m), C.byref(params), a.max_matches, C.byref(st), C.byref(r)))
                t1 = time.perf_counter()
                kernel_ms, launches = h.last_phase_ms(7)
                n, cols = size_of(r)
                lib.lx_iterate_result_free(r)
                return (t1 - t0) * 1e3, kernel_ms, n, cols, launches, st, cst

            for _ in range(a.warmup):
                path_a(), path_b()
            ra, rb = [], []
            for _ in range(a.runs):
                ra.append(path_a())
                rb.append(path_b())
            ta, tb = [x[0] for x in ra], [x[0] for x in rb]
            n_a, cols_a, kept_a, st_a = ra[0][2:6]
            n_b, cols_b, _, st_b = rb[0][2:6]
            same = kept_a == n_b and all(getattr(st_a, f) == getattr(st_b, f) for f, _ in capi.RecordStats._fields_) and bytes(ra[0][6]) == bytes(rb[0][6])
            med_a, med_b, spread = statistics.median(ta), statistics.median(tb), max(ta) - min(ta)
            print(f"\n## {name}: {len(m)} matches -> {n_a} records ({n_a / max(st_a.qrys_with_hit, 1):.1f} per query with hits) -> {kept_a} kept "
                  f"(duplicates {st_a.hits_duplicate2}, abundant {st_a.hits_abundant}); (b) gives the same count and statistics: {same}")
            print("(a) lx_iterate_matches_dev + lx_postprocess_records: " + " ".join(f"{t:.2f}" for t in ta) + f" | median {med_a:.2f}, max - min {spread:.2f}")
            print("    of which lx_postprocess_records alone:            " + " ".join(f"{x[1]:.2f}" for x in ra) + f" | median {statistics.median(x[1] for x in ra):.2f}")
            print("(b) lx_iterate_matches_dev_top:                       " + " ".join(f"{t:.2f}" for t in tb) + f" | median {med_b:.2f}, max - min {max(tb) - min(tb):.2f}")
            print("    of which the step's kernels (device time):        " + " ".join(f"{x[1]:.2f}" for x in rb) + f" | median {statistics.median(x[1] for x in rb):.2f} ({rb[0][4]} range(s))")
            if cull:
                print(f"max_hsps {a.max_hsps} dropped {ra[0][6].hits_max_hsps}, culling_limit {a.culling_limit} dropped {ra[0][6].hits_culled} (host step); "
                      f"(b): {rb[0][6].hits_max_hsps}, {rb[0][6].hits_culled}")
            print(f"bytes down: (a) {n_a * 128 + cols_a} ({n_a} rows + {cols_a} columns), (b) {n_b * 128 + cols_b} ({n_b} rows + {cols_b} columns)")
            verdict = "gpu" if med_a - med_b > spread else "host"
            print(f"(a) - (b) = {med_a - med_b:.2f} ms against (a)'s spread of {spread:.2f} ms -> --records auto = {verdict} for lists of this kind")
            del d_m


if __name__ == "__main__":
    main()
