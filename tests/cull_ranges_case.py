"""Helper of tests/test_gpu_cull_records.py: lx_iterate_matches_dev_top_ex on a list of tests/level2_ranges_case.py (cut to 5 records
per query) against lx_iterate_matches_dev followed by the host step lx_postprocess_records_ex -- rows, alignment columns, both
statistics structs.  The test calls compare() on its own handle; run as a script (argv = list names) it does the same in a process
of its own, because the library reads LX_L2_RANGES, which forces the number of ranges, once per process.  "ok NAME" per list on stdout."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from lambda_amd import capi
from tests.level2_ranges_case import make_list, scheme

CUT = 5
OPTIONS = ((1, 0), (0, 1), (1, 1))  # (max_hsps, culling_limit)


def compare(h, name):
    """{(K, L): (hits_max_hsps, hits_culled)} after comparing everything."""
    import torch

    q, qoff, qlen, s, soff, slen, m = make_list(name)
    sc, ka = scheme(name)
    h.set_scoring(sc, 0)
    h.set_subjects(s)
    h.set_subject_seqs(soff, slen)
    h.set_queries(q, qoff, qlen, qlen, 1)
    d_m = torch.from_numpy(m.view(np.uint8).copy()).to("cuda:0")
    dropped = {}
    for flags in (0, capi.LX_ITERATE_NO_OPS):
        params = capi.SearchParams(1e-2, -1, 0, int(slen.sum()), 0, 1, 1, 0, capi.LX_FRAMES_NONE, capi.LX_FRAMES_NONE, ka, 0, flags)
        plain, pops, pst = h.iterate_matches_dev(d_m, len(m), params)
        where = {int(o): i for i, o in enumerate(plain["ops_off"])} if not flags else {}
        for K, L in OPTIONS:
            want, wst, wcst = capi.postprocess_records_ex(plain, CUT, K, L, qlen, False)
            got, gops, gst, rst, cst = h.iterate_matches_dev_top_ex(d_m, len(m), params, CUT, K, L)
            assert 0 < len(want) <= len(plain) and len(got) == len(want), (name, K, L, len(got), len(want))
            for f in got.dtype.names:
                if f != "ops_off":
                    assert np.array_equal(got[f], want[f]), (name, K, L, f)
            assert bytes(rst) == bytes(wst) and bytes(cst) == bytes(wcst), (name, K, L)
            assert bytes(gst) == bytes(pst)  # (what the extension did, not what the step removed)
            if flags:
                assert gops == [] and (got["ops_off"] == 0).all()
            else:
                assert gops == [pops[where[int(o)]] for o in want["ops_off"]], (name, K, L)
                assert np.array_equal(got["ops_off"], np.concatenate([[0], np.cumsum(got["n_ops"].astype(np.uint64))[:-1]]).astype(np.uint64))
            dropped[(K, L)] = (int(cst.hits_max_hsps), int(cst.hits_culled))
    return dropped


if __name__ == "__main__":
    with capi.Handle(0) as handle:
        for list_name in sys.argv[1:]:
            print(f"ok {list_name} {compare(handle, list_name)}", flush=True)
            print(f"list {list_name} done", file=sys.stderr, flush=True)
