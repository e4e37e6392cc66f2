"""_writeRecord's sort / unique / sort / cut as kernels (lx_toprec.hip) against the Python restatement of src/search_algo.hpp:820-882
(tests/toprec_reference.py), with the host form lx_postprocess_records as a second witness: the same rows in the same order (the
128 bytes of every row) and the same five counters -- for lx_postprocess_records_dev on crafted rows, and for
lx_iterate_matches_dev_top against lx_iterate_matches_dev followed by the restatement."""
import ctypes as C

import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import toprec_reference as ref
from tests.test_gpu_level2 import _seed_list, _to_device
from tests.test_oracle import SCHEMES

pytestmark = pytest.mark.gpu


def _check(handle, m, max_matches):
    want, wst = ref.write_record(m, max_matches)
    host, hst = capi.postprocess_records(m, max_matches)
    assert ref.stats_dict(hst) == wst and np.array_equal(host, want)  # (the two witnesses agree)
    got, gst = capi.postprocess_records_dev(handle, m, max_matches)
    assert ref.stats_dict(gst) == wst, (ref.stats_dict(gst), wst)
    assert len(got) == len(want)
    assert np.array_equal(got, want) and got.tobytes() == want.tobytes()
    return wst


@pytest.mark.parametrize("max_matches", [0, 1, 25, 2 ** 40])
def test_segments_on_every_edge_of_the_layout(handle, max_matches):
    """Segments of 1 .. 3 000 rows in one list: below, at and above a wavefront, a workgroup's rows and the staged tile (beyond which
    the large-segment path takes further turns), 30 % duplicated keys, ties in the bit score."""
    m = ref.crafted_rows(np.random.default_rng(1), ref.EDGE_SEGMENTS)
    st = _check(handle, m, max_matches)
    assert st["hits_duplicate2"] > 1000


@pytest.mark.parametrize("sizes", [[512], [513], [511, 1], [256, 256], [255, 257], [1, 512, 1], [768, 256], [1024], [1025]])
def test_spans_at_the_tile_edge(handle, sizes):
    """Lists that begin at a workgroup's first row, so that a workgroup's span is exactly the staged tile, one row more, one less."""
    m = ref.crafted_rows(np.random.default_rng(len(sizes) + sizes[0]), sizes, n_sid=7)
    for mm in (3, 2 ** 40):
        _check(handle, m, mm)


def test_empty_and_single_row_lists(handle):
    m = ref.crafted_rows(np.random.default_rng(2), [1])
    for mm in (0, 1, 25):
        got, st = capi.postprocess_records_dev(handle, m[:0], mm)
        assert len(got) == 0 and ref.stats_dict(st) == dict.fromkeys(ref.STAT_FIELDS, 0)
        _check(handle, m, mm)


def test_bad_arguments_with_a_live_handle(handle):
    m = np.zeros(4, dtype=capi.BLAST_MATCH_DTYPE)
    st, n = capi.RecordStats(), C.c_uint64(7)
    assert handle.lib.lx_postprocess_records_dev(handle.h, None, 4, 25, C.byref(st), C.byref(n)) == capi.LX_EINVAL
    assert handle.lib.lx_postprocess_records_dev(handle.h, capi._ptr(m), 4, 25, C.byref(st), None) == capi.LX_EINVAL
    assert handle.lib.lx_postprocess_records_dev(handle.h, None, 0, 25, None, C.byref(n)) == 0 and n.value == 0  # (no rows, no stats asked)


def test_exact_duplicates_keep_the_best_and_then_the_earliest(handle):
    rng = np.random.default_rng(3)
    m = ref.crafted_rows(rng, [6, 300], dup_share=0.0)
    for f in ("n_sid", "q_start", "q_end", "s_start", "s_end", "q_frame", "s_frame"):
        m[f][:6] = m[f][0]
        m[f][6:] = m[f][6 + (np.arange(300) % 11)]  # eleven keys, about 27 copies of each
    m["bit_score"][:6] = [30.5, 41.0, 41.0, 12.0, 41.0, 40.5]  # the best three times: the earliest of them (input row 1) survives
    m["bit_score"][6:] = rng.integers(0, 3, 300) + 50.0          # ties among the copies
    want, _ = ref.write_record(m, 25)
    assert want["qry_id"][0] == 1 and len(want) == 1 + 11
    st = _check(handle, m, 25)
    assert st["hits_duplicate2"] == 5 + 289 and st["pairs"] <= 12
    _check(handle, m, 2 ** 40)


def test_equal_bit_scores_keep_the_first_order(handle):
    m = ref.crafted_rows(np.random.default_rng(4), [700, 90, 5], dup_share=0.0, n_sid=1000)
    m["bit_score"] = 33.25
    want, _ = ref.write_record(m, 2 ** 40)
    k = want[:700]
    assert (np.diff(k["n_sid"].astype(np.int64)) >= 0).all()  # order 2 left order 1 as it was
    _check(handle, m, 2 ** 40)
    _check(handle, m, 25)


def test_fields_beyond_bit_32_and_signed_frames(handle):
    rng = np.random.default_rng(6)
    m = ref.crafted_rows(rng, [400, 64, 33], wide=True, n_sid=3)
    assert (m["n_sid"] >> np.uint64(32)).max() > 0 and (m["s_start"] >> np.uint64(32)).max() > 0
    _check(handle, m, 2 ** 40)
    # frames -3 .. +3 on both sides and nothing else that differs
    f = ref.crafted_rows(rng, [49, 49], dup_share=0.0)
    for name in ("n_sid", "q_start", "q_end", "s_start", "s_end"):
        f[name] = 5
    grid = np.array([(a, b) for a in range(-3, 4) for b in range(-3, 4)])[rng.permutation(49)]
    f["q_frame"], f["s_frame"] = np.tile(grid[:, 0], 2), np.tile(grid[:, 1], 2)
    f["bit_score"] = 20.0
    want, _ = ref.write_record(f, 2 ** 40)
    assert want["q_frame"][:8].tolist() == [-3] * 7 + [-2] and want["s_frame"][:7].tolist() == list(range(-3, 4))
    _check(handle, f, 2 ** 40)


def test_a_query_in_two_separated_runs_is_two_queries(handle):
    m = ref.crafted_rows(np.random.default_rng(7), [120, 30, 80, 1], qids=[4, 2, 4, 2])
    st = _check(handle, m, 25)
    assert st["qrys_with_hit"] == 4


def test_random_list_of_ragged_segments(handle):
    rng = np.random.default_rng(20240607)
    sizes = np.concatenate([rng.integers(1, 40, 6000), rng.integers(200, 700, 100), [2500, 1, 1300]])
    sizes = sizes[rng.permutation(len(sizes))]
    m = ref.crafted_rows(rng, sizes, dup_share=0.3, n_sid=60)
    assert 150_000 < len(m) < 250_000
    st = _check(handle, m, 25)
    assert st["hits_duplicate2"] > 0.2 * len(m) and st["hits_abundant"] > 10_000


# ---- lx_iterate_matches_dev_top ---------------------------------------------------------------------------------------------------

_IST = ("hits_duplicate", "failed_bitscore", "failed_evalue", "failed_identity", "num_ext_score", "num_ext_ali")


def _top_against_plain(handle, d_m, n, params_of, min_records, cuts=(1, 25)):
    """lx_iterate_matches_dev_top == lx_iterate_matches_dev + the restatement: rows (but ops_off), record statistics, the columns of
    every kept record, the call's own statistics -- with and without alignment columns, cut to 1 and to 25."""
    plain, pops, pst = handle.iterate_matches_dev(d_m, n, params_of(0))
    assert len(plain) >= min_records
    for mm in cuts:
        want, wst, at = ref.write_record(plain, mm, with_index=True)
        assert 0 < len(want) < len(plain)
        for flags in (0, capi.LX_ITERATE_NO_OPS):
            got, gops, gst, rst = handle.iterate_matches_dev_top(d_m, n, params_of(flags), mm)
            assert ref.stats_dict(rst) == wst, (mm, flags)
            assert len(got) == len(want)
            for f in got.dtype.names:
                if f != "ops_off":
                    assert np.array_equal(got[f], want[f]), (f, mm, flags)
            for f in _IST:
                assert getattr(gst, f) == getattr(pst, f), f
            if flags:
                assert gops == [] and (got["ops_off"] == 0).all()
            else:
                assert gops == [pops[i] for i in at]
                # the kept records' columns stand behind one another, in output order
                assert np.array_equal(got["ops_off"], np.concatenate([[0], np.cumsum(got["n_ops"].astype(np.uint64))[:-1]]).astype(np.uint64))
    return plain


@pytest.mark.parametrize("scheme", ["blosum62", "nucl"])
def test_iterate_top_on_protein_and_nucleotide_lists(handle, scheme):
    handle.set_scoring(SCHEMES[scheme], 0)
    rng = np.random.default_rng(88)
    dna = scheme == "nucl"
    # no e-value filter: every window becomes a record; few subjects: a query has several records of one subject, and more than 25
    q, qoff, qlen, s, soff, slen, m = _seed_list(rng, 1200, 40, 90, lq_range=(140, 160) if dna else (50, 300), alphabet=np.arange(4, dtype=np.uint8) if dna else None)
    ka = capi.karlin_params(0, 2, -3, -5, -2) if dna else capi.karlin_params(62)
    params_of = lambda flags: capi.SearchParams(-1.0, -1, 0, int(slen.sum()) * 50, 0, 1, 1, 0, capi.LX_FRAMES_NONE, capi.LX_FRAMES_NONE, ka, 0, flags)
    handle.set_subjects(s)
    handle.set_subject_seqs(soff, slen)
    handle.set_queries(q, qoff, qlen, qlen, 1)
    m = m[rng.permutation(len(m))]
    plain = _top_against_plain(handle, _to_device(m), len(m), params_of, 20000)
    assert np.bincount(plain["n_qid"].astype(np.int64)).max() > 25


def test_iterate_top_on_a_bisulfite_list(handle):
    handle.set_scoring(SCHEMES["bs_fwd"], 0)
    handle.set_scoring(SCHEMES["bs_rev"], 1)
    rng = np.random.default_rng(32)
    q, qoff, qlen, s, soff, slen, m = _seed_list(rng, 300 * 4, 6 * 2, 40, lq_range=(100, 150), alphabet=np.arange(4, dtype=np.uint8))
    ka = capi.karlin_params(0, 2, -3, -5, -2)
    qorig = qlen[::4].copy()
    params_of = lambda flags: capi.SearchParams(-1.0, -1, 0, int(slen.sum()) * 100, 0, 4, 2, 1, capi.LX_FRAMES_BISULFITE, capi.LX_FRAMES_BISULFITE, ka, 0, flags)
    handle.set_subjects(s)
    handle.set_subject_seqs(soff, slen)
    handle.set_queries(q, qoff, qlen, qorig, 4)
    m = m[rng.permutation(len(m))]
    plain = _top_against_plain(handle, _to_device(m), len(m), params_of, 1000)
    assert set(np.unique(plain["subj_id"] % 2)) == {0, 1}  # a query has records of both strand directions


def test_iterate_top_on_a_protein_list_planned_in_more_than_one_range(handle):
    """300 000 windows and more are served in two ranges of the list: each range's records are cut behind its own kernels."""
    handle.set_scoring(SCHEMES["blosum62"], 0)
    rng = np.random.default_rng(89)
    nq, ns, hits, L = 8000, 400, 50, 10
    qlen, slen = rng.integers(50, 120, nq).astype(np.uint64), rng.integers(600, 2500, ns).astype(np.uint64)
    qoff, soff = (np.concatenate([[0], np.cumsum(x)[:-1]]).astype(np.uint64) for x in (qlen, slen))
    q, s = (synth.STD20[rng.integers(0, 20, int(x.sum()))].astype(np.uint8) for x in (qlen, slen))
    m = np.zeros(nq * hits, dtype=capi.MATCH_DTYPE)
    m["qryId"], m["subjId"] = np.repeat(np.arange(nq), hits), rng.integers(0, ns, nq * hits)
    m["qryStart"] = (rng.random(len(m)) * (qlen[m["qryId"]] - L)).astype(np.uint64)
    m["subjStart"] = (rng.random(len(m)) * (slen[m["subjId"]] - L)).astype(np.uint64)
    m["qryEnd"], m["subjEnd"] = m["qryStart"] + L, m["subjStart"] + L
    params_of = lambda flags: capi.SearchParams(-1.0, -1, 0, int(slen.sum()) * 50, 0, 1, 1, 0, capi.LX_FRAMES_NONE, capi.LX_FRAMES_NONE, capi.karlin_params(62), 0, flags)
    handle.set_subjects(s)
    handle.set_subject_seqs(soff, slen)
    handle.set_queries(q, qoff, qlen, qlen, 1)
    d_m = _to_device(m[rng.permutation(len(m))])
    assert len(handle.widen_and_preprocess_dev(d_m, len(m))) >= 300_000
    _top_against_plain(handle, d_m, len(m), params_of, 300_000, cuts=(25,))
