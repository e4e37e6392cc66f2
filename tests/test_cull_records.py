"""CPU tests of --max-hsps / --culling-limit: the host form lx_postprocess_records_ex against the independent model of
tests/cull_reference.py (a walk that keeps lists of survivors, where the library counts better rows), hand cases of the rule, the
refusals of lx_cull_options with their texts, the device entry points without a handle, and the front end's options."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from lambda_amd import capi
from tests import cull_reference as cref
from tests import toprec_reference as ref
from tests.test_cli import _cli, _fasta, _small_dbs

KS, LS, CUTS = (0, 1, 2, 5), (0, 1, 2, 3), (0, 1, 5, 25)


@pytest.fixture(scope="module", params=list(cref.MODES))
def random_list(request):
    """Several hundred queries of 1 .. 60 rows, one list per frame mode (made once, shared by the combinations below)."""
    mode = request.param
    rng = np.random.default_rng(1000 + list(cref.MODES).index(mode))
    sizes = rng.integers(1, 61, 300)
    m, q_lens, translated = cref.nested_rows(rng, sizes, mode)
    # duplicates of the seven-field key as well, so that the rules start from what the unique step left
    for i in np.flatnonzero(rng.random(len(m)) < 0.1):
        j = int(rng.integers(np.searchsorted(m["n_qid"], m["n_qid"][i]), i + 1))
        for f in ("n_sid", "q_start", "q_end", "s_start", "s_end", "q_frame", "s_frame"):
            m[f][i] = m[f][j]
    return mode, m, q_lens, translated


def test_host_form_equals_the_survivor_model(lx_lib, random_list):
    mode, m, q_lens, translated = random_list
    seen = dict.fromkeys(cref.CULL_FIELDS, 0)
    for K in KS:
        for L in LS:
            for mm in CUTS:
                want, wst = cref.write_record(m, mm, K, L, q_lens, translated)
                got, st, cst = capi.postprocess_records_ex(m, mm, K, L, q_lens, translated)
                assert cref.stats_dict(st, cst) == wst, (mode, K, L, mm)
                assert got.tobytes() == want.tobytes(), (mode, K, L, mm)
                assert (K > 0 or wst["hits_max_hsps"] == 0) and (L > 0 or wst["hits_culled"] == 0)
                for f in seen:
                    seen[f] += wst[f]
            if L == 3:  # a row culled at L = 3 has three better rows around it: nesting of depth >= 3 occurs
                assert cref.write_record(m, 25, K, 3, q_lens, translated)[1]["hits_culled"] > 0
    assert seen["hits_max_hsps"] > 1000 and seen["hits_culled"] > 1000
    # the lists hold what the rule distinguishes: equal intervals and partial overlaps inside a query, ties in the bit score
    iv = np.array([cref.printed_interval(int(r["q_start"]), int(r["q_end"]), int(r["q_frame"]), int(q_lens[r["n_qid"]]), translated) for r in m])
    same_q = m["n_qid"][1:] == m["n_qid"][:-1]
    a, b = iv[:-1][same_q], iv[1:][same_q]
    assert ((a == b).all(axis=1)).any()
    assert ((a[:, 0] < b[:, 0]) & (b[:, 0] <= a[:, 1]) & (a[:, 1] < b[:, 1])).any()
    assert (m["bit_score"][:-1][same_q] == m["bit_score"][1:][same_q]).any()
    if translated:
        assert (q_lens % 3 != 0).all() and set(np.unique(m["q_frame"])) == {-3, -2, -1, 1, 2, 3}


def test_options_off_equal_the_plain_step(lx_lib, random_list):
    _, m, q_lens, translated = random_list
    for mm in CUTS:
        plain, pst = capi.postprocess_records(m, mm)
        got, st, cst = capi.postprocess_records_ex(m, mm, 0, 0, q_lens, translated)
        assert got.tobytes() == plain.tobytes() and ref.stats_dict(st) == ref.stats_dict(pst) and (cst.hits_max_hsps, cst.hits_culled) == (0, 0)
        # opt == NULL
        buf, st2, cst2 = m.copy(), capi.RecordStats(), capi.CullStats()
        n = lx_lib.lx_postprocess_records_ex(capi._ptr(buf), len(buf), mm, None, C.byref(st2), C.byref(cst2))
        assert n == len(plain) and buf[:n].tobytes() == plain.tobytes() and ref.stats_dict(st2) == ref.stats_dict(pst)
        # no stats asked
        buf = m.copy()
        assert lx_lib.lx_postprocess_records_ex(capi._ptr(buf), len(buf), mm, None, None, None) == len(plain)


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------

def _rows(*rows):
    """rows of one query: (n_sid, q_start, q_end, q_frame, bit_score); qry_id = the row's input position"""
    m = np.zeros(len(rows), dtype=capi.BLAST_MATCH_DTYPE)
    for k, (sid, a, e, f, bs) in enumerate(rows):
        m[k]["n_sid"], m[k]["q_start"], m[k]["q_end"], m[k]["q_frame"], m[k]["bit_score"], m[k]["qry_id"] = sid, a, e, f, bs, k
    m["s_end"] = 10
    return m


def _kept(m, K=0, L=0, q_len=1000, translated=False, mm=25):
    got, st, cst = capi.postprocess_records_ex(m, mm, K, L, [q_len], translated)
    want, wst = cref.write_record(m, mm, K, L, [q_len], translated)
    assert got.tobytes() == want.tobytes() and cref.stats_dict(st, cst) == wst
    return got["qry_id"].tolist(), cst


def test_a_partial_overlap_is_never_culled(lx_lib):
    m = _rows((1, 0, 50, 0, 50.0), (2, 39, 90, 0, 40.0), (3, 0, 50, 0, 30.0))
    assert _kept(m[:2], L=1)[0] == [0, 1]
    kept, cst = _kept(m, L=1)
    assert kept == [0, 1] and cst.hits_culled == 1  # (the third has the first's interval)


def test_an_equal_interval_is_culled_by_score_then_by_place(lx_lib):
    kept, cst = _kept(_rows((1, 10, 60, 0, 30.0), (2, 10, 60, 0, 45.5)), L=1)
    assert kept == [1] and cst.hits_culled == 1
    # equal scores: the place in order 1 decides -- subject 5 stands before subject 9 there, whatever the input order
    kept, _ = _kept(_rows((9, 10, 60, 0, 30.0), (5, 10, 60, 0, 30.0)), L=1)
    assert kept == [1]
    assert _kept(_rows((9, 10, 60, 0, 30.0), (5, 10, 60, 0, 30.0)), L=2)[0] == [1, 0]


def test_both_strands_over_the_same_nucleotides_envelop_each_other(lx_lib):
    # BLASTN, a query of 100: [10, 40) on the plus strand prints 11 .. 40; [60, 90) of the reverse complement prints 40 .. 11
    for plus_score, minus_score, survivor in ((50.0, 40.0, 0), (40.0, 50.0, 1)):
        kept, _ = _kept(_rows((1, 10, 40, 1, plus_score), (2, 60, 90, -1, minus_score)), L=1, q_len=100)
        assert kept == [survivor]
    assert cref.printed_interval(10, 40, 1, 100, False) == cref.printed_interval(60, 90, -1, 100, False) == (11, 40)
    # BLASTX, 100 nucleotides: protein [3, 10) of frame +2 covers 11 .. 31; protein [23, 30) of frame -1 prints 31 .. 11
    assert cref.printed_interval(3, 10, 2, 100, True) == cref.printed_interval(23, 30, -1, 100, True) == (11, 31)
    for plus_score, minus_score, survivor in ((50.0, 40.0, 0), (40.0, 50.0, 1)):
        kept, _ = _kept(_rows((1, 3, 10, 2, plus_score), (2, 23, 30, -1, minus_score)), L=1, q_len=100, translated=True)
        assert kept == [survivor]
    # ... and one codon further it is a partial overlap
    assert _kept(_rows((1, 3, 10, 2, 50.0), (2, 24, 31, -1, 40.0)), L=1, q_len=100, translated=True)[0] == [0, 1]


def test_a_row_enveloped_only_by_a_row_that_max_hsps_dropped_stays(lx_lib):
    m = _rows((1, 200, 300, 0, 100.0), (1, 0, 80, 0, 90.0), (2, 10, 70, 0, 80.0))
    kept, cst = _kept(m, K=1, L=1)
    assert kept == [0, 2] and (cst.hits_max_hsps, cst.hits_culled) == (1, 0)
    kept, cst = _kept(m, K=0, L=1)
    assert kept == [0, 1] and (cst.hits_max_hsps, cst.hits_culled) == (0, 1)


def test_a_chain_of_three_at_limit_two(lx_lib):
    m = _rows((3, 20, 60, 0, 50.0), (1, 0, 100, 0, 70.0), (2, 10, 80, 0, 60.0))  # c, a, b
    kept, cst = _kept(m, L=2)
    assert kept == [1, 2] and cst.hits_culled == 1
    assert _kept(m, L=1)[0] == [1] and _kept(m, L=3)[0] == [1, 2, 0]


def test_max_hsps_counts_per_subject_and_frees_places_for_other_subjects(lx_lib):
    m = _rows(*[(1, 10 * k, 10 * k + 5, 0, 90.0 - k) for k in range(10)], (2, 500, 520, 0, 20.0))
    assert _kept(m, mm=5)[0] == [0, 1, 2, 3, 4]  # the cut counts HSPs: subject 2 never reaches the output
    kept, cst = _kept(m, K=2, mm=5)
    assert kept == [0, 1, 10] and cst.hits_max_hsps == 8


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def _ex(lx_lib, m, opt):
    buf, st, cst = m.copy(), capi.RecordStats(), capi.CullStats()
    n = lx_lib.lx_postprocess_records_ex(capi._ptr(buf), len(buf), 25, C.byref(opt), C.byref(st), C.byref(cst))
    assert n >= 0 or buf.tobytes() == m.tobytes()  # a refusal leaves the rows as they were
    return n, capi.last_output_error()


def test_refusals_of_the_options_come_with_a_text(lx_lib):
    m = _rows((1, 0, 50, 0, 50.0), (2, 10, 60, 0, 40.0))
    m["n_qid"] = 3
    opt, keep = capi.cull_options(0, 1, [100, 100, 100])
    n, text = _ex(lx_lib, m, opt)
    assert n == capi.LX_EINVAL and "names query 3" in text and "3 entries" in text
    opt, keep = capi.cull_options(0, 1, [100, 100, 100, 55])  # the second row ends at 60
    n, text = _ex(lx_lib, m, opt)
    assert n == capi.LX_EINVAL and "row 1 does not fit its query's length of 55" in text
    opt, keep = capi.cull_options(0, 1, [100, 100, 100, 150], q_translated=True)  # 3 * 60 > 150
    n, text = _ex(lx_lib, m, opt)
    assert n == capi.LX_EINVAL and "does not fit" in text
    opt, keep = capi.cull_options(0, 1, None)
    n, text = _ex(lx_lib, m, opt)
    assert n == capi.LX_EINVAL and "needs q_lens" in text
    # with culling_limit == 0 none of this is looked at
    opt, keep = capi.cull_options(1, 0, None)
    assert _ex(lx_lib, m, opt) == (2, "")
    opt, keep = capi.cull_options(0, 1, [100, 100, 100, 60])
    assert _ex(lx_lib, m, opt)[0] == 2
    del keep


def test_device_entry_points_without_a_handle(lx_lib):
    assert {"lx_cull_options_default", "lx_postprocess_records_ex", "lx_postprocess_records_dev_ex", "lx_iterate_matches_dev_top_ex"} <= set(capi.EXPORTED_SYMBOLS)
    m = np.zeros(4, dtype=capi.BLAST_MATCH_DTYPE)
    st, cst, n, res = capi.RecordStats(), capi.CullStats(), C.c_uint64(7), C.c_void_p()
    opt, _ = capi.cull_options(1, 0)
    assert (opt.max_hsps, opt.culling_limit, opt.q_lens, opt.n_q, opt.q_translated) == (1, 0, None, 0, 0)
    params = capi.SearchParams(1e-2, -1, 0, 1000, 0, 1, 1, 0, capi.LX_FRAMES_NONE, capi.LX_FRAMES_NONE, capi.karlin_params(62))
    assert lx_lib.lx_postprocess_records_dev_ex(None, capi._ptr(m), 4, 25, C.byref(opt), C.byref(st), C.byref(cst), C.byref(n)) == capi.LX_EINVAL
    assert lx_lib.lx_iterate_matches_dev_top_ex(None, 0, None, 0, C.byref(params), 25, C.byref(opt), C.byref(st), C.byref(cst), C.byref(res)) == capi.LX_EINVAL


# ---- the front end --------------------------------------------------------------------------------------------------------------------

def _search(tmp, *more, program="searchp", q="pq.fasta", d="db.fasta", out="o.m8"):
    return subprocess.run([str(_cli()), program, "-q", str(tmp / q), "-d", str(tmp / d), "-o", str(tmp / out), "--version-to-outputfile", "0", *more],
                          capture_output=True, text=True)


@pytest.mark.parametrize("option", ["--max-hsps", "--culling-limit"])
def test_cli_refuses_what_is_no_count(tmp_path, option):
    _fasta(tmp_path / "pq.fasta", ["q"], ["ACDEFGHIKLMNPQRSTVWY" * 3])
    _fasta(tmp_path / "db.fasta", ["s"], ["ACDEFGHIKLMNPQRSTVWY" * 5])
    for bad in ("-1", "1.5", "two", "", "+3"):
        r = _search(tmp_path, option, bad)
        assert r.returncode != 0 and f"{option} takes a number (0 = off, the default)" in r.stderr, (bad, r.stderr)
        assert not (tmp_path / "o.m8").exists()
    r = _search(tmp_path, option)
    assert r.returncode != 0 and f"missing value for {option}" in r.stderr
    r = subprocess.run([str(_cli()), "mkindexp", "-d", str(tmp_path / "db.fasta"), option, "1"], capture_output=True, text=True)
    assert r.returncode != 0 and f"unknown option {option}" in r.stderr


def test_cli_max_hsps_one_keeps_the_first_row_of_every_pair(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("the search needs a device")
    _small_dbs(tmp_path)
    # (-n large enough to hold everything, and the same in both runs: it is the seeding's budget as well)
    r = _search(tmp_path, "-n", "500", "--records", "host", out="all.m8")
    assert r.returncode == 0 and "lambda3 culling" not in r.stderr, r.stderr
    r = _search(tmp_path, "-n", "500", "--records", "host", "--max-hsps", "1", out="one.m8")
    assert r.returncode == 0, r.stderr
    assert "lambda3 culling: --max-hsps 1 dropped" in r.stderr and "--culling-limit 0 dropped 0 record(s), on the host" in r.stderr
    every = [l.split("\t") for l in (tmp_path / "all.m8").read_text().splitlines()]
    one = [l.split("\t") for l in (tmp_path / "one.m8").read_text().splitlines()]
    pairs = [(x[0], x[1]) for x in one]
    assert len(pairs) == len(set(pairs)) > 0
    first, seen = [], set()
    for x in every:
        if (x[0], x[1]) not in seen:
            seen.add((x[0], x[1]))
            first.append(x)
    assert one == first
