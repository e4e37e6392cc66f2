"""The two chunk drivers of lx_extend_batch* (lx_xb_run.cpp: chunks of the ordered list for the one-query-per-wavefront kernels;
lx_xb_wf.cpp: chunks of the plan's wavefronts for the multi-query sweep) with the smallest chunks, and the three places their
results go (lx_xb_sinks.cpp): rows of column bytes, rows of run-length codes, the survivor list."""
import functools

import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import oracle_lib
from tests.test_gpu_list import FIELDS, codes_of
from tests.test_gpu_score import SCHEMES

pytestmark = pytest.mark.gpu

# both sides of every boundary between the geometry classes of the one-query-per-wavefront kernels (104 / 152 / 200 / 208 columns,
# then panels of 152), and one length of three panels
CLASS_EDGE_LENGTHS = (100, 104, 105, 152, 153, 200, 201, 208, 209, 320)


@functools.lru_cache(maxsize=None)
def class_edge_list():
    """About 3000 extensions: queries of the lengths above with 1 to 20 windows of 30 to 300 rows each (half of them hold a
    mutated copy of the query's start), every 17th extension dead, per-extension cut-offs, shuffled.  With chunks of 1024 several
    chunk ends fall on a class boundary and several inside a class, and both lanes are used more than once."""
    rng = np.random.default_rng(2024)
    alphabet = synth.STD20
    lqs, nwin = [], []
    while sum(nwin) < 3000:
        lqs.append(int(rng.choice(CLASS_EDGE_LENGTHS)))
        nwin.append(int(rng.integers(1, 21)))
    lqs, nwin = np.array(lqs), np.array(nwin)
    q_off = np.concatenate([[0], np.cumsum(lqs)[:-1]])
    q = alphabet[rng.integers(0, len(alphabet), int(lqs.sum()))].astype(np.uint8)
    qid = np.repeat(np.arange(len(lqs)), nwin)
    ls = rng.integers(30, 301, len(qid))
    s_off = np.concatenate([[0], np.cumsum(ls)[:-1]])
    s = alphabet[rng.integers(0, len(alphabet), int(ls.sum()))].astype(np.uint8)
    for e in np.nonzero(rng.random(len(qid)) < 0.5)[0]:
        n = int(min(lqs[qid[e]], ls[e]))
        at = int(rng.integers(0, ls[e] - n + 1))
        piece = q[q_off[qid[e]]: q_off[qid[e]] + n].copy()
        mut = rng.random(n) < 0.2
        piece[mut] = alphabet[rng.integers(0, len(alphabet), int(mut.sum()))]
        s[s_off[e] + at: s_off[e] + at + n] = piece
    ext = np.zeros(len(qid), dtype=capi.EXT_DTYPE)
    ext["q_off"], ext["q_len"], ext["s_off"], ext["s_len"] = q_off[qid], lqs[qid], s_off, ls
    ext = ext[rng.permutation(len(ext))].copy()
    ext["s_len"][::17] = 0
    mins = np.where(np.arange(len(ext)) % 4 == 0, 95, 55).astype(np.int32)
    return q, s, ext, mins


@functools.lru_cache(maxsize=None)
def ragged_list():
    """The shape of test_host_plan_on_ragged_lists' case 5: mixed query lengths, a few windows per query, several multi-query chunks."""
    q, s, ext = synth.make_ragged_lists_np(500, seed=105, lq_range=(40, 420), mean_windows=4)
    mins = np.where(np.arange(len(ext)) % 5 == 0, 95, 55).astype(np.int32)
    return q, s, ext, mins


def in_small_chunks(handle, sweep, call):
    """call() with chunks of 1024 and the multi-query sweep on or off; the options as the session's handle has them afterwards."""
    handle.set_option(capi.LX_OPT_PASS2_MODE, 2)
    handle.set_option(capi.LX_OPT_EXTEND_CHUNK, 1024)
    try:
        handle.set_option(capi.LX_OPT_MQ_SWEEP, sweep)  # (set before every call: it also forgets what the last call's chunks taught the pipeline)
        got = call()
        return got, handle.last_trace_kernel_name()
    finally:
        handle.set_option(capi.LX_OPT_MQ_SWEEP, 1)
        handle.set_option(capi.LX_OPT_EXTEND_CHUNK, 0)
        handle.set_option(capi.LX_OPT_PASS2_MODE, 1)


def test_run_driver_across_geometry_classes_with_the_smallest_chunks(handle, oracle):
    sc_p = SCHEMES["blosum62"]
    handle.set_scoring(sc_p, 0)
    osc = oracle_lib.scoring_from(sc_p)
    q, s, ext, mins = class_edge_list()
    assert 2900 < len(ext) < 3200
    (score, hsp, off, ops), name = in_small_chunks(handle, 0, lambda: handle.extend_batch(q, s, ext, mins))
    assert "sweep_mq" not in name
    want = oracle.score_batch(q, s, ext, osc, threads=8)
    assert (score == want).all()
    surv = np.nonzero((want >= mins) & (ext["s_len"] > 0))[0]
    assert len(surv) > 10
    dead = np.setdiff1d(np.arange(len(ext)), surv)
    assert (hsp["n_ops"][dead] == 0).all() and (hsp["score"][dead] == want[dead]).all()
    for i, (oh, oops) in zip(surv, oracle.align_batch(q, s, ext[surv], osc)):
        g = hsp[i]
        assert (g["score"], g["q_begin"], g["q_end"], g["s_begin"], g["s_end"], g["n_ops"]) == \
               (oh.score, oh.q_begin, oh.q_end, oh.s_begin, oh.s_end, oh.n_ops), (i, ext[i])
        st = int(off[i]) + int(g["ops_shift"])
        assert bytes(ops[st: st + oh.n_ops]) == oops, (i, ext[i])


@pytest.mark.parametrize("make,sweep", [(class_edge_list, 0), (ragged_list, 1)], ids=["run_driver", "wavefront_driver"])
def test_the_three_forms_agree(handle, make, sweep):
    handle.set_scoring(SCHEMES["blosum62"], 0)
    q, s, ext, mins = make()
    (score, hsp, off, ops), name_b = in_small_chunks(handle, sweep, lambda: handle.extend_batch(q, s, ext, mins))
    (score_r, hsp_r, off_r, codes), name_r = in_small_chunks(handle, sweep, lambda: handle.extend_batch_rle(q, s, ext, mins))
    (score_l, index, hsp_l, off_l, codes_l), name_l = in_small_chunks(handle, sweep, lambda: handle.extend_batch_list(q, s, ext, mins))
    for name in (name_b, name_r, name_l):
        assert ("sweep_mq_kernel" in name) == bool(sweep), name
    assert (score_r == score).all() and (score_l == score).all()
    surv = np.nonzero((ext["q_len"] > 0) & (ext["s_len"] > 0) & (score >= mins))[0]
    assert len(surv) >= 10
    # the list is exactly the survivors of the row forms
    assert len(index) == len(surv) and (np.sort(index) == surv).all()
    assert (hsp_l["ops_shift"] == 0).all()
    for f in FIELDS:
        assert (hsp_r[f] == hsp[f]).all(), f
        assert (hsp_l[f] == hsp_r[f][index]).all(), f
    place = {int(i): k for k, i in enumerate(index)}
    for i in surv:
        n_ops = int(hsp[i]["n_ops"])
        assert n_ops > 0
        st = int(off[i]) + int(hsp[i]["ops_shift"])
        mine = codes_of(codes, int(off_r[i]) + int(hsp_r[i]["ops_shift"]), n_ops)
        assert capi.Handle.expand_ops(np.frombuffer(mine, dtype=np.uint8), n_ops) == bytes(ops[st: st + n_ops]), i
        assert codes_of(codes_l, off_l[place[int(i)]], n_ops) == mine, i
