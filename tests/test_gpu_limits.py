"""GPU tests that sit ON the number-range gates of the extension step, from both sides (tests/limit_cases.py builds the inputs,
tests/test_limit_cases.py proves their true scores on the CPU):

  2046 / 2047   what the packed-half sweep and the compact 16-bit checkpoint codes hold: the a-priori bound per wavefront
                (lx_score_f16.hip, lx_sweep_mq.hip) and the best score after the sweep (lx_score_i16.hip COMPACT && MULTI, lx_sweep_mq.hip)
  29695         0x7BFF - 2048, the biased 16-bit integer sweeps (kI16Limit, kMqLimit)
  32000, 65535  the host's admission of checkpoint mode (fits_int16, lx_step_plan.cpp)
  31            the gap field of the compact codes (kC16MaxGap)

Every case: scores bit for bit against the oracle over the whole batch; for every survivor the record with its five counts and the op
bytes (the run-length codes expanded, where the entry point has them); and the kernel that ran, so that no case passes through a
fall-back.  (The single-panel COMPACT form of sweep_pair16_kernel is not here: nothing launches it -- plan_step takes the compact
integer sweep only for queries wider than a panel.)"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lambda_amd import capi
from tests import limit_cases, oracle_lib
from tests.limit_gpu import FIELDS, cached, check_list, check_rle_rows, check_rows, dev_scores, oracle_results, run_dev

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

SWEEPS = {"one_panel_16": ("score_pair_kernel<8,25,true>", 16), "one_panel_32": ("score_pair_kernel<8,25,true>", 32),
          "three_panels": ("sweep_pair16_kernel<8,19,true,true,true>", 16)}


# ---- 3a: true scores 2044 .. 2050 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [2, 1, 0])
@pytest.mark.parametrize("case", sorted(SWEEPS))
def test_true_scores_around_2046_device_lists(handle, oracle, case, mode):
    """One-panel queries of 190 columns in runs of 16 and 32 (packed-half sweep: the a-priori bound sends the W-rich wavefronts to the
    int32 launch, their neighbours stay) and 450-column queries (compact integer sweep: declines by extension, after the sweep, what
    scored beyond 2046): planted verbatim and with one gap, early and late in the window, the score collected over all panels or
    complete before the last one."""
    kernel, run = SWEEPS[case]
    sc, q, s, ext, target = cached(case)
    handle.set_scoring(sc, 0)
    ores = oracle_results(oracle, case, sc, q, s, ext, 60)
    assert set(limit_cases.TARGETS_2046) <= set(ores[0].tolist())
    score, hsp, off, ops, name = run_dev(handle, q, s, ext, run, 60, mode)
    if mode == 2:
        assert kernel in name and "single sweep" in name and "int32 fix-up" in name, name
    else:
        assert ("ckpt_forward_kernel" if mode == 1 else "trace_forward_kernel") in name and "sweep" not in name, name
    check_rows(ores, score, hsp, off, ops, (case, mode, name))


@pytest.mark.parametrize("case", sorted(SWEEPS))
def test_true_scores_around_2046_pass1(handle, oracle, case):
    """lx_score_batch_dev with the packed kernels on (score_pair_kernel / sweep_pair16_kernel, CKPT = false) and off."""
    _, run = SWEEPS[case]
    sc, q, s, ext, target = cached(case)
    handle.set_scoring(sc, 0)
    want = oracle_results(oracle, case, sc, q, s, ext, 60)[0]
    got, name = dev_scores(handle, q, s, ext, run, 1)
    assert ("sweep_pair16_kernel<8,19,true,false>" if case == "three_panels" else "score_pair_kernel<8,24>") in name and "fix-up" in name, name
    assert (got == want).all(), np.nonzero(got != want)[0][:8]
    got32, name32 = dev_scores(handle, q, s, ext, run, 0)
    assert "pair" not in name32 and (got32 == want).all(), name32


def host_calls(handle, oracle, key, sc, q, s, ext, cutoff, mode):
    """lx_extend_batch, lx_extend_batch_rle and lx_extend_batch_list on one list; returns the kernel names."""
    ores = oracle_results(oracle, key, sc, q, s, ext, cutoff)
    names = []
    handle.set_option(capi.LX_OPT_PASS2_MODE, mode)
    try:
        score, hsp, off, ops = handle.extend_batch(q, s, ext, cutoff)
        names.append(handle.last_trace_kernel_name())
        check_rows(ores, score, hsp, off, ops, (key, "rows", names[-1]))
        score, hsp, off, codes = handle.extend_batch_rle(q, s, ext, cutoff)
        names.append(handle.last_trace_kernel_name())
        check_rle_rows(ores, score, hsp, off, codes, (key, "rle", names[-1]))
        score, index, hsp, off, codes = handle.extend_batch_list(q, s, ext, cutoff)
        names.append(handle.last_trace_kernel_name())
        check_list(ores, score, index, hsp, off, codes, (key, "list", names[-1]))
    finally:
        handle.set_option(capi.LX_OPT_PASS2_MODE, 1)
    return names


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_true_scores_around_2046_ragged_host_list(handle, oracle, mode):
    """The ragged list through the three host entry points.  Mode 2 is the multi-query sweep: the first call writes compact codes and
    leaves what scored beyond 2046 to the int32 launch; it counts those windows (a third of this list), so the calls after it run the
    WIDE form -- int16-pair slots, nothing declined below 29695."""
    sc, q, s, ext, target = cached("ragged_list")
    handle.set_scoring(sc, 0)
    if mode == 2:  # (a handle that has not seen strong hits lately: two lists of ordinary windows)
        from lambda_amd import synth

        q0, s0, e0 = synth.make_ragged_lists_np(40, seed=6, lq_range=(160, 400), mean_windows=4.0)
        handle.set_option(capi.LX_OPT_PASS2_MODE, 2)
        try:
            for _ in range(2):
                handle.extend_batch_list(q0, s0, e0, 60)
        finally:
            handle.set_option(capi.LX_OPT_PASS2_MODE, 1)
    names = host_calls(handle, oracle, "ragged_list", sc, q, s, ext, 60, mode)
    if mode == 2:
        assert "sweep_mq_kernel<19,true,false>" in names[0] and "int32 fix-up" in names[0], names
        assert "sweep_mq_kernel<19,true,true>" in names[2], names
    else:
        assert all("sweep" not in n for n in names), names


def test_true_scores_around_2046_compact_codes_only(tmp_path, oracle):
    """The same list in a process with LX_MQ_NO_WIDE: the multi-query sweep keeps its compact codes in every call, and its own count
    of the windows beyond them is at least the number of windows that truly score beyond 2046."""
    sc, q, s, ext, target = cached("ragged_list")
    want, surv, want_ops, want_rec = oracle_results(oracle, "ragged_list", sc, q, s, ext, 60)
    out = tmp_path / "no_wide.npz"
    env = dict(os.environ, LX_MQ_NO_WIDE="1", LX_HOST_TIMING="1")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "limit_cases_child.py"), str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    for k in range(3):
        assert "sweep_mq_kernel<19,true,false>" in str(got[f"kernel{k}"]) and "int32 fix-up" in str(got[f"kernel{k}"])
        check_list((want, surv, want_ops, want_rec), got[f"score{k}"], got[f"index{k}"], got[f"hsp{k}"], got[f"off{k}"], got[f"codes{k}"], ("no wide", k))
    import re

    # the sweep's own count of the windows beyond the codes, per call (one chunk each).  Every wavefront here is MULTI, whose bound is
    # tested against 29695, so nothing is declined up front: the count is the number of slots whose best score is above 2046 -- the
    # windows that truly score so, and at most one filler (a copy of its last window) per query that has such windows
    beyond = [int(x) for x in re.findall(r"(\d+) beyond the codes", r.stderr)]
    over = want > 2046
    n_over, q_over = int(over.sum()), len(set(ext["q_off"][over].tolist()))
    assert "(wide)" not in r.stderr and len(beyond) == 3 and n_over > 0, (beyond, r.stderr[-1500:])
    assert all(n_over <= b <= n_over + q_over for b in beyond), (beyond, n_over, q_over)


# ---- 3b: the a-priori bound ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rows", "cols", "mq_rows"])
def test_a_priori_bound_across_2046(handle, oracle, kind):
    """All-W queries whose bound grows with the window length or by eleven per column, over a range that holds the point where it passes
    what half precision and the compact codes hold; `rows` and `cols` through score_pair_kernel (runs of 16), `mq_rows` through the
    one-panel multi-query sweep (runs of 4, 146 columns).  The row families have a member whose bound is 2046 in planner and kernel
    alike and one right behind it (limit_cases.case_bound_family).  lx_plan_step says for each member whether the sweep may decline;
    the run must agree -- the int32 launch is issued exactly where the plan says so --, and every member is exact: a sweep that
    declined where the plan had promised it would not leaves the sentinel -1 for all to see."""
    sc = limit_cases.blosum62()
    handle.set_scoring(sc, 0)
    osc = oracle_lib.scoring_from(sc)
    run, mq, nq, kernel = (4, 2, 8, "sweep_mq_kernel<19,false,false>") if kind == "mq_rows" else (16, 1, 3, "score_pair_kernel")
    declines, bounds = [], []
    for lq, ls in limit_cases.case_bound_family(kind):
        q, s, ext, target = limit_cases.family_member(lq, ls, run=run, n_queries=nq)
        want = oracle.score_batch(q, s, ext, osc, threads=4)
        assert (want == target).all()
        plan = capi.plan_step(sc, lq, ls, run, len(ext), pass2_mode=2, mq_sweep=mq, adapt_permille=0)
        score, hsp, off, ops, name = run_dev(handle, q, s, ext, run, 60, 2, mq=mq)
        assert kernel in name and plan.name.decode() == name, (plan.name, name)
        assert ("int32 fix-up" in name) == bool(plan.may_decline), (lq, ls, name)
        assert (score == want).all(), (lq, ls, name, plan.score_bound, score[score != want][:4])
        live = np.nonzero(want >= 60)[0]
        assert (hsp["score"][live] == want[live]).all() and (hsp["n_ops"][live] == min(lq, ls - 3)).all()
        declines.append(bool(plan.may_decline))
        bounds.append(int(plan.score_bound))
    assert not declines[0] and declines[-1], declines
    assert declines == sorted(declines) and bounds == sorted(bounds)  # one flip, where the bound grows
    flip = declines.index(True)
    assert bounds[flip - 1] < bounds[flip]


def test_a_priori_bound_across_29695_wide_multi_query_sweep(handle, oracle):
    """The WIDE multi-query sweep (int16-pair slots) is the one 16-bit sweep whose plan issues no int32 launch while its bound stays
    within 29695, so here the flip shows: limit_cases.mq_wide_family steps the bound from below 29695 to exactly 29695 (planner and
    kernel alike) and on beyond it.  Every member must be exact -- a kernel that declines where the plan issued no int32 launch leaves
    -1 --, the lowest member runs without the launch, the highest with it, and there is one flip."""
    sc = limit_cases.mq_wide_scoring()
    handle.set_scoring(sc, 0)
    osc = oracle_lib.scoring_from(sc)
    fixups = []
    handle.set_option(capi.LX_OPT_PASS2_MODE, 2)
    try:
        fam = limit_cases.mq_wide_family()
        _, (q, s, ext, target) = limit_cases.mq_wide_member(*fam[0])
        for _ in range(2):  # (every window scores beyond the compact codes: the handle learns it and sweeps WIDE from here on)
            handle.extend_batch_list(q, s, ext, 60)
        for ls, low in fam:
            _, (q, s, ext, target) = limit_cases.mq_wide_member(ls, low)
            want = oracle.score_batch(q, s, ext, osc, threads=8)
            assert (want == target).all()
            score, index, hsp, off, codes = handle.extend_batch_list(q, s, ext, 60)
            name = handle.last_trace_kernel_name()
            assert "sweep_mq_kernel<19,true,true>" in name, (ls, low, name)
            assert (score == want).all(), (ls, low, name, score[score != want][:4])
            assert sorted(index.tolist()) == list(range(len(ext)))
            for k, i in enumerate(index):
                n_ops = int(ext["q_len"][i]) if want[i] == target.max() else 700
                assert (int(hsp[k]["score"]), int(hsp[k]["n_ops"]), int(hsp[k]["num_gap_opens"])) == (int(want[i]), n_ops, 0), (ls, low, i)
                assert capi.Handle.expand_ops(codes[int(off[k]):], n_ops) == b"M" * n_ops
            fixups.append("int32 fix-up" in name)
    finally:
        handle.set_option(capi.LX_OPT_PASS2_MODE, 1)
        handle.set_scoring(limit_cases.blosum62(), 0)
    assert not fixups[0] and fixups[-1] and fixups == sorted(fixups), fixups


def test_a_priori_bound_across_29695(handle, oracle):
    """The limit of the 16-bit integer sweep with int16-pair slots (sweep_pair16_kernel<8,19,MULTI>, kI16Limit): 30 per column, 940 ..
    970 columns.  That sweep always has the int32 launch behind it (the plan never promises otherwise: may_decline stays 1) and no
    count of what it declined leaves the library, so which side of the limit a member fell on CANNOT be observed here: this test shows
    only that the members come back exact on both sides -- it catches a limit so high that the 16-bit patterns overflow, not one
    that is off by a few.  The flip itself is pinned where it can be seen, in the WIDE multi-query sweep above."""
    for lq in limit_cases.wide_family():
        sc, (q, s, ext, target) = limit_cases.wide_member(lq)
        handle.set_scoring(sc, 0)
        try:
            want = oracle.score_batch(q, s, ext, oracle_lib.scoring_from(sc), threads=4)
            assert (want == target).all()
            plan = capi.plan_step(sc, lq, lq + 20, 16, len(ext), pass2_mode=2, adapt_permille=0)
            score, hsp, off, ops, name = run_dev(handle, q, s, ext, 16, 60, 2)
        finally:
            handle.set_scoring(limit_cases.blosum62(), 0)
        assert "sweep_pair16_kernel<8,19,true>" in name and "int32 fix-up" in name and plan.may_decline == 1, (lq, name)
        assert (score == want).all(), (lq, plan.score_bound, score[score != want][:4])
        live = np.nonzero(want >= 60)[0]
        assert (hsp["score"][live] == want[live]).all() and (hsp["n_ops"][live] == lq).all()
    first = capi.plan_step(limit_cases.custom_scoring(gap_open=-32), 940, 960, 16, 32, pass2_mode=2, adapt_permille=0).score_bound
    last = capi.plan_step(limit_cases.custom_scoring(gap_open=-32), 970, 990, 16, 32, pass2_mode=2, adapt_permille=0).score_bound
    assert first < 0x7BFF - 2048 < last  # (the range holds the flip)


# ---- 3c: true scores around 29695 ----------------------------------------------------------------------------------------------

def test_true_scores_around_29695_int16_pair_sweep(handle, oracle):
    """Custom matrix, 1040 columns, true scores 29692 .. 29698 and 31100, through sweep_pair16_kernel<8,19,MULTI> with int16-pair
    slots.  No 16-bit sweep computes these: the a-priori bound lies about 1100 above the score, so every one of these wavefronts is
    declined up front and the test is of the decline chain -- the int32 launch must return them exact."""
    sc, q, s, ext, target = cached("i16_pairs")
    handle.set_scoring(sc, 0)
    try:
        ores = oracle_results(oracle, "i16_pairs", sc, q, s, ext, 60)
        score, hsp, off, ops, name = run_dev(handle, q, s, ext, 16, 60, 2)
        got, name1 = dev_scores(handle, q, s, ext, 16, 1)
    finally:
        handle.set_scoring(limit_cases.blosum62(), 0)
    assert "sweep_pair16_kernel<8,19,true>" in name and "int32 fix-up" in name, name
    check_rows(ores, score, hsp, off, ops, name)
    assert "sweep_pair16_kernel<8,19,true,false>" in name1 and (got == ores[0]).all(), name1


def test_true_scores_around_29695_wide_multi_query_sweep(handle, oracle):
    """The same targets under gap costs the multi-query sweep takes.  Every window is beyond the compact codes: the first call's
    overflow area runs out and its chunk is run again WIDE, the later calls start WIDE -- and WIDE declines what its bound puts beyond
    29695, which is every wavefront here."""
    sc, q, s, ext, target = cached("i16_mq_wide")
    handle.set_scoring(sc, 0)
    try:
        names = host_calls(handle, oracle, "i16_mq_wide", sc, q, s, ext, 60, 2)
    finally:
        handle.set_scoring(limit_cases.blosum62(), 0)
    assert "sweep_mq_kernel<19,true,true>" in names[2] and "int32 fix-up" in names[2], names


def test_true_scores_around_29695_blosum62(handle, oracle):
    """BLOSUM62, 2702 columns, nearly all W, 8 windows per query: 29695 and 29696 -- the multi-query sweep with compact codes over 18
    panels (MULTI && !WIDE: its bound is tested against 29695, its codes against 2046)."""
    sc, q, s, ext, target = cached("i16_blosum")
    handle.set_scoring(sc, 0)
    ores = oracle_results(oracle, "i16_blosum", sc, q, s, ext, 60)
    score, hsp, off, ops, name = run_dev(handle, q, s, ext, 8, 60, 2)
    assert "sweep_mq_kernel<19,true,false>" in name and "int32 fix-up" in name, name
    assert len(ores[1]) == 4 and (score == ores[0]).all()
    for i, oops, rec in zip(ores[1], ores[2], ores[3]):
        assert tuple(int(hsp[i][f]) for f in FIELDS) == rec
        st = int(off[i]) + int(hsp[i]["ops_shift"])
        assert bytes(ops[st: st + rec[5]]) == oops


# ---- 3d: the host's 32000 and 65535 --------------------------------------------------------------------------------------------

def align_rows(handle, oracle, key, sc, q, s, ext):
    want, surv, want_ops, want_rec = oracle_results(oracle, key, sc, q, s, ext, 1)
    hsp, ops = handle.align_batch(q, s, ext)
    name = handle.last_trace_kernel_name()
    for i, oops, rec in zip(surv, want_ops, want_rec):
        assert tuple(int(hsp[i][f]) for f in FIELDS) == rec, (key, i, name)
        assert ops[i] == oops, (key, i, name)
    return name


@pytest.mark.parametrize("cols", [1066, 1067])
def test_checkpoint_mode_up_to_32000(handle, oracle, cols):
    """30 x 1066 = 31980 is admitted to checkpoint mode (int16 pairs), 30 x 1067 = 32010 is not (direction bits); the true scores are
    the products."""
    key = f"gate_{cols}"
    sc, q, s, ext, target = cached(key)
    handle.set_scoring(sc, 0)
    try:
        name = align_rows(handle, oracle, key, sc, q, s, ext)
        ores = oracle_results(oracle, key, sc, q, s, ext, 1)
        assert ores[0].max() == 30 * cols
        handle.set_option(capi.LX_OPT_PASS2_MODE, 2)
        score, hsp, off, ops = handle.extend_batch(q, s, ext, 1)
        name2 = handle.last_trace_kernel_name()
    finally:
        handle.set_option(capi.LX_OPT_PASS2_MODE, 1)
        handle.set_scoring(limit_cases.blosum62(), 0)
    assert ("ckpt_forward_kernel" in name) == (cols == 1066) and ("trace_forward_kernel" in name) == (cols == 1067), name
    want, surv, want_ops, want_rec = ores
    assert (score == want).all(), name2
    for i, oops, rec in zip(surv, want_ops, want_rec):
        assert tuple(int(hsp[i][f]) for f in FIELDS) == rec, (i, name2)
        st = int(off[i]) + int(hsp[i]["ops_shift"])
        assert bytes(ops[st: st + rec[5]]) == oops, (i, name2)
    assert ("trace_forward_kernel" in name2) == (cols == 1067), name2


def test_checkpoint_mode_largest_score(handle, oracle):
    """31999 = 11 x 2909: the largest score checkpoint mode is ever handed."""
    sc, q, s, ext, target = cached("largest")
    handle.set_scoring(sc, 0)
    name = align_rows(handle, oracle, "largest", sc, q, s, ext)
    assert "ckpt_forward_kernel" in name, name
    assert oracle_results(oracle, "largest", sc, q, s, ext, 1)[0].max() == 31999


@pytest.mark.parametrize("rows", [65535, 65536])
def test_checkpoint_mode_up_to_65535_rows(handle, oracle, rows):
    """A window of 65535 residues is the last the checkpoint slots address, 65536 the first that is traced through direction bits."""
    key = f"rows_{rows}"
    sc, q, s, ext, target = cached(key)
    handle.set_scoring(sc, 0)
    ores = oracle_results(oracle, key, sc, q, s, ext, 40)
    assert ores[0][0] == 777
    score, hsp, off, ops, name = run_dev(handle, q, s, ext, 8, 40, 1)
    assert ("ckpt_forward_kernel" in name) == (rows == 65535) and ("trace_forward_kernel" in name) == (rows == 65536), name
    check_rows(ores, score, hsp, off, ops, name)
    score, hsp, off, ops, name = run_dev(handle, q, s, ext, 8, 40, 2)
    assert ("single sweep" in name) == (rows == 65535) and ("trace_forward_kernel" in name) == (rows == 65536), name
    check_rows(ores, score, hsp, off, ops, name)
    handle.set_option(capi.LX_OPT_PASS2_MODE, 2)
    try:
        score, index, hsp, off, codes = handle.extend_batch_list(q, s, ext, 40)
    finally:
        handle.set_option(capi.LX_OPT_PASS2_MODE, 1)
    check_list(ores, score, index, hsp, off, codes, key)
    assert 0 in index  # (the long window's record is among them)


# ---- 3e: the gap field of the compact codes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", [30, 31, 32])
def test_first_gap_character_at_the_code_limit(handle, oracle, cost):
    """A first gap character of 30, 31 (the last the 5-bit field holds) and 32 (int16 pairs from the int32 kernel), with gaps four
    columns after the alignment's begin and four before its end."""
    sc = capi.builtin_scoring(62, gap_open=-(cost - 1), gap_extend=-1)
    assert sc.gap_open == -cost
    q, s, ext, target = limit_cases.case_gap_field()(sc)
    handle.set_scoring(sc, 0)
    try:
        ores = oracle_results(oracle, f"gap_field_{cost}", sc, q, s, ext, 60)
        score, hsp, off, ops, name = run_dev(handle, q, s, ext, 16, 60, 2)
        handle.set_option(capi.LX_OPT_PASS2_MODE, 2)
        hscore, hhsp, hoff, hops = handle.extend_batch(q, s, ext, 60)
        hname = handle.last_trace_kernel_name()
    finally:
        handle.set_option(capi.LX_OPT_PASS2_MODE, 1)
        handle.set_scoring(limit_cases.blosum62(), 0)
    assert "single sweep" in name and ("score_pair_kernel<8,19,true>" if cost <= 31 else "sweep_pair16_kernel<8,19,false>") in name, name
    assert sum(b"D" in o for o in ores[2]) >= 8
    check_rows(ores, score, hsp, off, ops, name)
    check_rows(ores, hscore, hhsp, hoff, hops, hname)
    assert "single sweep" in hname and ("score_pair_kernel" in hname or "sweep_mq_kernel" in hname) == (cost <= 31), hname
