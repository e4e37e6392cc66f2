"""The packed-half sweep's biased frame (lx_score_f16.hip): the skewed frame is raised by B = |g2| + |ge| * G so that no value of
the sweep is negative, and the two wave-constant gap adds of a cell pair, A = h + g2 and E = max(E, A) + ge, are 32-bit integer
subtracts of both halves at once.  A subtract that borrowed would corrupt the neighbouring half, so the cases sit where a minuend is
smallest -- the first rows of a window, the first column of a strip, the first lane group's E = -inf beside a finite neighbour --,
where the gap costs (and with them B) are largest, and at the exactness gate, which B has moved.

Built like tests/test_gpu_pair_slots.py: every batch is made for a condition, the condition is asserted on the ORACLE's output before
the GPU is asked, the kernel's name is asserted, and every score and every survivor's record and ops are compared with the oracle.

Two things the scoring interface rules out, so they are not cases here: gap_extend = 0 (lx_set_scoring wants gap_extend < 0), and a
scheme whose B alone exceeds the range (gap_open >= -120 and gap_extend >= -27 give B <= 119 + 27 * 16 = 551).  A gap cannot open in
a window's row 0 on an optimal path either (one matched cell never pays for a gap): row 1 is the first."""
import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import limit_cases, oracle_lib
from tests.limit_gpu import run_dev
from tests.test_gpu_pair_lanes import P, Q_ONLY, S_ONLY, W, kernel_for, pack, rand, run_gpu_dev
from tests.test_gpu_pair_slots import gap_ops, oracle_alignments, run_gpu, tryptophan_batch
from tests.test_oracle import SCHEMES

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)  # (per test: tests.limit_gpu.run_dev leaves the options at their defaults)
def _single_sweep_one_query_per_wavefront(handle):
    before = {o: handle.get_option(o) for o in (capi.LX_OPT_PASS2_MODE, capi.LX_OPT_MQ_SWEEP)}
    handle.set_option(capi.LX_OPT_PASS2_MODE, 2)
    handle.set_option(capi.LX_OPT_MQ_SWEEP, 0)
    handle.set_option(capi.LX_OPT_ADAPT_PERMILLE, handle.get_option(capi.LX_OPT_ADAPT_PERMILLE))
    yield
    for o, v in before.items():
        handle.set_option(o, v)
    handle.set_scoring(SCHEMES["blosum62"], 0)


def frame_bias(sc, G):
    """B as the kernel and the planner add it: |g2| + |ge| * G, g2 = (cost of a gap's first character) - gap_extend."""
    return (sc.gap_extend - sc.gap_open) + (-sc.gap_extend) * G


def biased_bound(sc, qq, ls_max, G):
    """The kernel's exactness test with the bias in: the wavefront is taken iff this is at most 2046."""
    M = sc.matrix_np()[: sc.alphabet_size, : sc.alphabet_size].astype(np.int64)
    steps = (ls_max + G - 1 + 3) & ~3
    return int(np.maximum(M.max(axis=1), 0)[qq & 31].sum()) + (-sc.gap_extend) * (steps + G + 2) + int(M.max()) - sc.gap_extend + 2 + frame_bias(sc, G)


def test_bias_of_the_schemes_under_test():
    b62 = SCHEMES["blosum62"]
    assert (frame_bias(b62, 8), frame_bias(b62, 16)) == (19, 27)
    assert frame_bias(SCHEMES["blosum62_first31_ext1"], 8) == 38 and frame_bias(SCHEMES["blosum62_first31_ext4"], 8) == 59
    assert {frame_bias(SCHEMES[n], 8) for n in ("nucl", "bs_fwd", "bs_rev")} == {21}


# ---- 1. where Z is lowest: the first rows, the first columns of a strip -------------------------------------------------------------

_M62 = SCHEMES["blosum62"].matrix_np()
CYS, HIS = (int(next(a for a in synth.STD20 if _M62[a, a] == v)) for v in (9, 8))  # the standard residues that score 9 and 8 with themselves
FIRST_LS = (1, 2, 7, 8, 9, 16)


def first_rows_batch(lq, C, seed):
    """One query, sixteen windows of 1, 2, 7, 8, 9 and 16 rows.  Around every strip boundary b = C k the query holds C H W | C
    (columns b - 3 .. b), letters that pay for a gap in pairs.  Window kinds, dealt over the strips in turn:
      col0:  rows H W, then the query from column b + 1 on -- the gap (one query column) opens in row 1, in column 0 of strip k;
      col1:  rows W C, then from b + 2 on -- the same in column 1 of strip k;
      cross: rows C H, then from b + 1 on -- the gap opens in column b - 1 and E ENTERS strip k's first column from the left lane.
    Where the query is too short for a kind, the window is a plain piece of the query."""
    rng = np.random.default_rng(seed)
    qq = rand(rng, lq, avoid=(P, W, CYS, HIS))
    bounds = [C * k for k in range(1, 8) if C * k + 6 <= lq]
    for b in bounds:
        qq[b - 3: b + 1] = (CYS, HIS, W, CYS)
    ws, plan, n = [], [], 0
    for w in range(16):
        ls = FIRST_LS[w % 6] if w < 12 else (9, 16, 8, 7)[w - 12]
        kind, piece = "plain", qq[(5 * w) % max(1, lq - ls + 1):][:ls]
        if ls >= 7 and bounds:  # twelve windows: seven that cross a boundary (every strip's, where there are seven), then col0 / col1 in turn
            b, what = bounds[n % len(bounds)], "cross" if n < 7 else ("col0", "col1")[n % 2]
            n += 1
            first = {"cross": b - 3, "col0": b - 2, "col1": b - 1}[what]
            rest = b + 2 if what == "col1" else b + 1
            if lq - rest >= 4:
                kind, piece = (what, b), np.concatenate([qq[first: first + 2], qq[rest: rest + ls - 2]])
        win = np.full(ls, P, np.uint8)
        win[: len(piece)] = piece
        ws.append(win)
        plan.append(kind)
    return pack([qq], [ws]), plan


def check_first_rows(oracle, lq, C, q, s, ext, plan):
    """The planned gaps are what the oracle aligns: one query column skipped (two for `cross`) between the window's rows 1 and 2."""
    score, al = oracle_alignments(oracle, q, s, ext, 1)
    assert len(al) == 16 and sorted({int(x) for x in ext["s_len"]}) == list(FIRST_LS)
    seen = set()
    for w, kind in enumerate(plan):
        if kind == "plain":
            continue
        what, b = kind
        cols = {"col0": [b], "col1": [b + 1], "cross": [b - 1, b]}[what]
        if gap_ops(al[w], Q_ONLY) == [(j, 2) for j in cols] and al[w][0].s_begin == 0:
            seen.add((what, b // C))
    if lq >= C + 6:
        strips = {k for k in range(1, 8) if C * k + 6 <= lq}
        assert {k for what, k in seen if what == "cross"} == strips, (seen, plan)  # E enters the first column of every such strip
        assert {what for what, k in seen} == {"cross", "col0", "col1"}, (seen, plan)
    return seen


@pytest.mark.parametrize("lq,route", [(1, "host"), (8, "host"), (19, "host"), (20, "host"), (152, "host"), (1, 152), (19, 152), (20, 152),
                                      (104, "host"), (200, "host"), (208, "host")])
def test_first_rows_and_first_columns(handle, oracle, lq, route):
    """Windows of 1 to 16 rows (every step on the checked path, most of a strip's cells in rows before or behind the window), queries
    of 1 to 208 columns in runs of 16, on all four checkpointing geometries: (8,13) for up to 104 columns, (8,19) -- also for the short
    queries under the promise of a widest query of 152, whose strips then lie wholly beyond the query --, (8,25) and (16,13)."""
    C = 19 if route == 152 else 13 if lq <= 104 or lq > 200 else 19 if lq <= 152 else 25
    (q, s, ext), plan = first_rows_batch(lq, C, 6100 + lq + C)
    check_first_rows(oracle, lq, C, q, s, ext, plan)
    if route == 152:
        assert run_gpu_dev(handle, oracle, q, s, ext, 1, 152, "score_pair_kernel<8,19,true>") == 16
    else:
        # (at 200 and 208 columns the plan keeps the int32 launch behind the sweep: a query of tryptophans that wide would be declined)
        run_gpu(handle, oracle, q, s, ext, 1, kernel_for(lq, 16), n_surv=16, fixup=False if lq <= 152 else None)


# ---- 2. the largest admitted gap costs ----------------------------------------------------------------------------------------------


def gap_cost_batch(scheme, seed):
    """150 columns, sixteen windows of 160 to 175 rows, each the query from its row 0 on with two columns left out behind its first
    twelve letters, six letters put in from row 22 + w % 4 on (rows 24 .. 31 are the strips' second row checkpoints) and two columns
    left out again behind which ten letters follow.  The filler is proline, which the protein query does not hold, or N."""
    rng = np.random.default_rng(seed)
    protein = scheme.startswith("blosum")
    fill = P if protein else 4
    qq = rand(rng, 150, avoid=(P,)) if protein else rng.integers(0, 4, 150).astype(np.uint8)
    ws = []
    for w in range(16):
        r = 22 + w % 4
        head = np.concatenate([qq[:12], qq[14:]])
        body = np.concatenate([head[:r], np.full(6, fill, np.uint8), head[r:]])
        piece = np.concatenate([body[:-12], body[-10:]])
        win = np.full(160 + w, fill, np.uint8)
        win[: len(piece)] = piece
        ws.append(win)
    return pack([qq], [ws])


@pytest.mark.parametrize("scheme", ["blosum62_first31_ext1", "blosum62_first31_ext4", "nucl", "bs_fwd", "bs_rev"])
def test_gaps_under_the_largest_gap_costs(handle, oracle, scheme):
    """A gap's first character at 31 with extensions of 1 and 4 (B = 38 and 59), and the nucleotide and both bisulfite schemes of the
    benchmark's other lines (B = 21): a gap near either end of the window and one across the first row checkpoint."""
    q, s, ext = gap_cost_batch(scheme, 6200)
    sc = SCHEMES[scheme]
    assert biased_bound(sc, q[:150], 175, 8) <= 2046  # the packed-half kernel takes the wavefront
    score, al = oracle_alignments(oracle, q, s, ext, 1, scheme)
    assert len(al) == 16
    for w, a in al.items():
        ins, dele = gap_ops(a, Q_ONLY), gap_ops(a, S_ONLY)
        rows = sorted(i for j, i in dele)
        assert len(ins) == 4 and len(dele) == 6, (w, ins, dele)
        assert ins[0][1] - a[0].s_begin == 12 and a[0].s_end - ins[-1][1] == 10, (w, ins)          # near either end
        assert rows == list(range(22 + w % 4, 28 + w % 4)) and a[0].s_begin == 0, (w, rows)  # rows 24 .. 31: the second row checkpoints
    # (whether an int32 launch stands behind the sweep is the plan's a-priori matter -- with extensions of 4 it does --; the kernel
    # itself takes this wavefront, as asserted above)
    run_gpu(handle, oracle, q, s, ext, 1, "score_pair_kernel<8,19,true>", n_surv=16, scheme=scheme)


# ---- 3. the moved gate ----------------------------------------------------------------------------------------------------------------

GATE_LQ, GATE_LS = 169, (105, 121, 137, 138, 141, 153, 169)  # windows of 16 k + 9 rows and right behind the one at the gate


def test_gate_arithmetic():
    """BLOSUM62 11/1 on the (8,25) strips: B = 19, and 169 tryptophans against 137 rows are 11 * 169 + (144 + 10) + 14 + 19 = 2046 in
    planner and kernel alike; a row more gives 2050 in the kernel (148 steps) and 2062 in the planner (160)."""
    sc = limit_cases.blosum62()
    assert frame_bias(sc, 8) == 19 and 11 * 169 + (144 + 10) + 14 + 19 == 2046
    q = np.full(GATE_LQ, W, np.uint8)
    kernel = [biased_bound(sc, q, ls, 8) for ls in GATE_LS]
    plans = [capi.plan_step(sc, GATE_LQ, ls, 16, 48, pass2_mode=2, mq_sweep=1, adapt_permille=0) for ls in GATE_LS]
    assert kernel == [2014, 2030, 2046, 2050, 2050, 2062, 2078]
    assert [int(p.score_bound) for p in plans] == [2014, 2030, 2046, 2062, 2062, 2062, 2078]
    assert [bool(p.may_decline) for p in plans] == [k > 2046 for k in kernel] == [False] * 3 + [True] * 4
    assert all((p.group_lanes, p.strip_cols, p.family) == (8, 25, capi.PLAN_HALF) for p in plans)


@pytest.mark.parametrize("ls", GATE_LS)
def test_gate_with_the_bias_in(handle, oracle, ls):
    """The family of test_a_priori_bound_across_2046 at the place the gate has moved to: the int32 launch is issued exactly where the
    plan says the sweep may decline, which is where the kernel's own test (bias in) fails, and every member is exact."""
    sc = limit_cases.blosum62()
    handle.set_scoring(sc, 0)
    osc = oracle_lib.scoring_from(sc)
    q, s, ext, target = limit_cases.family_member(GATE_LQ, ls)
    want = oracle.score_batch(q, s, ext, osc, threads=4)
    assert (want == target).all()
    plan = capi.plan_step(sc, GATE_LQ, ls, 16, len(ext), pass2_mode=2, mq_sweep=1, adapt_permille=0)
    score, hsp, off, ops, name = run_dev(handle, q, s, ext, 16, 60, 2)
    assert "score_pair_kernel<8,25,true>" in name and plan.name.decode() == name, (plan.name, name)
    assert ("int32 fix-up" in name) == bool(plan.may_decline) == (biased_bound(sc, q[:GATE_LQ], ls, 8) > 2046), (ls, name)
    assert (score == want).all(), (ls, name, plan.score_bound, score[score != want][:4])
    live = np.nonzero(want >= 60)[0]
    n_ops = min(GATE_LQ, ls - 3)
    assert len(live) == 9 and (hsp["score"][live] == want[live]).all() and (hsp["n_ops"][live] == n_ops).all()
    for i in live:
        at = int(off[i]) + int(hsp[i]["ops_shift"])
        assert bytes(ops[at: at + n_ops]) == b"M" * n_ops, (ls, i)


@pytest.mark.parametrize("gap", [False, True])
def test_values_pass_1024_earlier(handle, oracle, gap):
    """152 tryptophans against 176 rows (tests/test_gpu_pair_slots.py): with the bias in, the values leave the subnormals for the first
    binade nineteen units earlier and reach 1672 + 184 + 19; the kernel's test admits 1899, so no int32 launch stands behind it."""
    q, s, ext = tryptophan_batch(gap)
    assert biased_bound(SCHEMES["blosum62"], q[:152], 176, 8) == 1672 + (184 + 10) + 14 + 19 == 1899
    score, al = oracle_alignments(oracle, q, s, ext, 1)
    assert len(al) == 16 and (gap or (score == 1672).all())
    run_gpu(handle, oracle, q, s, ext, 1, "score_pair_kernel<8,19,true>", n_surv=16, fixup=False)
