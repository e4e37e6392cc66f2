"""The packed-half single sweep's own number domain and slots (lx_score_f16.hip, score_pair_kernel<G,C,true>): every value of the
kernel is a multiple of 2^-24 -- half-precision subnormals and the first binade, whose bit patterns are the integers --, and the
checkpoint codes of the two windows of a lane group leave side by side, one window in the low half of a dword and the other in the
high half (CkptPairLayout, lx_device.h); the backtrace (lx_ckpt.hip) takes a window's half by the window's parity in its pair.

Built like tests/test_gpu_pair_lanes.py: every batch is made for a condition, the condition is asserted on the ORACLE's output before
the GPU is asked, the GPU goes through the single sweep with one query per wavefront (LX_OPT_MQ_SWEEP = 0), the kernel's name is
asserted, and scores, coordinates, op bytes and run-length codes are compared with the oracle (tests.test_gpu_bt_walk._check).
Each case is one or two wavefronts."""
import numpy as np
import pytest

from lambda_amd import capi
from tests import oracle_lib
from tests.test_gpu_bt_walk import _check
from tests.test_gpu_pair_lanes import P, Q_ONLY, S_ONLY, W, kernel_for, pack, rand, run_gpu_dev, walk
from tests.test_oracle import SCHEMES

pytestmark = pytest.mark.gpu

# a gap's first character at the compact codes' limit of 31 (lambda's gap_open excludes the first extension), with both ends of
# what a further character may cost beside it
SCHEMES.setdefault("blosum62_first31_ext1", capi.builtin_scoring(62, gap_open=-30, gap_extend=-1))
SCHEMES.setdefault("blosum62_first31_ext4", capi.builtin_scoring(62, gap_open=-27, gap_extend=-4))


@pytest.fixture(scope="module", autouse=True)
def _single_sweep_one_query_per_wavefront(handle):
    before = {o: handle.get_option(o) for o in (capi.LX_OPT_PASS2_MODE, capi.LX_OPT_MQ_SWEEP)}
    handle.set_option(capi.LX_OPT_PASS2_MODE, 2)
    handle.set_option(capi.LX_OPT_MQ_SWEEP, 0)
    # (setting it forgets the survivor share of the last batch another module ran: the adaptive mode would leave the sweep at < 3 %)
    handle.set_option(capi.LX_OPT_ADAPT_PERMILLE, handle.get_option(capi.LX_OPT_ADAPT_PERMILLE))
    yield
    for o, v in before.items():
        handle.set_option(o, v)


def oracle_alignments(oracle, q, s, ext, cutoff, scheme="blosum62"):
    osc = oracle_lib.scoring_from(SCHEMES[scheme])
    score = oracle.score_batch(q, s, ext, osc, threads=8)
    surv = np.nonzero((score >= cutoff) & (score > 0))[0]
    return score, dict(zip(surv.tolist(), oracle.align_batch(q, s, ext[surv], osc)))


def gap_ops(al, op):
    """(query column, window row) of the alignment's ops of one kind"""
    return [(j, i) for o, j, i in walk(*al) if o == op]


def kernel_bound(scheme, qq, ls_max, G=8):
    """The packed-half kernel's exactness test (lx_score_f16.hip): it takes a wavefront iff this is at most 2046."""
    sc = SCHEMES[scheme]
    M = sc.matrix_np()[: sc.alphabet_size, : sc.alphabet_size].astype(np.int64)
    rowmax = np.maximum(M.max(axis=1), 0)
    steps = (ls_max + G - 1 + 3) & ~3
    return int(rowmax[qq & 31].sum()) + (-sc.gap_extend) * (steps + G + 2) + int(M.max()) - sc.gap_extend + 2


def run_gpu(handle, oracle, q, s, ext, cutoff, kernel, n_surv=None, scheme="blosum62", fixup=None):
    n, gaps, ops = _check(handle, oracle, q, s, ext, cutoff, scheme=scheme)
    name = handle.last_trace_kernel_name()
    assert "single sweep" in name and kernel in name, name
    assert fixup is None or ("int32 fix-up" in name) == fixup, name
    assert n_surv is None or n == n_surv
    return n


# ---- 1. which half of a dword ---------------------------------------------------------------------------------------------------

GAP_COL = 8  # the planted gaps sit in front of column 19 k + 8 of every strip k


def half_batch(nwin, parity, seed):
    """One query of 150 letters.  The windows of one parity hold the query with a gap inside every strip: two query letters left out
    in the even strips, two prolines put in in the odd ones.  Their neighbours in the pair are random windows."""
    rng = np.random.default_rng(seed)
    qq = rand(rng, 150, avoid=(P,))
    qq[146:] = W
    ws = []
    for w in range(nwin):
        if w % 2 != parity:
            ws.append(rand(rng, 200))
            continue
        piece, at = [], 0
        for k in range(8):
            c = 19 * k + GAP_COL
            piece.append(qq[at:c])
            if k % 2 == 0:
                at = c + 2
            else:
                piece.append(np.full(2, P, np.uint8))
                at = c
        piece = np.concatenate(piece + [qq[at:]])
        win = np.full(200, P, np.uint8)
        win[3 + w: 3 + w + len(piece)] = piece
        ws.append(win)
    return pack([qq], [ws])


def check_half_batch(oracle, nwin, parity, q, s, ext):
    score, al = oracle_alignments(oracle, q, s, ext, 100)
    assert sorted(al) == [w for w in range(nwin) if w % 2 == parity]  # the random neighbours stay below the cut-off
    for w, a in al.items():
        in_window = {j // 19 for j, i in gap_ops(a, Q_ONLY)}
        in_query = {j // 19 for j, i in gap_ops(a, S_ONLY)}
        assert in_window == {0, 2, 4, 6} and in_query == {1, 3, 5, 7}, (w, in_window, in_query)  # a gap inside every strip
    assert len({int(score[w]) for w in al}) == 1 and len({int(ext["s_off"][w]) for w in al}) == len(al)


@pytest.mark.parametrize("nwin,parity", [(16, 0), (16, 1), (15, 0), (15, 1), (17, 0), (17, 1)])
def test_a_window_reads_its_own_half_of_every_code(handle, oracle, nwin, parity):
    """Only the even (then only the odd) windows of a run are homologous, with a gap inside every strip: their backtrace reads boundary
    codes and row checkpoints of every strip, and the other half of each of those dwords belongs to a random window.  A run of 15
    leaves the last pair's B half idle, a run of 17 begins a second wavefront."""
    q, s, ext = half_batch(nwin, parity, 5100 + 2 * nwin + parity)
    check_half_batch(oracle, nwin, parity, q, s, ext)
    run_gpu(handle, oracle, q, s, ext, 100, "score_pair_kernel<8,19,true>", n_surv=(nwin + 1 - parity) // 2)


# ---- 2. step counts ---------------------------------------------------------------------------------------------------------------

STEP_LS = [1, 5, 8, 9, 16, 17, 25, 176]


def steps_of(ls_max, G=8):
    return (ls_max + G - 1 + 3) & ~3


def steps_batch(ls, seed):
    """A 150-column query and one wavefront of sixteen windows of `ls` letters: pieces of the query; from 25 letters on with four
    prolines put in around row 16, at 176 letters around row 32 as well (and a long gap further down)."""
    rng = np.random.default_rng(seed)
    qq = rand(rng, 150, avoid=(P,))
    ws = []
    for w in range(16):
        if ls < 25:
            a = (9 * w) % (150 - ls + 1)
            ws.append(qq[a: a + ls].copy())
            continue
        r1, r2 = 13 + w % 4, 29 + w % 4  # the gaps' first rows: rows r1 .. r1 + 3 hold row 16, r2 .. r2 + 3 hold row 32
        gap = np.full(4, P, np.uint8)
        a = 5 * w if ls == 25 else 0
        if ls == 25:
            piece = np.concatenate([qq[a: a + r1], gap, qq[a + r1:]])[:ls]
        else:  # (eighteen more prolines in front of column 100: the copy ends in the window's last row)
            piece = np.concatenate([qq[:r1], gap, qq[r1: r2 - 4], gap, qq[r2 - 4: 100], np.full(ls - 158, P, np.uint8), qq[100:]])
        win = np.full(ls, P, np.uint8)
        win[: len(piece)] = piece
        ws.append(win)
    return pack([qq], [ws])


def check_steps_batch(oracle, ls, q, s, ext):
    score, al = oracle_alignments(oracle, q, s, ext, 1)
    assert len(al) == 16
    if ls >= 25:
        for w, a in al.items():
            rows = {i for j, i in gap_ops(a, S_ONLY)}
            assert 16 in rows and (ls == 25 or 32 in rows), (w, sorted(rows))
        assert any(15 in {i for j, i in gap_ops(a, S_ONLY)} for a in al.values())  # ... and crosses into it from row 15
    assert any(a[0].s_end == ls for a in al.values())  # an alignment that ends in the window's last row: the last steps' codes


def test_step_counts_cover_the_cases():
    steps = [steps_of(ls) for ls in STEP_LS]
    assert {st & 4 for st in steps} == {0, 4}             # a last, half-filled group of eight and none
    assert min(steps) < 16 and steps.count(16) and max(steps) > 32  # no row checkpoint, one, several


@pytest.mark.parametrize("ls", STEP_LS)
def test_step_counts_and_gaps_across_row_checkpoints(handle, oracle, ls):
    """Windows of 1 to 176 letters against 150 columns: step counts with and without a last half group of eight, with no, one and
    several row checkpoints, and gaps in the query that cross rows 16 and 32."""
    q, s, ext = steps_batch(ls, 5200 + ls)
    check_steps_batch(oracle, ls, q, s, ext)
    run_gpu(handle, oracle, q, s, ext, 1, "score_pair_kernel<8,19,true>", n_surv=16)


# ---- 3. strip edges and geometries ------------------------------------------------------------------------------------------------


def geometry_batch(lq, C, seed):
    """One query, 16 windows of prolines (the query has none).  Windows 0-5: the query's prefix that ends in the middle of a strip.
    Queries of at least two strips: windows 6-9 hold the query without the four letters around a strip boundary (a gap in the window
    that crosses it), windows 10-13 hold it with two prolines put in inside the last real strip.  The others: plain copies."""
    rng = np.random.default_rng(seed)
    nstrips = (lq + C - 1) // C
    qq = rand(rng, lq, avoid=(P,))
    if lq >= 2 * C:
        qq[-4:] = W
    last0 = (nstrips - 1) * C
    ins = last0 + max(1, (lq - last0) // 2)  # the prolines stand in front of this column
    ws, plan = [], []
    for w in range(16):
        kind, piece = "copy", qq
        if w < 6:
            e = min(lq, C * (w % nstrips) + C // 2 + 1)
            kind, piece = "prefix", qq[:e]
        elif lq >= 2 * C and w < 10:
            b = 1 + w % (nstrips - 1)
            kind, piece = ("cross", b), np.concatenate([qq[: b * C - 2], qq[b * C + 2:]])
        elif lq >= 2 * C and w < 14:
            kind, piece = "last", np.concatenate([qq[:ins], np.full(2, P, np.uint8), qq[ins:]])
        win = np.full(lq + 40, P, np.uint8)
        win[3 + w: 3 + w + len(piece)] = piece
        ws.append(win)
        plan.append(kind)
    return pack([qq], [ws]), plan, ins


def check_geometry_batch(oracle, lq, C, q, s, ext, plan, ins):
    score, al = oracle_alignments(oracle, q, s, ext, 1)
    assert len(al) == 16
    nstrips = (lq + C - 1) // C
    assert {(al[w][0].q_end - 1) // C for w in range(6)} == set(range(min(nstrips, 6)))
    assert any(a[0].q_end == lq for a in al.values())
    for w, kind in enumerate(plan):
        if kind == "last":
            assert gap_ops(al[w], S_ONLY) == [(ins, 3 + w + ins), (ins, 3 + w + ins + 1)], (w, gap_ops(al[w], S_ONLY))
            assert (ins - 1) // C == ins // C == nstrips - 1  # between two columns of the last real strip
        elif kind not in ("copy", "prefix"):
            b = kind[1]
            assert {j for j, i in gap_ops(al[w], Q_ONLY)} == set(range(b * C - 2, b * C + 2)), (w, b)
    assert lq < 2 * C or ("last" in plan and sum(k not in ("copy", "prefix", "last") for k in plan) == 4)


@pytest.mark.parametrize("lq", [1, 19, 20, 38, 150, 152])
def test_strip_edges_on_the_8_19_strips(handle, oracle, lq):
    """Query lengths around a strip's 19 columns and the panel's 152, all on the (8,19) strips under the promise of a widest query of
    152 (lx_extend_batch_dev): strips wholly beyond the query, a query that ends on a strip's last column and on a strip's first.
    From two strips on: a gap in the last real strip and one that crosses a strip boundary."""
    (q, s, ext), plan, ins = geometry_batch(lq, 19, 5300 + lq)
    check_geometry_batch(oracle, lq, 19, q, s, ext, plan, ins)
    assert run_gpu_dev(handle, oracle, q, s, ext, 1, 152, "score_pair_kernel<8,19,true>") == 16


@pytest.mark.parametrize("lq,C", [(104, 13), (200, 25), (208, 13)])
def test_the_other_geometries(handle, oracle, lq, C):
    """(8,13) with 104 columns, (8,25) with 200 and a run of 16, (16,13) with 208 (eight windows per wavefront, four pairs): each with
    a gap in the last real strip and one that crosses a strip boundary.  (8,25) has seven quads per row checkpoint, (8,13) four."""
    (q, s, ext), plan, ins = geometry_batch(lq, C, 5300 + lq)
    check_geometry_batch(oracle, lq, C, q, s, ext, plan, ins)
    run_gpu(handle, oracle, q, s, ext, 1, kernel_for(lq, 16), n_surv=16)


# ---- 4. the number range ------------------------------------------------------------------------------------------------------------


def tryptophan_batch(gap):
    """152 tryptophans against windows of 176 letters: tryptophans behind w prolines (window w), or -- gap -- 110 tryptophans, six
    prolines and tryptophans again."""
    qq = np.full(152, W, np.uint8)
    ws = []
    for w in range(16):
        win = np.full(176, W, np.uint8)
        win[:w] = P
        if gap:
            win[w + 110: w + 116] = P
        ws.append(win)
    return pack([qq], [ws])


@pytest.mark.parametrize("gap", [False, True])
def test_values_beyond_1024(handle, oracle, gap):
    """H grows by 11 per cell along the diagonal and passes 1024, where the kernel's values leave the subnormals for the first binade,
    in every strip's rows; row checkpoints and boundary codes hold values on both sides of it.  The score of 1672 is what the
    kernel's exactness test still admits, so no int32 launch stands behind the sweep.  With a gap opened beyond column 100."""
    q, s, ext = tryptophan_batch(gap)
    score, al = oracle_alignments(oracle, q, s, ext, 1)
    assert len(al) == 16 and kernel_bound("blosum62", q[:152], 176) <= 2046
    if gap:
        for w, a in al.items():
            g = gap_ops(a, S_ONLY)
            assert len(g) == 6 and g[0][0] == 110 and score[w] > 1024 + 11 * 42, (w, g)  # opened where H is 1210
    else:
        assert (score == 1672).all()
    run_gpu(handle, oracle, q, s, ext, 1, "score_pair_kernel<8,19,true>", n_surv=16, fixup=False)


# ---- 5. the gap field of a row code -----------------------------------------------------------------------------------------------

# (strip, column in it, checkpoint, first row of the gap minus the checkpoint's row, length): a gap in the query whose only row is
# the one below the checkpoint's (there F = H + the first character's cost: the field at its top) or the checkpoint's own, and
# gaps of five rows that begin there or three rows above (inside a gap F = H + an extension's cost: the field at its bottom)
GAP_PLANS = [(g, c, m, d, n) for (g, c, m) in ((1, 4, 1), (3, 12, 1), (5, 7, 2)) for (d, n) in ((1, 1), (0, 1), (1, 5), (0, 5), (-3, 5))]


def gap_field_batch(seed):
    """120 columns, windows of 150 rows: strip g keeps rows 16 m + 15 - g.  One plan per window, sixteen windows (the last plan twice)."""
    rng = np.random.default_rng(seed)
    qq = rand(rng, 120, avoid=(P, W))
    ws, want = [], []
    for g, c, m, d, n in GAP_PLANS + GAP_PLANS[-1:]:
        col, r0 = 19 * g + c, 16 * m + 15 - g + d  # the gap sits behind this column; its first row
        a = max(0, col + 1 - r0)                   # the copy begins at query column a, in row r0 - (col + 1 - a)
        at = r0 - (col + 1 - a)
        piece = np.concatenate([qq[a: col + 1], np.full(n, P, np.uint8), qq[col + 1:]])
        win = np.full(150, P, np.uint8)
        win[at: at + len(piece)] = piece
        ws.append(win)
        want.append((col, r0, n))
    return pack([qq], [ws]), want


@pytest.mark.parametrize("scheme", ["blosum62_first31_ext1", "blosum62_first31_ext4"])
def test_gap_field_at_both_ends_of_its_range(handle, oracle, scheme):
    """A gap's first character costs 31, the most a code's five-bit field holds, a further one 1 or 4.  A row checkpoint's code in the
    column of a gap in the query holds H - F = 31 where the gap opens in the row below, and 1 (4) where the checkpoint's row lies
    inside the gap."""
    (q, s, ext), want = gap_field_batch(5500)
    sc = SCHEMES[scheme]
    assert sc.gap_open == -31 and sc.gap_extend == (-1 if scheme.endswith("1") else -4)
    assert kernel_bound(scheme, q[:120], 150) <= 2046  # the packed-half kernel takes the wavefront
    score, al = oracle_alignments(oracle, q, s, ext, 100, scheme)
    assert len(al) == 16
    for w, (col, r0, n) in enumerate(want):
        assert gap_ops(al[w], S_ONLY) == [(col + 1, r0 + t) for t in range(n)], (w, col, r0, n)
    run_gpu(handle, oracle, q, s, ext, 100, "score_pair_kernel<8,19,true>", n_surv=16, scheme=scheme)


# ---- 6. two slot kinds in one list ------------------------------------------------------------------------------------------------


def test_overflow_slot_beside_pair_slots(handle, oracle):
    """152 tryptophans against windows of 360 rows fail the packed-half kernel's exactness test: the wavefront is declined, the int32
    launch gives its windows int16-pair slots in the overflow area.  The query beside it keeps its pair slots."""
    rng = np.random.default_rng(5600)
    big, small = np.full(152, W, np.uint8), rand(rng, 150, avoid=(P,))
    wb, wsm = [], []
    for w in range(16):
        win = np.full(360, P, np.uint8)
        win[20 * w: 20 * w + 60] = W  # sixty tryptophans somewhere
        wb.append(win)
        win = np.full(200, P, np.uint8)
        piece = np.concatenate([small[:70], small[72:]])
        win[w: w + len(piece)] = piece
        wsm.append(win)
    q, s, ext = pack([big, small], [wb, wsm])
    assert kernel_bound("blosum62", big, 360) > 2046 >= kernel_bound("blosum62", small, 200)
    score, al = oracle_alignments(oracle, q, s, ext, 100)
    assert len(al) == 32 and (score[:16] == 660).all()
    assert all(len(gap_ops(al[w], Q_ONLY)) == 2 for w in range(16, 32))
    run_gpu(handle, oracle, q, s, ext, 100, "score_pair_kernel<8,19,true>", n_surv=32, fixup=True)
