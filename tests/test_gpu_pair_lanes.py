"""The packed-half single sweep (lx_score_f16.hip, score_pair_kernel<G,C,true>) where a lane's number decides something:
which group and strip a lane is, who its left neighbour is, where its boundary codes and row checkpoints go, which part
of the LDS profile it builds.  Everything goes through lx_extend_batch with the single sweep and is compared with the
oracle: scores, coordinates, op bytes (as column bytes and as run-length codes) and the five counts.

Every batch is built for a condition, and the condition is asserted on the ORACLE's output before the GPU is asked: a case
cannot pass without being the case it was meant to be.  The one-query-per-wavefront kernels are what is under test, so the
multi-query sweep (LX_OPT_MQ_SWEEP), which would take runs of 8 and ragged runs, is switched off for the module.

lx_extend_batch pads every run to whole groups of 8 or 16 slots with empty windows, so an idle B half is the empty window
beside a run's last real one.  It also orders a list by the queries' geometry class (lx_host_plan.h: query_class; at most 104
columns, at most 152, ...) and never puts two classes into one chunk (lx_host_plan.cpp: HostPlan::run_chunk_end), so on that entry point a query
of at most 104 columns runs on the (8,13) strips whatever else the list holds.  The strip-edge cases therefore run twice:
through lx_extend_batch, on the strips the library picks, and through lx_extend_batch_dev under the promise
LX_OPT_MAX_QLEN = 152, which puts all seven lengths on the (8,19) strips -- with strips that lie wholly beyond the query."""
import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import oracle_lib
from tests.test_gpu_bt_walk import _check
from tests.test_oracle import SCHEMES

pytestmark = pytest.mark.gpu

A = synth.STD20
P, W = 15, 22  # proline, tryptophan: s(P, W) = -4, s(W, W) = 11 in BLOSUM62
Q_ONLY, S_ONLY = ord("I"), ord("D")  # an op that uses up a query column only (a gap in the window) / a window row only


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


def kernel_for(lq, run):
    if lq <= 104:
        return "score_pair_kernel<8,13,true>"
    if lq <= 152:
        return "score_pair_kernel<8,19,true>"
    return "score_pair_kernel<8,25,true>" if lq <= 200 and run % 16 == 0 else "score_pair_kernel<16,13,true>"


def rand(rng, n, avoid=()):
    pool = np.array([a for a in A if a not in avoid], dtype=np.uint8)
    return pool[rng.integers(0, len(pool), n)]


def pack(queries, windows):
    """queries[k]: residues; windows[k]: the windows of query k, in order.  -> q, s, ext (runs of one query, as lambda lists them)"""
    q = np.concatenate(queries).astype(np.uint8)
    q_off = np.concatenate([[0], np.cumsum([len(x) for x in queries])[:-1]])
    flat = [w for ws in windows for w in ws]
    s = np.concatenate(flat).astype(np.uint8)
    ext = np.zeros(len(flat), dtype=capi.EXT_DTYPE)
    ext["q_off"] = np.repeat(q_off, [len(ws) for ws in windows])
    ext["q_len"] = np.repeat([len(x) for x in queries], [len(ws) for ws in windows])
    ext["s_len"] = [len(w) for w in flat]
    ext["s_off"] = np.concatenate([[0], np.cumsum(ext["s_len"])[:-1]])
    return q, s, ext


def oracle_alignments(oracle, q, s, ext, cutoff):
    osc = oracle_lib.scoring_from(SCHEMES["blosum62"])
    score = oracle.score_batch(q, s, ext, osc, threads=8)
    surv = np.nonzero((score >= cutoff) & (score > 0))[0]
    return score, dict(zip(surv.tolist(), oracle.align_batch(q, s, ext[surv], osc)))


def walk(hsp, ops):
    """(op byte, query column, window row) of every op of an oracle alignment"""
    j, i, out = hsp.q_begin, hsp.s_begin, []
    for o in ops:
        out.append((o, j, i))
        j += o != S_ONLY
        i += o != Q_ONLY
    assert (j, i) == (hsp.q_end, hsp.s_end)
    return out


def run_gpu(handle, oracle, q, s, ext, cutoff, kernel, n_surv=None):
    n, gaps, ops = _check(handle, oracle, q, s, ext, cutoff)
    name = handle.last_trace_kernel_name()
    assert "single sweep" in name and kernel in name, name
    assert n_surv is None or n == n_surv
    return n, gaps, ops


def run_gpu_dev(handle, oracle, q, s, ext, cutoff, max_qlen, kernel):
    """The same comparison through lx_extend_batch_dev: the slots as they are (whole runs of 16), the strips picked by the caller's
    promise of the widest query."""
    import torch

    n, dev = len(ext), torch.device("cuda:0")
    pad = np.zeros(256, np.uint8)
    d_q, d_s = torch.from_numpy(np.concatenate([q, pad])).to(dev), torch.from_numpy(np.concatenate([s, pad])).to(dev)
    d_ext = torch.from_numpy(ext.view(np.uint8).copy()).to(dev)
    sizes = ext["q_len"].astype(np.uint64) + ext["s_len"].astype(np.uint64)
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(sizes)[:-1]
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ops = torch.zeros(int(sizes.sum()) + 16, dtype=torch.uint8, device=dev)
    d_hsp = torch.zeros(n * capi.HSP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_score = torch.zeros(n, dtype=torch.int32, device=dev)
    d_count = torch.zeros(2, dtype=torch.int64, device=dev)
    handle.set_scoring(SCHEMES["blosum62"], 0)
    handle.set_option(capi.LX_OPT_MAX_QLEN, max_qlen)
    handle.set_option(capi.LX_OPT_MAX_SLEN, int(ext["s_len"].max()))
    handle.set_option(capi.LX_OPT_QUERY_RUN, 16)
    torch.cuda.synchronize()
    try:
        handle.extend_batch_dev(d_q, d_s, d_ext, n, cutoff, d_score, d_hsp, d_ops, d_off, d_count)
        handle.synchronize()
        name = handle.last_trace_kernel_name()
    finally:
        for o in (capi.LX_OPT_MAX_QLEN, capi.LX_OPT_MAX_SLEN, capi.LX_OPT_QUERY_RUN):
            handle.set_option(o, 0)
    assert "single sweep" in name and kernel in name, name
    score, ops = d_score.cpu().numpy(), d_ops.cpu().numpy()
    hsp = np.frombuffer(d_hsp.cpu().numpy().tobytes(), dtype=capi.HSP_DTYPE)
    osc = oracle_lib.scoring_from(SCHEMES["blosum62"])
    want_score, al = oracle_alignments(oracle, q, s, ext, cutoff)
    assert (score == want_score).all() and int(d_count.cpu().numpy()[1]) == len(al)
    for i, (oh, oops) in al.items():
        x = ext[i]
        st = oracle.alignment_stats(q[int(x["q_off"]): int(x["q_off"]) + int(x["q_len"])], s[int(x["s_off"]): int(x["s_off"]) + int(x["s_len"])],
                                    oh, oops, osc, 0)
        want = (oh.score, oh.q_begin, oh.q_end, oh.s_begin, oh.s_end, oh.n_ops, st.num_matches, st.num_mismatches, st.num_positives,
                st.num_gap_opens, st.num_gap_extensions)
        got = tuple(int(hsp[i][f]) for f in ("score", "q_begin", "q_end", "s_begin", "s_end", "n_ops", "num_matches", "num_mismatches",
                                             "num_positives", "num_gap_opens", "num_gap_extensions"))
        assert got == want, (i, got, want)
        at = int(off[i]) + int(hsp[i]["ops_shift"])
        assert bytes(ops[at: at + oh.n_ops]) == oops, i
    return len(al)


# ---- 1. lane map ------------------------------------------------------------------------------------------------------------


def lane_map_batch(lq, run, seed):
    """Runs of `run` windows, the last one three short of it (its last real window has an empty window as its pair); window w of a
    query holds the query's first 24 + 5 w letters: every slot of a run has a score of its own."""
    rng = np.random.default_rng(seed)
    nq = 3 if run == 16 else 5
    queries = [rand(rng, lq, avoid=(P,)) for _ in range(nq)]
    windows = []
    for k, qq in enumerate(queries):
        ws = []
        for w in range(run - 3 * (k == nq - 1)):
            win = np.full(lq + 40, P, np.uint8)
            keep = min(lq, 24 + 5 * w)
            at = 3 + (7 * w + k) % 30
            win[at: at + keep] = qq[:keep]
            ws.append(win)
        windows.append(ws)
    return pack(queries, windows)


LANE_MAP = [(150, 16), (100, 16), (200, 16), (205, 16), (150, 8), (100, 8), (205, 8)]


def check_lane_map_batch(oracle, lq, run, q, s, ext):
    score, al = oracle_alignments(oracle, q, s, ext, 30)
    assert len(al) == len(ext)
    at = 0
    while at < len(ext):
        k = int((ext["q_off"] == ext["q_off"][at]).sum())
        sc = score[at: at + k]
        assert len(set(sc.tolist())) == k and (np.diff(sc) > 0).all()  # a slot's score says which slot it is
        at += k
    assert len(ext) % 2 == 1  # the last real window has no real partner


@pytest.mark.parametrize("lq,run", LANE_MAP)
def test_every_slot_of_a_wavefront_keeps_its_own_window(handle, oracle, lq, run):
    """3 queries x 16 windows (one profile per wavefront) and 5 queries x 8 windows (two profiles per wavefront of the 8-lane
    geometries), in all four geometries: a lane group that took another group's pair, or the other half of its own, would
    report that window's score and alignment."""
    q, s, ext = lane_map_batch(lq, run, 4100 + lq + run)
    check_lane_map_batch(oracle, lq, run, q, s, ext)
    run_gpu(handle, oracle, q, s, ext, 30, kernel_for(lq, run), n_surv=len(ext))
    # what the library made of the runs: padded to `run` slots each, not to 16 -- runs of 8 on an 8-lane geometry are two queries
    # (two profiles) per wavefront, and five of them leave the last wavefront half filled
    nq = len(np.unique(ext["q_off"]))
    assert handle.last_extend_stats()[:2] == (len(ext), nq * run)
    assert run == 16 or (nq * run) % 16 == 8


# ---- 2. strip edges and the end cell ------------------------------------------------------------------------------------------


def strip_edge_batch(lq, seed, C):
    """One query, 16 windows of tryptophans (the query has none; 8 and 9: of prolines).  Window w < 8 holds the query's prefix that ends
    in the middle of strip w of C columns (w modulo the strips the query has); windows 8 and 9, for the long queries, hold twice, 48 rows apart, a twelve-letter
    word that the query has in strips 1 and 5; the others hold the whole query."""
    rng = np.random.default_rng(seed)
    nstrips = (lq + C - 1) // C
    qq = rand(rng, lq, avoid=(P, W))
    word = rand(rng, 12, avoid=(P, W))
    if lq >= 112:
        qq[20:32] = word
        qq[100:112] = word
    ws = []
    for w in range(16):
        win = np.full(max(lq, 70) + 30, W, np.uint8)
        if w in (8, 9) and lq >= 112:
            win[:] = P                  # (the query has none either, and nothing scores against it: the word's ends are the alignment's)
            win[5 + w: 17 + w] = word   # its last letter in row 16 + w: block 1
            win[53 + w: 65 + w] = word  # ... in row 64 + w: block 4
        else:
            e = lq if w >= 8 else min(lq, C * (w % nstrips) + C // 2 + 1)
            win[3 + w: 3 + w + e] = qq[:e]
        ws.append(win)
    return pack([qq], [ws]), word


def check_strip_edge_batch(oracle, lq, C, q, s, ext, word):
    score, al = oracle_alignments(oracle, q, s, ext, 1)
    assert len(al) == 16
    strips = {(al[w][0].q_end - 1) // C for w in range(16)}
    assert strips == set(range((lq + C - 1) // C)), strips  # the end column falls into every strip the query has
    assert any(al[w][0].q_end == lq for w in range(16))
    if lq >= 112:
        osc = oracle_lib.scoring_from(SCHEMES["blosum62"])
        self_score = int(oracle.score(word, word, osc)[0])
        for w in (8, 9):  # the word's score, met in (rows 16 + w, 64 + w) x (columns 31, 111): two strips, two blocks of sixteen rows
            assert score[w] == self_score and al[w][0].q_end in (32, 112) and al[w][0].s_end in (17 + w, 65 + w)


STRIP_EDGE_LQ = [1, 18, 19, 20, 133, 150, 152]


@pytest.mark.parametrize("lq", STRIP_EDGE_LQ)
def test_end_cell_in_every_strip_and_met_twice(handle, oracle, lq):
    """The (8,19) strips at query lengths around a strip's 19 columns and around the panel's 152, under the promise of a widest query
    of 152: one column, a query that ends on a strip's last column (19, 133, 152) and on a strip's first (20),
    strips that lie wholly beyond the query (all but the first one or two at 1 - 20: the profile's padding), the end column in every
    strip the query has, and a best value that two strips and two blocks of sixteen rows reach."""
    (q, s, ext), word = strip_edge_batch(lq, 4200 + lq, 19)
    check_strip_edge_batch(oracle, lq, 19, q, s, ext, word)
    assert run_gpu_dev(handle, oracle, q, s, ext, 1, 152, "score_pair_kernel<8,19,true>") == 16


@pytest.mark.parametrize("lq", STRIP_EDGE_LQ)
def test_end_cell_in_every_strip_on_the_strips_the_library_picks(handle, oracle, lq):
    """The same through lx_extend_batch: at most 104 columns run on the (8,13) strips there, and the windows are built for those."""
    C = 13 if lq <= 104 else 19
    (q, s, ext), word = strip_edge_batch(lq, 4200 + lq, C)
    check_strip_edge_batch(oracle, lq, C, q, s, ext, word)
    run_gpu(handle, oracle, q, s, ext, 1, kernel_for(lq, 16), n_surv=16)


# ---- 3. boundaries between lanes ----------------------------------------------------------------------------------------------


def lane_boundary_batch(seed):
    """lq 150, (8,19).  Windows 0-2: the query's first 60 letters from row 0, 1, 40 on.  Windows 3-9: a copy of the query without
    the four letters 19 k - 2 .. 19 k + 1 (a gap in the window across the strip boundary).  Windows 10-15: plain copies."""
    rng = np.random.default_rng(seed)
    qq = rand(rng, 150, avoid=(P,))
    ws = []
    for w in range(16):
        win = np.full(200, P, np.uint8)
        if w < 3:
            at = (0, 1, 40)[w]
            win[at: at + 60] = qq[:60]
        elif w < 10:
            k = w - 2
            piece = np.concatenate([qq[: 19 * k - 2], qq[19 * k + 2:]])
            win[5: 5 + len(piece)] = piece
        else:
            win[w: w + 150] = qq
        ws.append(win)
    return pack([qq], [ws])


def check_lane_boundary_batch(oracle, q, s, ext):
    score, al = oracle_alignments(oracle, q, s, ext, 60)
    assert len(al) == 16
    for w, row in enumerate((0, 1, 40)):
        assert (al[w][0].q_begin, al[w][0].s_begin) == (0, row)
    for k in range(1, 8):
        cols = {j for o, j, i in walk(*al[k + 2]) if o == Q_ONLY}
        assert {19 * k - 1, 19 * k} <= cols, (k, cols)  # E crosses from strip k - 1 into strip k
    for w in range(10, 16):
        cols = {j for o, j, i in walk(*al[w]) if o == ord("M")}
        assert cols == set(range(150))                  # H crosses every strip boundary on the diagonal


def test_values_cross_from_a_strip_to_the_next(handle, oracle):
    """What a lane takes from its left neighbour: nothing in strip 0 (alignments that begin in column 0, at rows 0, 1 and 40), E
    where a gap in the window runs across a strip boundary, H where the diagonal does -- at every one of the seven boundaries."""
    q, s, ext = lane_boundary_batch(4300)
    check_lane_boundary_batch(oracle, q, s, ext)
    run_gpu(handle, oracle, q, s, ext, 60, "score_pair_kernel<8,19,true>", n_surv=16)


# ---- 4. chunks and tails --------------------------------------------------------------------------------------------------------

LENGTHS = (4, 9, 150, 176, 177, 180, 185, 200)


def steps_of(ls_max, G=8):
    return (ls_max + G - 1 + 3) & ~3


def chunk_batch(seed):
    """Query 0: one wavefront with two windows of each length of LENGTHS (its shortest window ends before the steady chunks could
    begin: checked chunks only).  Queries 1-8: a wavefront of sixteen windows of one of these lengths each."""
    rng = np.random.default_rng(seed)
    queries = [rand(rng, 150) for _ in range(1 + len(LENGTHS))]
    windows = []
    for k, qq in enumerate(queries):
        ws = []
        for w in range(16):
            ls = LENGTHS[w // 2] if k == 0 else LENGTHS[k - 1]
            win = rand(rng, ls)
            at = ls - 150 if ls >= 150 else min(w % 5, ls - 1)  # (the copy ends with the window: its last rows are the last steps')
            piece = np.where(rng.random(150) < 0.06, rand(rng, 150), qq)[: ls - at]
            win[at: at + len(piece)] = piece
            ws.append(win)
        windows.append(ws)
    return pack(queries, windows)


def check_chunk_batch(oracle, q, s, ext):
    score, al = oracle_alignments(oracle, q, s, ext, 10)
    assert len(al) >= 16 * 6 + 12  # every window of 150 letters and more, and some of the short ones
    assert min(LENGTHS) - 3 <= (8 - 1 + 3) & ~3                        # the mixed wavefront has no steady chunk
    assert any(steps_of(ls) % 8 == 4 for ls in LENGTHS)                # a tail flush
    assert any(steps_of(ls) % 16 not in (0, 4) for ls in LENGTHS) and any(steps_of(ls) % 16 == 0 for ls in LENGTHS)
    for k in range(1 + len(LENGTHS)):  # every wavefront has alignments that reach its windows' last rows
        sl = range(16 * k, 16 * k + 16)
        assert any(w in al and al[w][0].s_end == int(ext["s_len"][w]) for w in sl), k


def test_checked_chunks_tail_flush_and_partial_block(handle, oracle):
    """The loop around the steps: a wavefront of windows from 4 to 200 letters (no steady chunk at all, every letter fetched with
    its bounds check), and wavefronts whose step counts end in a half group of eight (the tail flush of the boundary codes) and in
    a partial block of sixteen (the last bookkeeping), with alignments that end in those last rows."""
    q, s, ext = chunk_batch(4400)
    check_chunk_batch(oracle, q, s, ext)
    run_gpu(handle, oracle, q, s, ext, 10, "score_pair_kernel<8,19,true>")


# ---- 5. row checkpoints: every code of a checkpoint, both halves of a pair ------------------------------------------------------

ROWCK_CELLS = [(0, 4), (0, 7), (0, 11), (0, 18), (3, 4), (3, 7), (3, 12), (3, 18), (7, 12), (7, 16)]  # (strip, column in it); (7, 16): column 149


def rowck_batch(seed):
    """lq 150, (8,19).  A gap in the query (two window letters with no partner) whose first row is the row below a row checkpoint of
    the gap's column: strip g keeps rows 16 m + 15 - g, m = 0, 1, 2 (for strip 0 rows 15, 31 and 47).  The columns: an even and an
    odd one, one of each quad of the checkpoint's codes, a strip's last, and column 145, the last one behind which a gap still pays
    (four tryptophans follow); every plan on an A and on a B half.  No alignment has a gap in the query's last column: there the copy
    ends in the checkpoint's row, which is where the backtrace then begins."""
    rng = np.random.default_rng(seed)
    plans = [(g, c, m) for m in range(3) for g, c in ROWCK_CELLS]
    plans += [plans[-1]] * (-len(plans) % 8)
    queries, windows, want = [], [], []
    for k in range(len(plans) // 8):
        qq = rand(rng, 150, avoid=(P,))
        qq[146:] = W
        ws = []
        for g, c, m in plans[8 * k: 8 * k + 8]:
            for half in range(2):
                col = 19 * g + c          # the gap sits in this column: below its cell of the checkpoint row
                r0 = 16 * m + 16 - g      # first row of the gap
                a = max(0, col + 1 - r0)  # the copy begins at query column a, in row r0 - (col + 1 - a)
                at = r0 - (col + 1 - a)
                gap = np.full(2, P, np.uint8)
                piece = np.concatenate([qq[a: col + 1], gap, qq[col + 1:]])
                if col == 149:            # the last column: the copy's last letter in row r0 - 1
                    piece = qq[a:]
                win = np.full(230, P, np.uint8)
                win[at: at + len(piece)] = piece[: 230 - at]
                ws.append(win)
                want.append((col, r0))
        queries.append(qq)
        windows.append(ws)
    return pack(queries, windows), want


def check_rowck_batch(oracle, q, s, ext, want):
    score, al = oracle_alignments(oracle, q, s, ext, 40)
    assert len(al) == len(ext)
    for w, (col, r0) in enumerate(want):
        gap = [(j, i) for o, j, i in walk(*al[w]) if o == S_ONLY]
        if col == 149:
            assert not gap and (al[w][0].q_end, al[w][0].s_end) == (150, r0), (w, r0)
            continue
        # the walk reports the column an op starts in front of: a window-only op behind column col stands at j = col + 1
        assert len(gap) == 2 and gap[0] == (col + 1, r0) and al[w][0].q_end == 150, (w, col, r0, gap)


def test_gap_opens_below_a_row_checkpoint(handle, oracle):
    """The backtrace recomputes a tile from the row checkpoint above it: a vertical gap that begins in the tile's first row takes
    H and F of exactly one code of that checkpoint."""
    (q, s, ext), want = rowck_batch(4500)
    check_rowck_batch(oracle, q, s, ext, want)
    run_gpu(handle, oracle, q, s, ext, 40, "score_pair_kernel<8,19,true>", n_surv=len(ext))
