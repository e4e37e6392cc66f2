"""The checkpoint backtrace's bookkeeping around gaps (lx_ckpt.hip): the writer of 'M' runs, the match count of a diagonal
piece, the hand-over between the diagonal shortcut, the nibble scan and the single-step walk of a tile.  Windows are built
around planted gaps so that every phase of the 16-row x C-column tile grid is hit; op strings, coordinates and the five
counts must equal the oracle's bit for bit, as column bytes and as run-length codes."""
import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import oracle_lib
from tests.test_oracle import SCHEMES, alphabet_of

pytestmark = pytest.mark.gpu

COUNTS = ("num_matches", "num_mismatches", "num_positives", "num_gap_opens", "num_gap_extensions")


def _planted(rng, alphabet, lq, ls, plans, sub_rate=0.08):
    """One query and one window per plan.  A plan is (offset of the copy in the window, [(query position, kind, length), ...]):
    the window holds the query from that offset on, with `length` random letters put in before the query position ('ins': a
    gap in the query) or `length` query letters left out from it on ('del': a gap in the window); the rest is random."""
    n = len(plans)
    q = alphabet[rng.integers(0, len(alphabet), (n, lq))].astype(np.uint8)
    s = alphabet[rng.integers(0, len(alphabet), (n, ls))].astype(np.uint8)
    for x, (off, edits) in enumerate(plans):
        piece, at = [], 0
        for pos, kind, length in sorted(edits):
            piece.append(q[x, at:pos])
            if kind == "ins":
                piece.append(alphabet[rng.integers(0, len(alphabet), length)].astype(np.uint8))
                at = pos
            else:
                at = pos + length
        piece.append(q[x, at:])
        piece = np.concatenate(piece)
        sub = rng.random(len(piece)) < sub_rate
        piece = np.where(sub, alphabet[rng.integers(0, len(alphabet), len(piece))], piece).astype(np.uint8)
        piece = piece[: ls - off]
        s[x, off: off + len(piece)] = piece
    ext = np.zeros(n, dtype=capi.EXT_DTYPE)
    ext["q_off"] = np.arange(n, dtype=np.uint64) * lq
    ext["q_len"] = lq
    ext["s_off"] = np.arange(n, dtype=np.uint64) * ls
    ext["s_len"] = ls
    return q.reshape(-1), s.reshape(-1), ext


def _check(handle, oracle, q, s, ext, cutoff, scheme="blosum62", bs_rule=0):
    handle.set_scoring(SCHEMES[scheme], 0)
    handle.set_option(capi.LX_OPT_BS_MATCH_RULE, bs_rule)
    try:
        osc = oracle_lib.scoring_from(SCHEMES[scheme])
        want_score = oracle.score_batch(q, s, ext, osc, threads=8)
        mins = np.full(len(ext), cutoff, np.int32)
        surv = np.nonzero((want_score >= mins) & (want_score > 0))[0]
        want = oracle.align_batch(q, s, ext[surv], osc)
        score, hsp, off, ops = handle.extend_batch(q, s, ext, mins)
        assert (score == want_score).all()
        name = handle.last_trace_kernel_name()
        assert "single sweep" in name or "ckpt_forward_kernel" in name, name
        score2, hsp2, off2, codes = handle.extend_batch_rle(q, s, ext, mins)
        assert (score2 == want_score).all()
        gaps = 0
        for i, (oh, oops) in zip(surv, want):
            x = ext[i]
            qq = q[int(x["q_off"]): int(x["q_off"]) + int(x["q_len"])]
            ss = s[int(x["s_off"]): int(x["s_off"]) + int(x["s_len"])]
            st = oracle.alignment_stats(qq, ss, oh, oops, osc, bs_rule)
            exp = (oh.score, oh.q_begin, oh.q_end, oh.s_begin, oh.s_end, oh.n_ops, st.num_matches, st.num_mismatches, st.num_positives,
                   st.num_gap_opens, st.num_gap_extensions)
            for g in (hsp[i], hsp2[i]):
                got = tuple(int(g[f]) for f in ("score", "q_begin", "q_end", "s_begin", "s_end", "n_ops") + COUNTS)
                assert got == exp, (i, got, exp)
            at = int(off[i]) + int(hsp[i]["ops_shift"])
            assert bytes(ops[at: at + oh.n_ops]) == oops, i
            c = codes[int(off2[i]): int(off2[i]) + oh.n_ops]
            assert capi.Handle.expand_ops(c, oh.n_ops) == oops, i
            gaps += st.num_gap_opens
        return len(surv), gaps, [w[1] for w in want]
    finally:
        handle.set_option(capi.LX_OPT_BS_MATCH_RULE, 0)


def test_gaps_longer_than_a_tile(handle, oracle):
    """Gaps of 17 to 44 characters, longer than a tile's 16 rows and 19 (13, 25) columns, in both directions: the walk leaves
    the tile inside the gap and the next tile phase continues it."""
    rng = np.random.default_rng(1701)
    plans = []
    for length in range(17, 45):
        for kind in ("ins", "del"):
            for rep in range(4):
                plans.append((int(rng.integers(0, 20)), [(int(rng.integers(45, 75)), kind, length)]))
    q, s, ext = _planted(rng, synth.STD20, 150, 230, plans)
    n, gaps, ops = _check(handle, oracle, q, s, ext, 60)
    assert n == len(plans)
    assert sum(b"D" * 17 in o for o in ops) > 50 and sum(b"I" * 17 in o for o in ops) > 50


def test_gap_ends_on_every_tile_phase(handle, oracle):
    """Short gaps at every query position of two strips and every window offset of one step block: among them gaps that end
    on a tile's first row, its first column or both, and gaps that begin on its last ones."""
    rng = np.random.default_rng(1702)
    plans = []
    for pos in range(30, 70):
        for off in range(0, 17):
            kind = "ins" if (pos + off) & 1 else "del"
            plans.append((off, [(pos, kind, 1 + (pos * 17 + off) % 6)]))
    q, s, ext = _planted(rng, synth.STD20, 150, 190, plans, sub_rate=0.05)
    n, gaps, _ = _check(handle, oracle, q, s, ext, 60)
    assert n == len(plans) and gaps >= n


@pytest.mark.parametrize("run", [15, 16, 17, 32])
def test_diagonal_run_between_two_gaps(handle, oracle, run):
    """Two gaps with a diagonal run of exactly 16 cells (and 15, 17, 32) between them, at every phase of the tile grid: the
    run is handed from the walk to the diagonal routine and back."""
    rng = np.random.default_rng(1703 + run)
    plans = []
    for pos in range(30, 62):
        for off in (0, 3, 7, 12):
            k1 = "ins" if pos & 1 else "del"
            k2 = "ins" if off & 1 else "del"
            plans.append((off, [(pos, k1, 1 + pos % 3), (pos + (pos % 3 + 1 if k1 == "del" else 0) + run, k2, 1 + off % 4)]))
    q, s, ext = _planted(rng, synth.STD20, 150, 190, plans, sub_rate=0.0)
    n, gaps, ops = _check(handle, oracle, q, s, ext, 60)
    assert n == len(plans) and gaps >= 2 * n - 8
    assert sum(any(g + b"M" * run + h in o for g in (b"D", b"I") for h in (b"D", b"I")) for o in ops) > n // 2


def test_alignment_begins_next_to_a_gap(handle, oracle):
    """A head of one to six tryptophans, a gap, then the body: the alignment's first cell lies one to six cells beyond the
    gap, so H = 0 is reached in the tile of the gap -- by the walk, the nibble run or the first shortcut after it."""
    rng = np.random.default_rng(1704)
    plans = []
    for head in range(1, 7):
        for length in (1, 2, 3):
            for off in range(0, 16):
                plans.append((off, [(head, "ins" if off & 1 else "del", length)]))
    q, s, ext = _planted(rng, synth.STD20, 150, 190, plans, sub_rate=0.0)
    q = q.copy().reshape(len(plans), 150)
    s = s.copy().reshape(len(plans), 190)
    for x, (off, edits) in enumerate(plans):
        head = edits[0][0]
        q[x, :head] = 22  # W
        s[x, off: off + head] = 22
        s[x, :off] = 15   # P: nothing before the head scores
    n, gaps, ops = _check(handle, oracle, q.reshape(-1), s.reshape(-1), ext, 60)
    assert n == len(plans)
    assert sum(o[:8].count(b"D") + o[:8].count(b"I") > 0 for o in ops) > 20  # heads that paid for their gap


@pytest.mark.parametrize("scheme,convert", [("bs_fwd", "CT"), ("bs_rev", "GA")])
def test_bisulfite_match_rule_around_gaps(handle, oracle, scheme, convert):
    """bs_match_rule = 1 counts a converted letter as a match: diagonal pieces (counted four letters at a time under the
    plain rule, cell by cell under this one) and walk cells around planted gaps, long ones included."""
    rng = np.random.default_rng(1705)
    plans = []
    for pos in range(25, 65):
        for off in (0, 5, 11):
            kind = "ins" if (pos + off) & 1 else "del"
            plans.append((off, [(pos, kind, 1 + (pos + off) % 5), (pos + 30, "del" if kind == "ins" else "ins", 1 + pos % 24)]))
    q, s, ext = _planted(rng, alphabet_of(scheme)[:4], 120, 190, plans, sub_rate=0.03)
    frm, to = synth.CONVERSIONS[convert]
    q = np.where((q == frm) & (rng.random(len(q)) < 0.9), to, q).astype(np.uint8)
    n, gaps, _ = _check(handle, oracle, q, s, ext, 40, scheme=scheme, bs_rule=1)
    assert n > len(plans) // 2 and gaps > n
