"""The lists of tests/test_gpu_backtrace_lockstep.py that are built by hand: windows whose optimal alignment has one gap of a
chosen length at a chosen place."""
import numpy as np

from lambda_amd import capi

NUCL = np.array([0, 1, 2, 4], dtype=np.uint8)  # A C G T (rank 3 is N)
# most lanes short, one or two long: the situation the walk's cut acts in
GAP_MIX = [1, 2, 1, 3, 1, 2, 5, 1, 2, 3, 8, 1, 2, 1, 3, 15, 1, 2, 5, 16, 1, 2, 3, 17, 1, 1, 2, 31, 1, 2, 3, 40]


def gap_cost(g):
    return 5 + 2 * g  # SCHEMES["nucl"]: +2 / -3, first gap character -7, further ones -2


def gap_list(nq, C, lq, seed):
    """nq queries of lq residues with a run of 16 windows each (the shared-profile sweeps, whose geometry follows lq): every window
    is an exact copy of its query with one gap of GAP_MIX's lengths -- alternately vertical (the window has g residues more) and
    horizontal (it lacks g of the query's) -- between two flanks of matches that each outweigh the gap, so that the gap is
    optimal.  The windows' lead-in takes every value mod 16 and the gap's column moves through the strips, every fourth one
    exactly onto a strip border: gaps start and end on tile rows and on strip borders.  Two windows of every run have a short gap
    6-8 cells from the alignment's end / from its begin (first and last tile).  A length that does not fit lq with its flanks
    becomes a gap of one."""
    rng = np.random.default_rng(seed)
    queries = NUCL[rng.integers(0, 4, (nq, lq))]
    ss, rows = [], []
    so = 0
    for k in range(nq * 16):
        Q = queries[k // 16]
        g = GAP_MIX[k % len(GAP_MIX)]
        horizontal = (k // len(GAP_MIX) + k) % 2 == 1
        if lq - (g if horizontal else 0) < 2 * (gap_cost(g) // 2 + 3):
            g, horizontal = 1, False
        fmin = gap_cost(g) // 2 + 3
        room = lq - (g if horizontal else 0)  # residues of the two flanks together
        edge = k % 8 if g <= 3 else -1
        if edge == 6:    # near the end (the backtrace's first tile)
            a = room - (6 + k % 3)
        elif edge == 7:  # near the begin (its last tile)
            a = 6 + k % 3
        else:
            a = fmin + (k * 7) % (room - 2 * fmin + 1)
            if k % 4 == 0 and a + (-a) % C <= room - fmin:
                a += (-a) % C  # exactly on a strip border
        w = np.concatenate([Q[:a], NUCL[rng.integers(0, 4, g)], Q[a:]]) if not horizontal else np.concatenate([Q[:a], Q[a + g:]])
        win = np.concatenate([NUCL[rng.integers(0, 4, k % 16)], w, NUCL[rng.integers(0, 4, 5 + k % 7)]])
        rows.append(((k // 16) * lq, so, lq, len(win)))
        ss.append(win)
        so += len(win)
    pad = np.zeros(256, np.uint8)
    return np.concatenate([queries.reshape(-1), pad]), np.concatenate(ss + [pad]), np.array(rows, dtype=capi.EXT_DTYPE)


# name -> (strip geometry of the sweep and the backtrace, query length, the list)
WALK_CASES = {
    "g8x13": ((8, 13), 80, lambda: gap_list(12, 13, 80, seed=813)),     # gaps up to 31 (17 where the query has the surplus)
    "g8x19": ((8, 19), 150, lambda: gap_list(10, 19, 150, seed=819)),   # all of them, the vertical ones between flanks of >= 60 matches
    "g16x13": ((16, 13), 206, lambda: gap_list(8, 13, 206, seed=1613)),
}
