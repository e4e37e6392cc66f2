"""Inputs whose true best local score is a chosen number -- for the tests that sit on the kernels' number-range gates
(tests/test_gpu_limits.py, tests/test_gpu_schemes_edges.py) and for the CPU tests that prove the numbers (tests/test_limit_cases.py).
Plain numpy; nothing here touches a GPU.

How a target T is hit exactly.  A query is a multiset of three letters (top, mid, base) whose diagonal entries are each the maximum
of their matrix row, so no alignment column with that residue can score more than its diagonal.  The window holds the query verbatim
between flanks of letters that score negatively against every query letter.  The full diagonal then scores the sum of the query's
diagonal entries, nothing scores more, and the counts of the three letters are solved so that the sum is T:

    T = base * lq + (top - base) * a + (mid - base) * c,        c = (T - base * lq) / (mid - base)  mod (top - base)

(mid - base and top - base are coprime: BLOSUM62 W / E / A = 11 / 5 / 4 -- or C = 9, H = 8 for the mid letter where E leaves no room --, the small custom matrix 30 / 29 / 1).  A `gap` window has one
flank letter inserted into the planted copy: its query is built for T - gap_open, the best alignment pays one gap of one character.
"""
import ctypes as C

import numpy as np

from lambda_amd import capi, synth

B62_TOP, B62_MID, B62_BASE = 22, [4, 2, 7], 0  # W; E, C or H; A: diagonals 11; 5, 9, 8; 4
CUSTOM_D = 30                          # the custom matrix' largest entry: d - ge = 31, the edge of what pass 2 accepts


def blosum62():
    return capi.builtin_scoring(62, gap_open=-11, gap_extend=-1)


def make_scoring(matrix, gap_open, gap_extend, alphabet_size=None):
    """A capi.Scoring from a small square matrix (first gap character gap_open, every further one gap_extend)."""
    matrix = np.asarray(matrix)
    sc = capi.Scoring()
    sc.alphabet_size = matrix.shape[0] if alphabet_size is None else alphabet_size
    sc.gap_open, sc.gap_extend = gap_open, gap_extend
    m = np.zeros((capi.LX_ALPH, capi.LX_ALPH), dtype=np.int8)
    m[: matrix.shape[0], : matrix.shape[1]] = matrix
    C.memmove(sc.matrix, m.ctypes.data, m.nbytes)
    return sc


def custom_scoring(gap_open=-12, gap_extend=-1, d=CUSTOM_D, off=-4):
    """Four letters: 0 and 1 with diagonals d and d - 1, 2 with diagonal 1 (targets adjustable by one), 3 the flank letter; every
    other entry `off` (negative).  d = 30, ge = -1: d - ge = 31."""
    m = np.full((4, 4), off, dtype=np.int64)
    m[0, 0], m[1, 1], m[2, 2] = d, d - 1, 1
    return make_scoring(m, gap_open, gap_extend)


class Letters:
    """The three query letters and the flank letters of a scheme."""

    def __init__(self, sc, top, mid, base, flank_from):
        self.M = sc.matrix_np().astype(np.int64)
        self.go, self.ge = sc.gap_open, sc.gap_extend
        self.top, self.mids, self.base = top, list(np.atleast_1d(mid)), base
        used = [top, base] + self.mids
        for x in used:
            assert self.M[x, x] == self.M[x, : sc.alphabet_size].max() > 0  # the diagonal is the row's maximum
        self.flank = np.array([f for f in flank_from if all(self.M[f, x] < 0 and self.M[x, f] < 0 for x in used)], dtype=np.uint8)
        assert len(self.flank) > 0

    def diag(self, x):
        return int(self.M[x, x])

    def compose(self, T, lq, rng, tail_top=0):
        """lq residues of (top, mid, base) whose diagonals sum to T, shuffled; the last `tail_top` are top letters."""
        t, b = self.diag(self.top), self.diag(self.base)
        R = T - b * lq
        for mid in self.mids:  # (the first mid letter whose count leaves room: W / E / A cannot make 2061 from 190 letters, W / C / A can)
            m = self.diag(mid)
            c = (R * pow(m - b, -1, t - b)) % (t - b)
            a = (R - (m - b) * c) // (t - b)
            if R >= 0 and a >= tail_top and a + c <= lq:
                break
        assert R >= 0 and a >= tail_top and a + c <= lq and b * lq + (t - b) * a + (m - b) * c == T, (T, lq, a, c)
        q = np.array([self.top] * (a - tail_top) + [mid] * c + [self.base] * (lq - a - c), dtype=np.uint8)
        rng.shuffle(q)
        return np.concatenate([q, np.full(tail_top, self.top, dtype=np.uint8)])

    def flanks(self, n, rng):
        return self.flank[rng.integers(0, len(self.flank), n)]


def b62_letters():
    return Letters(blosum62(), B62_TOP, B62_MID, B62_BASE, synth.STD20)


def custom_letters(sc):
    return Letters(sc, 0, 1, 2, [3])


class Batch:
    """Collects queries and their windows; extensions are query-major, every query's run padded to `run` windows with noise windows
    (flank letters only: score 0)."""

    def __init__(self, run=16):
        self.run = run
        self.q, self.s, self.ext, self.target = [], [], [], []
        self.qo = self.so = 0

    def add_query(self, q, windows, targets, L=None, rng=None, pad_len=None):
        assert len(windows) <= self.run or self.run == 0
        windows, targets = list(windows), list(targets)
        while self.run and len(windows) < self.run:
            windows.append(L.flanks(pad_len or len(windows[0]), rng))
            targets.append(0)
        for w, t in zip(windows, targets):
            self.ext.append((self.qo, self.so, len(q), len(w)))
            self.s.append(np.asarray(w, dtype=np.uint8))
            self.so += len(w)
            self.target.append(t)
        self.q.append(np.asarray(q, dtype=np.uint8))
        self.qo += len(q)

    def add_batch(self, q, s, ext):
        """Ordinary queries (synth.make_batch_np and its kin): targets unknown (-1)."""
        e = ext.copy()
        e["q_off"] += self.qo
        e["s_off"] += self.so
        self.ext += [tuple(x) for x in e.tolist()]
        self.target += [-1] * len(e)
        self.q.append(q)
        self.s.append(s)
        self.qo += len(q)
        self.so += len(s)

    def done(self):
        ext = np.array(self.ext, dtype=capi.EXT_DTYPE)
        return np.concatenate(self.q), np.concatenate(self.s), ext, np.array(self.target, dtype=np.int64)


def plain_window(L, q, rng, left, right):
    return np.concatenate([L.flanks(left, rng), q, L.flanks(right, rng)])


def gap_window(L, q, rng, left, right, at):
    """The copy of q with one flank letter inserted `at` residues before its end (the query was built for T - gap_open)."""
    k = len(q) - at
    return np.concatenate([L.flanks(left, rng), q[:k], L.flanks(1, rng), q[k:], L.flanks(right, rng)])


def add_target_queries(B, L, T, lq, rng, ls, tail_top=4):
    """Two queries for one target: one planted verbatim (early, late, in the middle), one planted with a single gap (in the middle,
    next to the end cell, late in the window).  Every window has `ls` residues (ls >= 2 * lq + 1 puts the late copies in the
    second half); the rest of the run are prefixes of the query (lower scores) and noise."""
    q = L.compose(T, lq, rng)
    room = ls - lq
    wins = [plain_window(L, q, rng, 3, room - 3), plain_window(L, q, rng, room - 2, 2), plain_window(L, q, rng, room // 2, room - room // 2)]
    tg = [T, T, T]
    half = lq // 2
    wins.append(np.concatenate([L.flanks(5, rng), q[:half], L.flanks(ls - 5 - half, rng)]))
    tg.append(int(sum(L.diag(x) for x in q[:half])))
    B.add_query(q, wins, tg, L, rng, ls)
    qg = L.compose(T - L.go, lq, rng, tail_top=tail_top)
    room = ls - lq - 1
    B.add_query(qg, [gap_window(L, qg, rng, 3, room - 3, lq // 2), gap_window(L, qg, rng, 4, room - 4, tail_top - 1),
                     gap_window(L, qg, rng, room - 2, 2, lq // 3), gap_window(L, qg, rng, room - 1, 1, tail_top - 1)], [T, T, T, T], L, rng, ls)


TARGETS_2046 = list(range(2044, 2051))
TARGETS_29695 = list(range(29692, 29699))


def ordinary(B, lq, nq, seed, run=None):
    q, s, ext = synth.make_batch_np(nq, lq, run or B.run, seed=seed, sub_rate=0.15, indel_rate=0.03)
    B.add_batch(q, s, ext)


def case_codes_one_panel(run=16, lq=190):
    """3a, one panel: BLOSUM62 queries of 190 columns with true scores 2044 .. 2050, among ordinary queries of the same width."""
    rng = np.random.default_rng(2046 + run)
    L = b62_letters()
    B = Batch(run)
    ls = 2 * lq + 9
    for k, T in enumerate(TARGETS_2046):
        if k % 2 == 0:
            ordinary(B, lq, 1, 100 + k)
        add_target_queries(B, L, T, lq, rng, ls)
    ordinary(B, lq, 2, 99)
    return B.done()


def case_codes_three_panels(run=16, lq=450):
    """3a, several panels: 450 columns (three panels of 152).  `across`: the W are spread over the query, the score is collected in all
    three panels; `early`: the query's last 146 columns are G, which no window holds, so the score is complete inside the second panel
    and the third only carries it (one panel alone cannot hold it: 152 x 11 = 1672)."""
    rng = np.random.default_rng(450 + run)
    L = b62_letters()
    B = Batch(run)
    ls = lq + 40
    G_ = 6
    assert (L.M[G_, [B62_TOP, B62_BASE] + B62_MID + list(L.flank)] <= 0).all()
    for k, T in enumerate(TARGETS_2046):
        if k % 3 == 0:
            ordinary(B, lq, 1, 200 + k)
        add_target_queries(B, L, T, lq, rng, ls)
        head = L.compose(T, 304, rng)
        q = np.concatenate([head, np.full(lq - 304, G_, dtype=np.uint8)])
        B.add_query(q, [plain_window(L, head, rng, 7, ls - 311), plain_window(L, head, rng, ls - 304 - 2, 2)], [T, T], L, rng, ls)
    return B.done()


def case_codes_ragged_list():
    """3a, a ragged list for lx_extend_batch / _rle / _list (the multi-query sweep): the boundary queries of 190 and 450 columns, few
    windows each, among ordinary queries of 60 - 456 columns."""
    rng = np.random.default_rng(77)
    L = b62_letters()
    B = Batch(0)
    q, s, ext = synth.make_ragged_lists_np(24, seed=9, lq_range=(60, 456), mean_windows=3.0, merged_frac=0.1)
    B.add_batch(q, s, ext)
    for T in TARGETS_2046:
        add_target_queries(B, L, T, 190, rng, 2 * 190 + 9)
        add_target_queries(B, L, T, 450, rng, 450 + 40)
    return B.done()


def case_bound_family(kind):
    """3b: all-W queries whose a-priori bound (sum of row maxima + |ge| x rows swept + ...) steps across the packed-half gate.  The
    planner rounds the rows swept up to a multiple of 16, the kernels to a multiple of 4, so the two bounds are the same number only
    for windows of 16 k + 9 residues (8-lane groups: rows + 7 swept); the members sit on that grid and right behind it.
    `rows`: 162 columns -- 233 residues give 11 x 162 + 240 + 24 = 2046 in planner and kernel alike, the last value admitted; 234 give
    2062 in the planner and 2050 in the kernel.  `mq_rows`: the same for the one-panel multi-query sweep, 146 columns, 409 residues.
    `cols`: a column more adds 11 (150 .. 175 columns, windows of 200).  Returns a list of (lq, ls)."""
    if kind == "rows":
        return [(162, ls) for ls in (201, 217, 233, 234, 237, 249, 265)]
    if kind == "mq_rows":
        return [(146, ls) for ls in (377, 393, 409, 410, 413, 425, 441)]
    return [(lq, 200) for lq in range(150, 176)]


def family_member(lq, ls, run=16, n_queries=3):  # (run 4, 8 queries: the multi-query sweep's family)
    """Queries of lq tryptophans, each with `run` windows of ls residues: the query (as much of it as fits) at three places, the rest
    noise.  True score 11 x min(lq, ls - 3)."""
    rng = np.random.default_rng(lq * 1000 + ls)
    L = b62_letters()
    B = Batch(run)
    q = np.full(lq, B62_TOP, dtype=np.uint8)
    n = min(lq, ls - 3)
    for _ in range(n_queries):
        wins = [plain_window(L, q[:n], rng, a, ls - n - a) for a in (0, (ls - n) // 2, ls - n)]
        B.add_query(q, wins, [11 * n] * 3, L, rng, ls)
    return B.done()


def case_i16_limit(gap_open, targets=None, run=16):  # (run 0: four windows per query, a ragged list)
    """3c, custom matrix: true scores 29692 .. 29698 (and one far above) at about 1000 columns.  gap_open = -32 keeps the compact codes
    out (int16-pair slots: sweep_pair16_kernel<..,MULTI>), -12 admits the multi-query sweep."""
    sc = custom_scoring(gap_open=gap_open)
    L = custom_letters(sc)
    rng = np.random.default_rng(29695)
    B = Batch(run)
    lq = 1040
    for T in (targets or TARGETS_29695 + [31100]):
        q = L.compose(T, lq, rng)
        qg = L.compose(T - L.go, lq, rng, tail_top=3)
        ls = lq + 24
        wins = [plain_window(L, q, rng, 2, ls - lq - 2), plain_window(L, q, rng, ls - lq, 0)]
        B.add_query(q, wins, [T, T], L, rng, ls)
        B.add_query(qg, [gap_window(L, qg, rng, 3, ls - lq - 4, lq // 2), gap_window(L, qg, rng, ls - lq - 1, 0, 2)], [T, T], L, rng, ls)
    return sc, B.done()


def case_i16_limit_blosum(run=8):
    """3c, BLOSUM62: 2702 columns, nearly all W, 8 windows per query; true scores 29695 and 29696."""
    L = b62_letters()
    rng = np.random.default_rng(2700)
    B = Batch(run)
    for T in (29695, 29696):
        q = L.compose(T, 2702, rng)
        B.add_query(q, [plain_window(L, q, rng, 5, 35), plain_window(L, q, rng, 40, 0)], [T, T], L, rng, 2742)
    return B.done()


def case_host_gate(cols, run=8):
    """3d: smax_entry x min(max_q, max_s) = 30 x cols -- 1066 columns: 31980, the last value checkpoint mode admits; 1067: 32010, the
    first it refuses.  All-d queries: the true score IS the product.  A second query one column shorter keeps the list ragged."""
    sc = custom_scoring()
    L = custom_letters(sc)
    rng = np.random.default_rng(cols)
    B = Batch(run)
    q = np.zeros(cols, dtype=np.uint8)
    B.add_query(q, [q.copy(), q.copy()], [30 * cols] * 2, L, rng, cols)  # (windows of exactly `cols` residues: min(max_q, max_s) = cols)
    q1 = np.zeros(cols - 2, dtype=np.uint8)
    B.add_query(q1, [plain_window(L, q1, rng, 1, 1), gap_window(L, q1, rng, 1, 0, 500)], [30 * (cols - 2), 30 * (cols - 2) + L.go], L, rng, cols)
    return sc, B.done()


def case_largest_checkpoint_score(run=8):
    """3d: 31999 = 11 x 2909 is the largest product below 32000 a scheme can reach with its largest entry: 2909 tryptophans against
    themselves score exactly that, the most an int16 checkpoint pair is ever asked to hold."""
    L = b62_letters()
    rng = np.random.default_rng(31999)
    B = Batch(run)
    q = np.full(2909, B62_TOP, dtype=np.uint8)
    B.add_query(q, [plain_window(L, q, rng, 0, 0), plain_window(L, q[:2900], rng, 4, 5)], [31999, 31900], L, rng, 2909)
    return B.done()


def case_long_window(rows):
    """3d: a window of `rows` residues (65535: the last the checkpoint slots address; 65536: the first that leaves them) that holds a
    100-column query, beside ordinary windows of the same query and of two others; runs of 8."""
    L = b62_letters()
    rng = np.random.default_rng(rows)
    B = Batch(8)
    T = 777
    q = L.compose(T, 100, rng)
    long_w = plain_window(L, q, rng, rows - 100 - 4000, 4000)
    B.add_query(q, [long_w, plain_window(L, q, rng, 10, 12), plain_window(L, q[:50], rng, 10, 60)], [T, T, int(L.M[q[:50], q[:50]].sum())], L, rng, 150)
    ordinary(B, 100, 2, 3)
    return B.done()


def case_gap_field(lq=150, run=16):
    """3e: gaps directly next to the best cell (one to three columns before the alignment's end, and right after its begin) under a
    dear first gap character; with ordinary gapped homologues around them."""
    def build(sc):
        L = Letters(sc, B62_TOP, B62_MID, B62_BASE, synth.STD20)
        rng = np.random.default_rng(-sc.gap_open)
        B = Batch(run)
        ordinary(B, lq, 3, 31337)
        ls = lq + 30
        edge = np.array([B62_TOP, 2, 7, B62_TOP], dtype=np.uint8)  # W C H W = 39: dearer to drop than any of the gaps here, and not
        for T in (900, 1000):                                         # repetitive (a shift by one instead of the gap finds mismatches)
            qg = np.concatenate([edge, L.compose(T, lq - 8, rng), edge])
            Tg = int(L.M[qg, qg].sum()) + L.go
            wins = [gap_window(L, qg, rng, 3 + k, ls - lq - 4 - k, at) for k, at in enumerate((4, 4, lq - 4, lq // 2))]
            B.add_query(qg, wins, [Tg] * 4, L, rng, ls)
        return B.done()
    return build


EXTREME_NAMES = ["entries_pm100", "gaps_120_27", "open_eq_extend_1", "open_eq_extend_27", "alphabet_1", "alphabet_31", "adj_pm31", "b8_0", "b8_m1"]


# every scheme of tests/test_gpu_schemes_edges.py that lx_set_scoring must accept, by name: (matrix, gap_open, gap_extend)
def extreme_schemes():
    def m4(d, off, extra=()):
        m = np.full((4, 4), off, dtype=np.int64)
        m[np.arange(4), np.arange(4)] = d
        for (a, b, v) in extra:
            m[a, b] = m[b, a] = v
        return m
    out = {
        "entries_pm100": (m4(100, -100, [(0, 1, 37), (2, 3, -1)]), -120, -27),
        "gaps_120_27": (m4(5, -4, [(0, 1, 2)]), -120, -27),
        "open_eq_extend_1": (m4(3, -2, [(0, 1, 1)]), -1, -1),
        "open_eq_extend_27": (m4(40, -30, [(0, 1, 9)]), -27, -27),
        "alphabet_1": (np.array([[3]]), -5, -2),
        "alphabet_31": (None, -11, -1),
        # the fused step's edges: v - ge at -31 and +31; v - go at 0 (byte profiles) and at -1 (no byte profiles).  (v - go = 255 cannot
        # be reached: entries end at 100 and gap_open at -120, so the sum ends at 220.)
        "adj_pm31": (m4(29, -33, [(0, 1, 5)]), -12, -2),
        "b8_0": (m4(29, -12, [(0, 1, 4)]), -12, -2),
        "b8_m1": (m4(29, -13, [(0, 1, 4)]), -12, -2),
    }
    rng = np.random.default_rng(31)
    m31 = rng.integers(-6, 4, (31, 31))
    m31 = np.minimum(m31, m31.T)
    m31[np.arange(31), np.arange(31)] = rng.integers(2, 12, 31)
    out["alphabet_31"] = (m31, -11, -1)
    return out


def refused_v_minus_ge_32():
    """v - ge = 32: lx_set_scoring accepts it, pass 1 scores with it, pass 2 refuses it."""
    m = np.full((4, 4), -5, dtype=np.int64)
    m[np.arange(4), np.arange(4)] = 30
    return make_scoring(m, -12, -2)


CASE_NAMES = ["one_panel_16", "one_panel_32", "three_panels", "ragged_list", "i16_pairs", "i16_mq_wide", "i16_blosum", "gate_1066", "gate_1067",
              "largest", "rows_65535", "rows_65536", "family_rows", "family_mq_rows", "family_cols", "family_wide", "family_mq_wide",
              "gap_field_30", "gap_field_31", "gap_field_32"]
_ALL = {}


def join(cases):
    """Several (q, s, ext, target) of one scheme as one list (for the CPU proof of a whole family's targets)."""
    B = Batch(0)
    for q, s, ext, target in cases:
        at = len(B.target)
        B.add_batch(q, s, ext)
        B.target[at:] = target.tolist()
    return B.done()


def all_cases():
    """name -> (scheme, (q, s, ext, target)) of every input the GPU tests run with a known true score (built once per process):
    tests/test_limit_cases.py proves each target with the int32 oracle.  A family is one entry: all its members in one list."""
    if _ALL:
        return _ALL
    b = blosum62()
    out = {"one_panel_16": (b, case_codes_one_panel(16)), "one_panel_32": (b, case_codes_one_panel(32)), "three_panels": (b, case_codes_three_panels()),
           "ragged_list": (b, case_codes_ragged_list()), "i16_pairs": case_i16_limit(-32), "i16_mq_wide": case_i16_limit(-12, run=0),
           "i16_blosum": (b, case_i16_limit_blosum()), "gate_1066": case_host_gate(1066), "gate_1067": case_host_gate(1067),
           "largest": (b, case_largest_checkpoint_score()), "rows_65535": (b, case_long_window(65535)), "rows_65536": (b, case_long_window(65536))}
    for kind in ("rows", "cols"):
        out[f"family_{kind}"] = (b, join([family_member(lq, ls) for lq, ls in case_bound_family(kind)]))
    out["family_mq_rows"] = (b, join([family_member(lq, ls, run=4, n_queries=8) for lq, ls in case_bound_family("mq_rows")]))
    out["family_wide"] = (custom_scoring(gap_open=-32), join([wide_member(lq)[1] for lq in wide_family()]))
    out["family_mq_wide"] = (mq_wide_scoring(), join([mq_wide_member(ls, low)[1] for ls, low in mq_wide_family()]))
    for cost in (30, 31, 32):
        sc = capi.builtin_scoring(62, gap_open=-(cost - 1), gap_extend=-1)
        out[f"gap_field_{cost}"] = (sc, case_gap_field()(sc))
    assert sorted(out) == sorted(CASE_NAMES)
    _ALL.update(out)
    return _ALL


def mq_wide_scoring():
    """Letters 0 / 1 / 2 with diagonals 18 / 17 / 1, flank letter 3; first gap character 12, further ones 1."""
    return custom_scoring(d=18)


def mq_wide_family():
    """3b across 29695 where the flip can be seen -- the WIDE multi-query sweep, whose plan issues no int32 launch while
    max_q x largest entry + |ge| x (rows swept + 10) + (largest entry - ge) + 2 <= 29695.  Queries of 1520 columns (ten whole panels:
    the host rounds max_q to panels) of the letter that scores 18: 27360 + rows swept + 31.  Windows of 2297 residues sweep 2304 rows in
    planner and kernel alike: 29695, the last value admitted.  2298 residues: 2320 rows in the planner (29711), 2308 in the kernel
    (29699); with three 17s among the 18s the kernel's own bound is 29696, the first value it refuses.  (ls, number of 17s)."""
    return [(2265, 0), (2281, 0), (2297, 0), (2298, 3), (2298, 0), (2313, 0)]


def mq_wide_member(ls, low):
    sc = mq_wide_scoring()
    L = custom_letters(sc)
    rng = np.random.default_rng(ls * 10 + low)
    B = Batch(0)
    lq = 1520
    for k in range(2):
        q = np.zeros(lq, dtype=np.uint8)
        q[rng.choice(lq, low, replace=False)] = 1
        T = 18 * lq - low
        wins = [plain_window(L, q, rng, a, ls - lq - a) for a in (0, (ls - lq) // 2, ls - lq)] + [plain_window(L, q[:700], rng, 5, ls - 705)]
        B.add_query(q, wins, [T, T, T, int(L.M[q[:700], q[:700]].sum())])
    return sc, B.done()


def wide_family():
    """3b across 29695: all-d queries of the custom matrix (30 per column), 940 .. 970 columns: 30 x lq + rows swept + ... passes the
    16-bit integer sweeps' limit inside this range."""
    return list(range(940, 971))


def wide_member(lq, run=16):
    sc = custom_scoring(gap_open=-32)
    L = custom_letters(sc)
    rng = np.random.default_rng(lq)
    B = Batch(run)
    q = np.zeros(lq, dtype=np.uint8)
    ls = lq + 20
    for _ in range(2):
        B.add_query(q, [plain_window(L, q, rng, a, 20 - a) for a in (0, 9, 20)], [30 * lq] * 3, L, rng, ls)
    return sc, B.done()
