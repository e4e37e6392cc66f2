"""The free-packing plan of the multi-query sweep, SEQUENTIALLY and without the library: the rules of lambda_amd/csrc/lx_plan_free.hip's
header and DESIGN.md 4.6 restated with Python loops and `sorted` -- no scans, no radix passes, no inverse permutations, no slot
arithmetic: wavefronts are lists that are appended to and closed.  tests/test_plan_model.py holds the model against the plan's promises
(tests.test_gpu_plan.check_plan) and asserts on it that every case below meets the condition it was made for;
tests/test_gpu_plan_edges.py holds the device's plan against the model, word for word.

The case lists live here so that both files read the same ones: every list sits on one of the kernels' own constants -- the run cut
at 512 list positions, shares of 64 runs, quads of four and eight pairs per wavefront, the med +- slack thresholds, the coarse regions
of the 16-bit sort key, the scan and sort tiles."""
import zlib

import numpy as np

EXT_DTYPE = np.dtype([("q_off", "<u8"), ("s_off", "<u8"), ("q_len", "<u4"), ("s_len", "<u4")])  # lx_extension (include/lambda_ext.h)

RUN_CUT = 512   # a run is cut at every multiple of this many list positions
SHARE = 64      # sorted runs per share of the stream's closing rule
FILLER = 0x80000000


def cols_per_lane(lq, C):
    """Columns per lane of a query of lq letters swept in strips of C columns: whole panels of 8 C letters, and for the rest the
    narrowest strip (a quarter, a half, three quarters of C, rounded up, or C) whose panel covers it."""
    panel = 8 * C
    P = max(1, -(-lq // panel))
    rem = max(lq, 1) - (P - 1) * panel
    last = next(w for w in ((C + 3) // 4, (C + 1) // 2, (3 * C + 3) // 4, C) if rem <= 8 * w)
    return min(0xfff, (P - 1) * C + last)


def key16(pan, length):
    """Widest first, longest first: lengths in steps of 8 below 1024, of 64 from there, saturating; columns per lane up to 255."""
    lc = length >> 3 if length < 1024 else 128 + min(127, (length - 1024) >> 6)
    return ((255 - min(pan, 255)) << 8) | (255 - lc)


class Run:
    """One run of the list: its windows longest first, what of them is pooled, what is streamed."""

    def __init__(self, rng, order, s_len, pan):
        c = len(order)
        med = s_len[order[c // 2]]
        slack = max(8, med // 8)
        nlong = sum(1 for i in order if s_len[i] > med + slack)
        nshort = sum(1 for i in order if s_len[i] < med - slack) if med > slack else 0
        phi = min(c, -(-nlong // 4) * 4)
        plo = min(c - phi, -(-nshort // 4) * 4)
        self.range, self.order, self.c, self.med, self.slack, self.phi, self.plo, self.pan = rng, order, c, med, slack, phi, plo, pan
        long_, short = order[:phi], order[c - plo:]
        self.quads = [long_[k: k + 4] for k in range(0, phi, 4)] + [short[k: k + 4] for k in range(0, plo, 4)]
        stream = order[phi: c - plo]
        self.pairs = [stream[k: k + 2] for k in range(0, len(stream), 2)]
        self.key = (rng, key16(pan, s_len[stream[0]]) if stream else key16(pan, 0) | 0xff)


class Plan:
    pass


def plan_model(ext, cuts, C=19):
    """The plan of the window list `ext` (EXT_DTYPE) in the ranges [cuts[r], cuts[r + 1]) for strips of C columns.  Returns an object
    with plan [nwf, 16] (uint32, bit 31 on fillers), wf_pan, wf_maxs, nruns, nquads, range_wf (first wavefront of every range, then
    nwf) -- what the device reports -- and, for the cases' own assertions, runs (Run objects in list order), quads ((key, windows) in
    list order), and per wavefront `kind` ('pool' / 'stream'), `closed` (why a stream wavefront ended: 'full', 'fifth', 'share') and
    `nruns_in` (the runs that have a pair in a stream wavefront, the quads of a pool wavefront)."""
    n = len(ext)
    q_off, q_len, s_len = (ext[f].tolist() for f in ("q_off", "q_len", "s_len"))
    nranges = len(cuts) - 1
    range_of = lambda i: max(r for r in range(nranges) if i >= cuts[r])
    heads = [i for i in range(n) if i == 0 or i % RUN_CUT == 0 or (q_off[i], q_len[i]) != (q_off[i - 1], q_len[i - 1])]
    runs = []
    for a, b in zip(heads, heads[1:] + [n]):
        order = sorted(range(a, b), key=lambda i: -s_len[i])  # (sorted is stable: ties stay in list order)
        runs.append(Run(range_of(a), order, s_len, cols_per_lane(q_len[a], C)))
    quads = [((run.range, key16(run.pan, s_len[q[0]])), q) for run in runs for q in run.quads]

    wavefronts, kind, closed, nruns_in, range_wf = [], [], [], [], []
    for r in range(nranges):
        range_wf.append(len(wavefronts))
        # pool: the range's quads by key, four to a wavefront (a quad takes four slots whatever it holds)
        mine = sorted((q for q in quads if q[0][0] == r), key=lambda q: q[0])
        for k in range(0, len(mine), 4):
            slots = [None] * 16
            for j, (_, q) in enumerate(mine[k: k + 4]):
                slots[4 * j: 4 * j + len(q)] = q
            wavefronts.append(slots)
            kind.append("pool")
            closed.append(None)
            nruns_in.append(len(mine[k: k + 4]))
        # stream: the range's runs by key, in shares; a wavefront closes at eight pairs or before a fifth run
        order = sorted((run for run in runs if run.range == r), key=lambda run: run.key)
        for s0 in range(0, len(order), SHARE):
            cur, cur_runs = None, 0  # the open wavefront (a list of pairs) and the runs in it

            def close(why):
                slots = [None] * 16
                for j, p in enumerate(cur):
                    slots[2 * j: 2 * j + len(p)] = p
                wavefronts.append(slots)
                kind.append("stream")
                closed.append(why)
                nruns_in.append(cur_runs)

            for run in order[s0: s0 + SHARE]:
                if not run.pairs:
                    continue
                if cur is not None and len(cur) == 8:
                    close("full")
                    cur = None
                elif cur is not None and cur_runs == 4:
                    close("fifth")
                    cur = None
                if cur is None:
                    cur, cur_runs = [], 0
                cur_runs += 1
                for p in run.pairs:
                    if len(cur) == 8:
                        close("full")
                        cur, cur_runs = [], 1  # (the run that crosses is the new wavefront's first)
                    cur.append(p)
            if cur is not None:
                close("share")
    range_wf.append(len(wavefronts))

    nwf = len(wavefronts)
    plan = np.zeros((nwf, 16), np.uint32)
    wf_pan, wf_maxs = np.zeros(nwf, np.uint32), np.zeros(nwf, np.uint32)
    for w, slots in enumerate(wavefronts):
        last = None
        for k, x in enumerate(slots):
            if x is None:
                plan[w, k] = last | FILLER  # (a wavefront's first slot is never empty: `last` is a window here)
            else:
                plan[w, k] = last = x
        wf_pan[w] = max(cols_per_lane(q_len[x], C) for x in slots if x is not None)
        wf_maxs[w] = max(s_len[x] for x in slots if x is not None)
    m = Plan()
    m.plan, m.wf_pan, m.wf_maxs, m.nruns, m.nquads, m.range_wf = plan, wf_pan, wf_maxs, len(runs), len(quads), range_wf
    m.runs, m.quads, m.kind, m.closed, m.nruns_in, m.nwf = runs, quads, kind, closed, nruns_in, nwf
    return m


def report_of(m, nranges):
    """The sixteen words the device reports for the model's plan (the words behind [4 + nranges] are not the plan's)."""
    return [m.nwf, 0, m.nruns, m.nquads] + list(m.range_wf[: nranges + 1])


# ---- the case lists -------------------------------------------------------------------------------------------------------------

def make_ext(queries):
    """queries: [(q_len, [s_len, ...]), ...] -> the list, grouped by query as the Level-2 driver leaves it (q_off: the queries
    concatenated; s_off: anything)."""
    rows, q_off, i = [], 0, 0
    for lq, lens in queries:
        for ls in lens:
            rows.append((q_off, 1000003 * i % (1 << 24), lq, ls))
            i += 1
        q_off += lq
    return np.array(rows, dtype=EXT_DTYPE)


def scrambled(lens, seed):
    """The same windows in another list order (fixed by the seed)."""
    lens = list(lens)
    return [lens[i] for i in np.random.default_rng(seed).permutation(len(lens))]


def query_cuts(ext, at_queries):
    """Range cuts in front of the given queries (counted in list order)."""
    heads = [0] + (np.nonzero(ext["q_off"][1:] != ext["q_off"][:-1])[0] + 1).tolist()
    return [0] + [heads[k] for k in at_queries] + [len(ext)]


class Case:
    """A list, its ranges, the strip widths it is planned for, the number of its queries, and `expect`: the condition the list was
    made for, asserted on the model's plan (for C = Cs[0])."""

    def __init__(self, queries, expect, cut_queries=(), Cs=(19,)):
        self.ext = queries if isinstance(queries, np.ndarray) else make_ext(queries)
        self.n = len(self.ext)
        self.cuts = query_cuts(self.ext, cut_queries)  # (ranges begin where the query changes)
        self.Cs = Cs
        self.n_qseq = len(set(self.ext["q_off"].tolist()))
        self.expect = expect


CASES = {}


def case(f):
    CASES[f.__name__] = f
    return f


def _distinct(c):
    return [150 + 389 * i % c for i in range(c)]  # (389 is prime to every c below: a permutation of 150 .. 150 + c - 1)


# ---- the run cut at 512 list positions

def _one_query(c, distinct):
    def expect(m):
        assert m.nruns == -(-c // RUN_CUT) and [run.c for run in m.runs] == [min(RUN_CUT, c - a) for a in range(0, c, RUN_CUT)]
        if not distinct:
            # nothing is pooled; a full run of 512 fills 32 wavefronts, the next run begins one of its own
            assert m.nquads == 0 and m.nwf == sum(-(-run.c // 16) for run in m.runs)
        else:
            assert m.nquads > 0 and all(run.phi and run.plo for run in m.runs if run.c > 16)
    return lambda: Case([(150, _distinct(c) if distinct else [176] * c)], expect)


for _c in (511, 512, 513, 1024, 1025):
    CASES[f"run_cut_{_c}_equal"] = _one_query(_c, False)
    CASES[f"run_cut_{_c}_distinct"] = _one_query(_c, True)


def _a500_b30(front):
    def expect(m):
        assert [run.c for run in m.runs][-3:] == [500, 12, 18] and min(m.runs[-1].order) % RUN_CUT == 0
        assert m.runs[-2].range == m.runs[-1].range == (1 if front else 0)
    a, b = scrambled([176] * 450 + [400] * 20 + [60] * 30, 1), scrambled([180] * 24 + [90] * 3 + [500] * 3, 2)
    qs = ([(120, scrambled([140] * 6 + [300, 50], k)) for k in range(64)] if front else []) + [(150, a), (157, b)]
    return lambda: Case(qs, expect, cut_queries=[64] if front else [])


CASES["run_cut_500_of_a_30_of_b"] = _a500_b30(False)
CASES["run_cut_500_of_a_30_of_b_behind_a_range"] = _a500_b30(True)


# ---- ties: the rank follows list order, quads and runs that tie in key keep run order

@case
def ties_all_equal():
    def expect(m):
        assert len({run.key for run in m.runs}) == 1 and m.nquads == 0 and m.nruns == 12
    return Case([(150, [176] * c) for c in (6, 1, 7, 6, 3, 16, 2, 5, 6, 9, 6, 4)], expect)


@case
def ties_two_lengths_interleaved():
    def expect(m):
        # every run pools its 200s and 201s: quads that tie in key16 and differ in their first window's length, in every run alike
        keys = [k for k, _ in m.quads]
        assert len(set(keys)) == 1 and len(keys) >= 8 and {int(ext["s_len"][q[0]]) for _, q in m.quads} == {200, 201}
    ext = make_ext([(150, [201 if i % 4 == 0 else 200 if i % 4 == 2 else 150 for i in range(c)]) for c in (40, 40, 24, 40)])
    return Case(ext, expect)


@case
def ties_two_lengths_no_pool():
    def expect(m):
        assert m.nquads == 0 and len({run.key for run in m.runs}) == 1
    return Case([(150, [176 if i % 2 else 180 for i in range(c)]) for c in (10, 3, 6, 7, 10, 1)], expect)


# ---- the thresholds med +- slack

def _nine(med, hi, lo, seed):
    return scrambled([hi] + [med] * 7 + [lo], seed)


def _thresholds(med):
    slack = max(8, med // 8)
    combos = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (the longest window is beyond med + slack, the shortest beyond med - slack)

    def expect(m):
        assert [run.med for run in m.runs] == [med] * 4 and [run.slack for run in m.runs] == [slack] * 4
        assert [(run.phi, run.plo) for run in m.runs] == [(4 * a, 4 * b) for a, b in combos]
    return lambda: Case([(150 + k, _nine(med, med + slack + a, med - slack - b, 10 * med + k)) for k, (a, b) in enumerate(combos)], expect)


for _med in (63, 64, 65, 72, 800):
    CASES[f"thresholds_med_{_med}"] = _thresholds(_med)


@case
def thresholds_gate_med_8_and_9():
    def expect(m):
        # med 8: slack 8, med > slack fails (and med - slack - 1 would wrap); med 9: the bound is 1 row, no window is shorter
        # (a window of no rows -- nothing the planner makes, plain integer work for the plan -- is the one thing shorter than 1 row:
        # pooled beside a median of 9, not beside a median of 8)
        assert [(run.med, run.slack) for run in m.runs] == [(8, 8)] * 4 + [(9, 8)] * 4
        assert [(run.phi, run.plo) for run in m.runs] == [(0, 0), (4, 0), (0, 0), (0, 0), (0, 0), (4, 0), (0, 0), (0, 4)]
    return Case([(150, _nine(8, 16, 1, 1)), (151, _nine(8, 17, 1, 2)), (152, _nine(8, 8, 1, 3)), (153, _nine(8, 8, 0, 7)),
                 (154, _nine(9, 17, 1, 4)), (155, _nine(9, 18, 1, 5)), (156, _nine(9, 9, 1, 6)), (157, _nine(9, 9, 0, 8))], expect)


@case
def thresholds_windows_of_1_to_8_rows():
    def expect(m):
        assert all(run.med <= 8 and run.plo == 0 for run in m.runs) and m.nquads == 0
    rng = np.random.default_rng(18)
    return Case([(40 + k, rng.integers(1, 9, size=c).tolist()) for k, c in enumerate((9, 16, 1, 2, 33, 5, 8, 12))], expect)


# ---- partly filled quads

def _partly(kind):
    nl, S = (1, []) if kind == "long" else (0, [60]) if kind == "short" else (1, [60])

    def runs_of(k):
        return [(150, scrambled([400 + 8 * (k + c)] * nl + [176] * (c - nl - len(S)) + S, 7 * k + c)) for c in (2, 3, 5, 6, 7)]

    def expect(m):
        sizes = sorted({len(q) for _, q in m.quads})
        assert sizes == {"long": [2, 3, 4], "short": [2, 3, 4], "both": [1, 2, 3, 4]}[kind], sizes
        if kind == "both":
            five = m.runs[2]
            assert (five.c, five.phi, five.plo, len(five.pairs)) == (5, 4, 1, 0)  # (400/176/176/176/60: two quads, no pair)
    return lambda: Case([q for k in range(3) for q in runs_of(k)], expect)


for _kind in ("long", "short", "both"):
    CASES[f"partly_filled_quads_{_kind}"] = _partly(_kind)


@case
def pool_only_run_between_streamed_runs():
    def expect(m):
        pooled = [run for run in m.runs if not run.pairs]
        assert [(run.c, run.phi) for run in pooled] == [(3, 3), (4, 4)]
        order = sorted(m.runs, key=lambda run: run.key)
        at = [order.index(run) for run in pooled]
        # behind the streamed runs of its width, in front of the narrower ones
        assert all(order[k].pan == pooled[0].pan and order[k].pairs for k in range(min(at)))
        assert all(order[k].pan < pooled[0].pan for k in range(max(at) + 1, len(order))) and max(at) + 1 < len(order)
    return Case([(150, [176] * 6), (150, [176, 400, 176]), (150, [60] * 6), (100, [120] * 5), (150, [500, 176, 500, 176]), (150, [176] * 3),
                 (60, [80] * 4)], expect)


# ---- the closing rule: eight pairs, or before a fifth run; shares of 64 runs

def _singles(nq):
    def expect(m):
        full, rest = divmod(nq, SHARE)
        assert m.nruns == nq and m.nquads == 0 and m.nwf == 16 * full + -(-rest // 4)
        assert m.closed.count("share") == full + (rest > 0) and "full" not in m.closed
    return lambda: Case([(150, [176])] * nq, expect)


for _nq in (4, 5, 63, 64, 65, 128, 129):
    CASES[f"closing_{_nq}_one_window_queries"] = _singles(_nq)


@case
def closing_sixteen_then_four_runs_then_a_fifth():
    def expect(m):
        assert m.closed == ["full", "fifth", "share"] and m.nruns_in == [1, 4, 1]
    return Case([(150, [176] * 16)] + [(150, [176, 176])] * 5, expect)


@case
def closing_seventeen_crosses_then_three_runs_then_a_fifth():
    def expect(m):
        # the crossing run is the second wavefront's first run: it closes before the fifth run, at four pairs
        assert m.closed == ["full", "fifth", "share"] and m.nruns_in == [1, 4, 1]
        assert ((m.plan[1] & FILLER) == 0).sum() == 1 + 3 * 2
    return Case([(150, [176] * 17)] + [(150, [176, 176])] * 4, expect)


@case
def closing_eighth_pair_by_the_fourth_run():
    def expect(m):
        assert m.closed == ["full", "full", "fifth", "share"] and m.nruns_in == [4, 4, 4, 1]
    return Case([(150, [176] * 4)] * 4 + [(150, [176] * c) for c in (6, 4, 4, 2)] + [(150, [176] * c) for c in (2, 3, 1, 2)] + [(150, [176] * 5)], expect)


@case
def closing_two_runs_of_one_query_count_twice():
    def expect(m):
        # query A stands at list positions 508 .. 515: two runs of four.  The rule counts runs, not queries: the wavefront of A's two
        # runs, B and C closes before D -- with three queries and six pairs
        assert [run.c for run in m.runs] == [508, 4, 4, 2, 2, 2, 2] and m.runs[1].pan > m.runs[0].pan
        k = m.kind.index("stream")
        assert (m.closed[k], m.nruns_in[k]) == ("fifth", 4) and m.plan[k].tolist() == list(range(508, 520)) + [519 | FILLER] * 4
        assert len(set(ext["q_off"][m.plan[k] & ~np.uint32(FILLER)].tolist())) == 3
    ext = make_ext([(100, [120] * 508), (150, [176] * 8), (150, [176] * 2), (150, [176] * 2), (150, [176] * 2), (150, [176] * 2)])
    return Case(ext, expect)


# ---- the regions of the 16-bit key

KEY_LENGTHS = (1016, 1023, 1024, 1087, 1088, 9151, 9152, 20000)


@case
def key_regions_of_the_length():
    def expect(m):
        by_len = {int(ext["s_len"][run.order[0]]): run.key[1] & 0xff for run in m.runs}
        assert [255 - by_len[l] for l in KEY_LENGTHS] == [127, 127, 128, 128, 129, 254, 255, 255]
    ext = make_ext([(150, [l]) for l in scrambled(KEY_LENGTHS + (1000, 1100, 5000), 3)])
    return Case(ext, expect)


def wide_query_lengths(C):
    """Query lengths at which the columns per lane pass 255: the first and the last length of every width from 250 to 262."""
    first, last = {}, {}
    for lq in range(1, 4096):
        w = cols_per_lane(lq, C)
        if 250 <= w <= 262:
            first.setdefault(w, lq)
            last[w] = lq
    return sorted(set(first.values()) | set(last.values()))


def _key_regions_width(C):
    lqs = wide_query_lengths(C)

    def expect(m):
        widths = [cols_per_lane(lq, C) for lq in lqs]
        assert min(widths) < 255 < max(widths) and sum(w > 255 for w in widths) >= 2 and sum(w < 255 for w in widths) >= 2
        assert {run.key[1] >> 8 for run in m.runs if run.pan >= 255} == {0} and len({run.pan for run in m.runs if run.pan >= 255}) >= 2
    return lambda: Case([(lq, scrambled([lq + 30] * (1 + k % 3) + ([3 * lq] if k % 4 == 1 else []), k)) for k, lq in enumerate(scrambled(lqs, C))], expect, Cs=(C,))


for _C in (19, 13, 11):
    CASES[f"key_regions_of_the_width_C{_C}"] = _key_regions_width(_C)


# ---- ranges

def _range_segments():
    rng = np.random.default_rng(8)

    def mixed(nq):
        out = []
        for _ in range(nq):
            lq = int(rng.integers(40, 700))
            base = lq + 2 * (int(np.sqrt(lq)) + 1)
            out.append((lq, [max(1, int(base * (rng.uniform(1.2, 3.0) if u < 0.1 else rng.uniform(0.1, 0.9) if u < 0.2 else 1.0)) - int(rng.integers(0, 4)))
                             for u in rng.random(int(1 + rng.poisson(7)))]))
        return out
    return [mixed(30), [(150, [176])], [(150, [400 + 8 * k, 176, 176]) for k in range(9)], [(150, [176] * c) for c in (16, 3, 6, 1, 1, 1, 9)],
            mixed(10), mixed(70), [(90, [100])], mixed(25)]


def _ranges(nranges):
    segs = _range_segments()
    first_query = np.cumsum([0] + [len(s) for s in segs]).tolist()

    def expect(m):
        if nranges == 8:
            per = [m.kind[a: b] for a, b in zip(m.range_wf, m.range_wf[1:])]
            assert per[1] == ["stream"] and per[6] == ["stream"] and set(per[2]) == {"pool"} and set(per[3]) == {"stream"}
            assert all("pool" in p and "stream" in p for p in (per[0], per[4], per[5], per[7]))
        assert len(m.range_wf) == nranges + 1
    at = {1: [], 2: [first_query[4]], 8: first_query[1:8]}[nranges]
    return lambda: Case([q for s in segs for q in s], expect, cut_queries=at, Cs=(19, 13, 11))


for _r in (1, 2, 8):
    CASES[f"ranges_{_r}"] = _ranges(_r)


# ---- the tiles of the scans (2048) and of the sorts (4096), many shares

def _tiles(nq):
    def expect(m):
        assert m.nruns == nq and m.nquads == 0 and m.closed.count("share") == -(-nq // SHARE)
    rng = np.random.default_rng(nq)
    lqs, lens = rng.integers(30, 1200, size=nq).tolist(), rng.integers(20, 1500, size=nq).tolist()
    return lambda: Case(list(zip(lqs, ([l] for l in lens))), expect)


for _nq in (2047, 2048, 2049, 4095, 4096, 4097):
    CASES[f"tiles_{_nq}_one_window_queries"] = _tiles(_nq)


@case
def tiles_2049_quads():
    def expect(m):
        assert m.nquads == 2049 and m.nruns == 2049 and m.kind.count("pool") == 513
    rng = np.random.default_rng(2049)
    # (two windows per query, one of them long: every run is one quad of two, and no run is cut at a multiple of 512)
    return Case([(int(lq), scrambled([int(l), 176], k)) for k, (lq, l) in enumerate(zip(rng.integers(100, 400, size=2049), rng.integers(300, 1400, size=2049)))], expect)


# ---- ordinary lists: the five of tests/test_gpu_plan.py at a tenth of their size

def _ordinary(name):
    def make():
        from tests.test_gpu_plan import CASES as ORDINARY, make_list
        nq, windows, qlen, merged = ORDINARY[name]
        if name == "a_query_with_thousands":
            windows = lambda r: 300 if r.random() < 0.1 else 5  # (a tenth of the windows: a tenth of the queries would be four)
        else:
            nq = max(1, nq // 10)
        ext = make_list(np.random.default_rng(zlib.crc32(name.encode())), nq, windows, qlen, merged)

        def expect(m):
            assert m.nwf > 0 and (name == "single_window" or (m.nquads > 0 and "stream" in m.kind))
            assert name != "a_query_with_thousands" or max(run.c for run in m.runs) >= 200
        return Case(ext.astype(EXT_DTYPE), expect)
    return make


for _name in ("headline_32_windows_of_150", "a_dozen_windows_ragged", "one_or_two_windows", "a_query_with_thousands", "single_window"):
    CASES[f"ordinary_{_name}"] = _ordinary(_name)


_made = {}


def get_case(name):
    """The case, made once (the lists are shared by the tests and left unchanged)."""
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


_planned = {}


def model_of(name, C):
    if (name, C) not in _planned:
        c = get_case(name)
        _planned[name, C] = plan_model(c.ext, c.cuts, C)
    return _planned[name, C]
