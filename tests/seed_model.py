"""An independent model of the reference's search() and the table of edge cases that hold both seeding paths against it
(tests/test_seed_model.py: the host path, h == NULL; tests/test_gpu_seed_edges.py: seed_reads_kernel).

model_search() restates src/search_algo.hpp:611-762 in plain Python, from the reference's text: it is no port of
host/lx_seeding.hpp or of lx_seed.hip and knows nothing of their word table -- no keys, no prefix table, no padding, no bit mask.
A cursor is the list of the (subject, position) pairs at which a word of reduced letters occurs, extendRight filters that list by
the next subject letter, and the words of a seed are looked up in a dict of every subject word of seed_length letters.  What it
takes from elsewhere is written from the reference as well: level3_cases.seed_starts (:652-663) and prefilter_cases.model
(seedLooksPromising, :426-481, which tests/test_oracle.py holds against the oracle).

Two things are not the reference's:
  * the per-read reset (:640-647) comes BEFORE the length test (:637), the project's documented departure
    (host/lx_seeding.hpp:623-626): a read's seeds must not depend on the read before it;
  * the cursors of a seed with substitutions are visited in lexicographic order of their words -- the order of
    searchHalfExactImpl's level-by-level expansion (:573-599, children appended in rank order), which the project uses for
    --seed-half-exact 0 as well (the reference's search schemes give no order the project could follow without its FM index).
The order matters: hitsThisSeq steers the elongation of the next cursor.

The `events` counter says what a run went through, so that a test can assert that it tested what it names."""
from collections import Counter, namedtuple
from functools import lru_cache

import numpy as np

from lambda_amd import capi, synth
from tests import level3_cases as L3
from tests import prefilter_cases
from tests.test_oracle import SCHEMES

_M64 = (1 << 64) - 1  # size_t arithmetic

EVENTS = ("cut_abundant", "kept_at_exactly_10x", "wanted_is_1_found_enough", "left_clamped_to_1", "elongated_beyond_key_len", "elongation_reverted",
          "elongated_to_read_end", "occurrence_dropped_at_subject_end", "window_clipped_at_start", "window_clipped_at_end", "seed_starts_on_unknown",
          "start_moved_by_run", "cursors_with_2_errors", "cursors_with_3_errors")


class Events(Counter):
    """the counter of EVENTS, and wide_reads: the first-frame ids of reads that extended a cursor of exactly key_len letters with more
    than 32 occurrences (nothing the reference knows of: it is where the device hands a read to the host)"""

    def __init__(self):
        super().__init__()
        self.wide_reads = set()


def _placement_events(ev, res, starts, seed_length, seed_offset, unknown):
    """why the starts of one frame lie where they do (:652-656)"""
    nominal = 0
    for b in starts:
        if any(res[x] != unknown and res[x] == res[x + 1] for x in range(nominal, b)):
            ev["start_moved_by_run"] += 1
        if res[b] == unknown:  # (only the last possible start: the loop of :652 stops there whatever the letter)
            ev["seed_starts_on_unknown"] += 1
        nominal = b + seed_offset


def _window_events(ev, q_len, s_len, qry_start, qry_end, subj_start, seed_length, pre_scoring):
    """whether seedLooksPromising's window is cut at a sequence start (:440-446) or end (:448-451)"""
    actual = qry_end - qry_start
    want = max(seed_length * pre_scoring, actual)
    if want <= actual:
        return
    half = (want - actual) // 2
    q, s = qry_start - half, subj_start - half
    mn = min(q, s)
    if mn < 0:
        ev["window_clipped_at_start"] += 1
        q, s, want = q - mn, s - mn, want + mn
    if min(q_len - q, s_len - s) < want:
        ev["window_clipped_at_end"] += 1


def model_search(case, params, matrix, matrix_rev=None, reads=None):
    """search() for the reads whose first frames are listed (None: all, in order; a repeated id is searched twice).
    case: a dict as level3_cases.make_case makes it; params: a capi.SeedParams; matrix[query rank][subject rank], matrix_rev for
    subjects with an odd id when given (:464-466).  Returns (matches as (qryId, subjId, qryStart, qryEnd, subjStart, subjEnd) in the
    order search() makes them, hitsAfterSeeding, hitsFailedPreExtendTest, events)."""
    sl, off, dist = int(params.seed_length), int(params.seed_offset), int(params.max_seed_dist)
    half_exact, adaptive = bool(params.half_exact), bool(params.adaptive)
    pre, thresh, max_matches = int(params.pre_scoring), float(params.pre_scoring_thresh), int(params.max_matches)
    frames, unknown = int(params.q_num_frames), int(params.unknown_rank)
    key_len = L3.key_len(case["alph"])
    ev = Events()

    def seqs(data, offs, lens):
        return [bytes(data[int(o):int(o) + int(n)]) for o, n in zip(offs, lens)]

    s_red, s_res = seqs(case["s_red"], case["s_off"], case["s_len"]), seqs(case["s_res"], case["s_off"], case["s_len"])
    q_red, q_res = seqs(case["q_red"], case["q_off"], case["q_len"]), seqs(case["q_res"], case["q_off"], case["q_len"])
    n_q = len(q_red)
    mat = np.asarray(matrix).tolist()
    mat_rev = None if matrix_rev is None else np.asarray(matrix_rev).tolist()

    # every subject word of seed_length letters that lies inside its subject, and where it occurs
    occ = {}
    for s, red in enumerate(s_red):
        for p in range(len(red) - sl + 1):
            occ.setdefault(red[p:p + sl], []).append((s, p))

    # the words of a seed: equal to it in the exact part, at most `dist` substitutions behind it.  Found by filtering the dict's words:
    # of dist + 1 pieces of the inexact part one is free of substitutions, so the candidates are the words that share a piece.
    exact = sl if dist == 0 else sl // 2 if half_exact else 0  # :664, :555
    cuts = [exact + (sl - exact) * k // (dist + 1) for k in range(dist + 2)]
    sharing = {}
    if dist:
        for w in occ:
            for k in range(dist + 1):
                sharing.setdefault((k, w[:exact], w[cuts[k]:cuts[k + 1]]), []).append(w)

    def cursors_of(seed):
        if dist == 0:
            return [(seed, 0)] if seed in occ else []
        errors = {}
        for k in range(dist + 1):
            for w in sharing.get((k, seed[:exact], seed[cuts[k]:cuts[k + 1]]), ()):
                if w not in errors:
                    errors[w] = sum(1 for a, b in zip(w, seed) if a != b)
        return sorted((w, e) for w, e in errors.items() if e <= dist)  # lexicographic in the word

    matches, after, failed = [], 0, 0
    hits = needles_sum = needles_pos = 0  # :624-626
    for read0 in (range(0, n_q, frames) if reads is None else [int(r) for r in reads]):
        for i in range(read0, min(read0 + frames, n_q)):
            if i % frames == 0:  # :640-647, before the length test (host/lx_seeding.hpp:623-626)
                hits = needles_pos = 0
                needles_sum = sum(len(q_red[j]) for j in range(i, min(i + frames, n_q)))
            L = len(q_red[i])
            if L < sl:  # :637
                continue
            starts = L3.seed_starts(q_res[i], sl, off, unknown)
            _placement_events(ev, q_res[i], starts, sl, off, unknown)
            for b in starts:
                for word, errors in cursors_of(q_red[i][b:b + sl]):
                    if errors >= 2:
                        ev["cursors_with_%d_errors" % errors] += 1
                    cur, length = occ[word], sl
                    if adaptive:  # :679-726
                        if hits >= max_matches:
                            ev["wanted_is_1_found_enough"] += 1
                            desired = 1
                        else:
                            left = ((needles_sum - needles_pos - b) & _M64) // off
                            if left < 1:
                                ev["left_clamped_to_1"] += 1
                                left = 1
                            desired = (((max_matches - hits) * 10) & _M64) // left
                        if desired == 0:
                            desired = 1
                        reached_end = True
                        while b + length < L:
                            c, new = q_red[i][b + length], []
                            for s, p in cur:
                                if p + length >= len(s_red[s]):
                                    ev["occurrence_dropped_at_subject_end"] += 1
                                elif s_red[s][p + length] == c:
                                    new.append((s, p))
                            if length == key_len and len(cur) > 32:
                                ev.wide_reads.add(read0)
                            if len(new) < desired and len(new) < len(cur):  # :714: revert the last extension
                                ev["elongation_reverted"] += 1
                                reached_end = False
                                break
                            cur, length = new, length + 1
                        if length > sl and reached_end:
                            ev["elongated_to_read_end"] += 1
                        if length > sl and length > key_len:
                            ev["elongated_beyond_key_len"] += 1
                    if len(cur) > (10 * max_matches) & _M64:  # :729
                        ev["cut_abundant"] += 1
                        continue
                    if len(cur) == 10 * max_matches:
                        ev["kept_at_exactly_10x"] += 1
                    for s, p in cur:  # :733-756
                        after += 1
                        _window_events(ev, L, len(s_res[s]), b, b + length, p, sl, pre)
                        m = mat_rev if mat_rev is not None and s & 1 else mat
                        if prefilter_cases.model(q_res[i], s_res[s], b, b + length, p, sl, pre, thresh, m):
                            matches.append((i, s, b, b + length, p, p + length))
                            hits += 1
                        else:
                            failed += 1
            needles_pos += L  # :760
    return matches, after, failed, ev


def sorted_rows(m):
    """a match list of the library (MATCH_DTYPE) or of the model as a sorted list of tuples"""
    if isinstance(m, np.ndarray):
        m = [tuple(int(x) for x in row) for row in m.tolist()]
    return sorted(m)


# ---------------------------------------------------------------------------------------------------------------------------------
# The case table.  Small on purpose: at most 65 reads and 40 subjects, a few thousand table entries.

MODES = {"protein": ("blosum62", None, 10), "translated": ("blosum62", None, 10), "nucleotide": ("nucl", None, 14), "bisulfite": ("bs_fwd", "bs_rev", 17)}
CASE_SEEDS = {"protein": 101, "translated": 102, "nucleotide": 103, "bisulfite": 104}  # (tests/test_gpu_level3.py's)

# Entry: name; inputs = the key of a builder below; kw = seeding parameters over the mode's defaults; need / absent = events the model
# must / must not report; on_device = the kernel is expected to serve every read alone (the GPU test then asserts no decline, no full
# launch and no word of key_len letters more frequent than 32); declines = "long_enough" (every read with a frame that holds a seed)
# where the case is meant to decline; some = the model must find matches; none = it must find none
Entry = namedtuple("Entry", "name inputs kw need absent on_device declines some none")


def _entry(name, inputs, kw, need=(), absent=(), on_device=True, declines=None, some=True, none=False):
    return Entry(name, inputs, kw, tuple(need), tuple(absent), on_device, declines, some and not none, none)


def _protein(rng, n):
    return synth.STD20[rng.integers(0, 20, n)].astype(np.uint8)


def _case_of(mode, subjects, reads):
    """a case dict from lists of residue arrays; reads: a flat list of frame sequences"""
    prot = mode in ("protein", "translated")
    frames = {"protein": 1, "translated": 6, "nucleotide": 2, "bisulfite": 2, "three_frames": 3}[mode]
    assert mode in ("protein", "nucleotide", "three_frames")
    red = (lambda x: L3.DNA4[x]) if mode == "nucleotide" else (lambda x: L3.LI10[x])
    s_off, s_len = L3.offsets([len(x) for x in subjects])
    q_off, q_len = L3.offsets([len(x) for x in reads])
    s_res, q_res = np.concatenate(subjects).astype(np.uint8), np.concatenate(reads).astype(np.uint8)
    return dict(mode="nucleotide" if mode == "nucleotide" else "protein", alph=4 if mode == "nucleotide" else 10, frames=frames, unknown=3 if mode == "nucleotide" else 25,
                s_res=s_res, s_red=red(s_res), s_off=s_off, s_len=s_len, q_res=q_res, q_red=red(q_res), q_off=q_off, q_len=q_len)


def identical_subjects(n, split=False):
    """Group C: n copies of one protein subject of 60 letters and three unrelated short ones (8, 10 and 17 letters: shorter than a
    seed, exactly a seed, shorter than key_len).  split: the odd copies carry other letters from position 30 on, so that a word of the
    first half occurs n times and one of the second half n / 2 times.  The reads: the subject, its [5:50], its last 10 letters, its
    first 10, a random one, and the subject's last 12 letters with 8 random ones behind them (elongation runs off the subjects' end)."""
    rng = np.random.default_rng(7)
    one, other = _protein(rng, 60), _protein(rng, 30)
    short = [_protein(rng, k) for k in (8, 10, 17)]
    for x in short:  # (their last letter and its padding must not add to the count of the copies' last word)
        x[-1] = next(y for y in synth.STD20 if L3.LI10[y] not in (L3.LI10[one[-1]], L3.LI10[other[-1]]))
    subjects = [np.concatenate([one[:30], other]) if split and k & 1 else one for k in range(n)] + short
    reads = [one, one[5:50], one[-10:], one[:10], _protein(rng, 45), np.concatenate([one[-12:], _protein(rng, 8)])]
    return _case_of("protein", subjects, reads)


def placement_case():
    """Group D: frames that isolate where seeds start (seed_length 10), each a read of its own, against the protein subjects."""
    base = L3.make_case("protein", 1, CASE_SEEDS["protein"])
    subj = [base["s_res"][int(o):int(o) + int(n)] for o, n in zip(base["s_off"], base["s_len"])]
    X, A = 25, 0
    # a subject word whose first letter reduces like the unknown letter does, so that the seed that starts on the unknown letter hits
    p = next(p for p in range(1, 40) if L3.LI10[subj[2][p]] == L3.LI10[X] and subj[2][p] != subj[2][p + 1])
    reads = [np.full(30, A, np.uint8),                                       # a homopolymer
             np.full(30, X, np.uint8),                                       # the unknown letter only
             np.concatenate([np.full(12, X, np.uint8), subj[1][:10]]),       # 12 unknown letters, then a subject's first 10
             np.concatenate([[X], subj[2][p + 1:p + 10]]).astype(np.uint8),  # exactly seed_length letters, the first unknown
             subj[4][20:31],                                                 # seed_length + 1
             subj[5][20:29],                                                 # seed_length - 1
             np.concatenate([np.full(25, subj[6][0], np.uint8), subj[6][:10]])]  # a run of 25, then a subject's first 10
    return _case_of("protein", subj, reads)


def frames_case():
    """Group E: 7 sequences at three frames per read, so the last read has one frame; lengths 9, 30, 40 | 30, 12, 6 | 50 with seeds of
    10: a first frame shorter than a seed before longer ones, and a needlesSum of its own per read.  Pieces of the protein subjects
    with a few substitutions, against those subjects and diverged copies of them."""
    base = L3.make_case("protein", 1, CASE_SEEDS["protein"])
    subj = [base["s_res"][int(o):int(o) + int(n)] for o, n in zip(base["s_off"], base["s_len"])]
    rng = np.random.default_rng(11)

    def mutated(x, rate):
        x = x.copy()
        sub = rng.random(len(x)) < rate
        x[sub] = _protein(rng, int(sub.sum()))
        return x

    # (four diverged copies of every piece the reads come from: a seed's words then occur several times and thin out letter by letter,
    # so that what the elongation keeps depends on desiredOccs -- on maxMatches, hitsThisSeq and the per-read bookkeeping)
    subj = subj[:7] + [mutated(subj[k][:70], 0.12) for k in range(7) for _ in range(4)]
    reads = []
    for k, n in enumerate((9, 30, 40, 30, 12, 6, 50)):
        reads.append(mutated(subj[k][10:10 + n], 0.05))
    return _case_of("three_frames", subj, reads)


def long_nucleotide_case():
    """Group B's longest seeds: the nucleotide set with read 3 cut to 20 letters per frame (no frame holds a seed of 48)"""
    c = dict(L3.make_case("nucleotide", 65, CASE_SEEDS["nucleotide"]))
    seqs = [c["q_res"][int(o):int(o) + int(n)] for o, n in zip(c["q_off"], c["q_len"])]
    seqs[6], seqs[7] = seqs[6][:20], seqs[7][:20]
    c["q_res"] = np.concatenate(seqs)
    c["q_red"] = L3.DNA4[c["q_res"]]
    c["q_off"], c["q_len"] = L3.offsets([len(x) for x in seqs])
    return c


def order_case():
    """Where the order of a seed's cursors shows.  Six subjects share the first 12, 14, .. 22 letters of one sequence, two more its first
    16 and 30 letters with another letter at position 7 -- in the inexact half of the read's first seed, so that seed has two cursors,
    of six and of two occurrences, which thin out as they are elongated.  With max_matches = 3 the cursor that comes first is
    elongated against desiredOccs = 3, the other one, after its hits, against a smaller one: which is which decides the matches.  The
    reads: the sequence itself and the one with the other letter."""
    rng = np.random.default_rng(13)
    one = _protein(rng, 40)
    two = one.copy()
    two[7] = next(x for x in synth.STD20 if L3.LI10[x] != L3.LI10[one[7]])
    subjects = [np.concatenate([one[:12 + 2 * k], _protein(rng, 20)]) for k in range(6)] + [np.concatenate([two[:n], _protein(rng, 20)]) for n in (16, 30)]
    return _case_of("protein", subjects, [one, two])


def declining_case():
    """tests/test_gpu_level3.py's 33 identical subjects -- a cursor elongated beyond key_len holds 33 > 32 entries, so the device hands
    its read to the host -- and, among its reads, pieces of the subject too short to be elongated to key_len, which stay with the
    device, and one that differs from the subject in its letter 14: its first seed is elongated to 14 letters and leaves matches
    before a later seed makes the read decline."""
    from tests.test_gpu_level3 import _identical_subjects

    c = dict(_identical_subjects(33))
    seqs = [c["q_res"][int(o):int(o) + int(n)] for o, n in zip(c["q_off"], c["q_len"])]
    one, late = seqs[0], seqs[0][:45].copy()
    late[14] = next(x for x in synth.STD20 if L3.LI10[x] != L3.LI10[one[14]])
    seqs = [one[:12], one, seqs[1], one[20:34], late, one[40:57], seqs[2], *seqs[3:], one[3:20]]
    c["q_res"] = np.concatenate(seqs).astype(np.uint8)
    c["q_red"] = L3.LI10[c["q_res"]]
    c["q_off"], c["q_len"] = L3.offsets([len(x) for x in seqs])
    return c


DECLINING = _entry("declining-33-copies", "declining", dict(adaptive=1, max_seed_dist=0, max_matches=10), on_device=False)
DECLINING_LATE_READ = 4  # the read that leaves matches before it declines


@lru_cache(maxsize=None)
def inputs(key):
    if key in MODES:
        return L3.make_case(key, 65, CASE_SEEDS[key])
    if key.startswith("identical"):
        _, n, split = key.split("-")
        return identical_subjects(int(n), split == "split")
    return {"placement": placement_case, "frames": frames_case, "long_nucleotide": long_nucleotide_case, "declining": declining_case, "order": order_case}[key]()


def k_max_second():
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parents[1] / "lambda_amd" / "csrc" / "lx_seed.h").read_text()
    return int(re.search(r"kMaxSecond\s*=\s*(\d+)", text).group(1))


# Group A's pre-scoring thresholds (score per letter of the window), chosen so that the model reports at least a tenth of the hits
# failing and a tenth passing in every run of the sweep -- asserted there
A_THRESH = {"protein": 5.5, "translated": 5.5, "nucleotide": 1.8, "bisulfite": 1.8}

# Group B's seed lengths are written against the table's geometry, which the tests read from the index: (what, delta)
B_LENGTHS = (("two", 0), ("prefix_len", 0), ("prefix_len", 1), ("key_len", -1), ("key_len", 0), ("key_len", 1), ("key_len", 2))


def seed_length_of(what, delta, key_len, prefix_len):
    return {"two": 2, "prefix_len": prefix_len, "key_len": key_len, "2key_len": 2 * key_len, "2kmax": 2 * k_max_second(), "abs": 0}[what] + delta


def table():
    out = []
    # ---- A: the walk's error budget, the pre-scoring window, dense and sparse seeds
    for mode in MODES:
        combos = [(2, 1), (2, 0), (3, 1)] + ([(3, 0)] if mode == "nucleotide" else [])
        for dist, half in combos:
            for pre, off in ((1, 1), (1, 7), (3, 1), (3, 7)):
                need = ["cursors_with_2_errors", "elongated_to_read_end"] + (["cursors_with_3_errors"] if dist == 3 else [])
                need += ["window_clipped_at_start", "window_clipped_at_end"] if pre == 3 else []
                out.append(_entry(f"A-{mode}-dist{dist}-half{half}-pre{pre}-off{off}", mode,
                                  dict(max_seed_dist=dist, half_exact=half, pre_scoring=pre, pre_scoring_thresh=A_THRESH[mode], seed_offset=off), need))
    # ---- B: the exact part against the table's regimes (prefix table, binary search, bit mask)
    for mode in ("protein", "nucleotide"):
        for what, delta in B_LENGTHS:
            for adaptive in (1, 0):
                if what == "two":  # words of two letters are over-abundant: let the cut fire
                    kw, need, absent = dict(max_matches=6 if mode == "protein" else 3), ["cut_abundant"], []
                else:
                    kw, need, absent = dict(max_matches=1 << 40), [], ["cut_abundant"]
                out.append(_entry(f"B-{mode}-{what}{delta:+d}-adaptive{adaptive}", mode, dict(seed_length=(what, delta), seed_offset=5, max_seed_dist=0, adaptive=adaptive, **kw),
                                  need, absent, some=not (what == "two" and not adaptive and mode == "nucleotide")))
    for delta in (0, 1):  # the exact half ends on key_len, the walk starts in the mask regime
        out.append(_entry(f"B-protein-half-exact-2key_len{delta:+d}", "protein", dict(seed_length=("2key_len", delta), seed_offset=3, max_seed_dist=1, half_exact=1)))
    out.append(_entry("B-nucleotide-half-exact-2kmax+0", "long_nucleotide", dict(seed_length=("2kmax", 0), seed_offset=3, max_seed_dist=1, half_exact=1)))
    for what, delta in (("2kmax", 1), ("abs", 63)):  # the second part exceeds kMaxSecond: the device declines every read that holds a seed
        out.append(_entry(f"B-nucleotide-half-exact-{what}{delta:+d}", "long_nucleotide", dict(seed_length=(what, delta), seed_offset=3, max_seed_dist=1, half_exact=1),
                          on_device=False, declines="long_enough"))
    # ---- C: the over-abundance cut and "found enough"
    exact = dict(max_seed_dist=0, adaptive=0, max_matches=3)
    out.append(_entry("C-30-copies-are-kept-at-max_matches-3", "identical-30-whole", exact, ["kept_at_exactly_10x"], ["cut_abundant"]))
    out.append(_entry("C-31-copies-are-cut-at-max_matches-3", "identical-31-whole", exact, ["cut_abundant"], ["kept_at_exactly_10x"], none=True))
    out.append(_entry("C-32-copies-adaptive-found-enough", "identical-32-split", dict(max_seed_dist=0, adaptive=1, max_matches=3),
                      ["wanted_is_1_found_enough", "occurrence_dropped_at_subject_end", "elongated_beyond_key_len", "cut_abundant"]))
    for mm in (1, 2):
        out.append(_entry(f"C-10-copies-max_matches-{mm}-offset-1", "identical-10-whole", dict(max_seed_dist=0, adaptive=1, max_matches=mm, seed_offset=1),
                          ["wanted_is_1_found_enough"]))
    out.append(_entry("C-30-copies-max_matches-40-offset-60", "identical-30-whole", dict(max_seed_dist=0, adaptive=1, max_matches=40, seed_offset=60), ["left_clamped_to_1"]))
    out.append(_entry("C-order-of-the-cursors-of-a-seed", "order", dict(max_seed_dist=1, half_exact=1, adaptive=1, max_matches=3, seed_offset=5),
                      ["wanted_is_1_found_enough", "elongation_reverted"]))
    out.append(_entry("C-order-of-the-cursors-of-a-seed-two-errors", "order", dict(max_seed_dist=2, half_exact=0, adaptive=1, max_matches=3, seed_offset=5),
                      ["wanted_is_1_found_enough", "elongation_reverted"]))
    # ---- D: where seeds start
    for off in (1, 5, 60):
        out.append(_entry(f"D-placement-offset-{off}", "placement", dict(seed_offset=off, max_seed_dist=0), ["seed_starts_on_unknown", "start_moved_by_run"]))
        out.append(_entry(f"D-placement-offset-{off}-one-error", "placement", dict(seed_offset=off, max_seed_dist=1, half_exact=1), ["seed_starts_on_unknown", "start_moved_by_run"]))
    # ---- E: frames of unequal length, a last read with fewer frames
    for mm in (256, 2, 5):
        for off in (5, 3):
            out.append(_entry(f"E-frames-max_matches-{mm}-offset-{off}", "frames", dict(max_matches=mm, seed_offset=off, max_seed_dist=1, half_exact=1, q_num_frames=3)))
    return out


TABLE = table()
BY_NAME = {e.name: e for e in TABLE}


def params_of(entry, key_len, prefix_len):
    """the entry's capi.SeedParams (the mode's real schemes) and its two matrices"""
    c = inputs(entry.inputs)
    fwd, rev, sl = MODES[c["mode"]]
    kw = dict(seed_length=sl, seed_offset=max(3, sl // 2), max_seed_dist=1, q_num_frames=c["frames"], unknown_rank=c["unknown"], max_matches=256)
    kw.update(entry.kw)
    if isinstance(kw["seed_length"], tuple):
        kw["seed_length"] = seed_length_of(*kw["seed_length"], key_len, prefix_len)
    m, mr = SCHEMES[fwd].matrix_np(), None if rev is None else SCHEMES[rev].matrix_np()
    return capi.seed_params(m, matrix_rev=mr, **kw), m, mr


_models = {}


def expected(entry, key_len, prefix_len, reads=None):
    """model_search for a table entry, computed once per process"""
    key = (entry.name, key_len, prefix_len, None if reads is None else tuple(int(r) for r in reads))
    if key not in _models:
        p, m, mr = params_of(entry, key_len, prefix_len)
        matches, after, failed, ev = model_search(inputs(entry.inputs), p, m, mr, reads=reads)
        _models[key] = (sorted_rows(matches), after, failed, ev)
    return _models[key]


def long_enough(c, seed_length):
    """how many reads have a frame that holds a seed"""
    n_q, fr = len(c["q_len"]), c["frames"]
    return sum(1 for i in range(0, n_q, fr) if any(int(c["q_len"][j]) >= seed_length for j in range(i, min(i + fr, n_q))))


def check_entry(entry, ev, n_matches, after, failed):
    """what an entry asserts of the model's own run: the events it names, matches where it expects some"""
    for name in entry.need:
        assert ev[name] > 0, (entry.name, name, dict(ev))
    for name in entry.absent:
        assert ev[name] == 0, (entry.name, name, ev[name])
    assert not entry.some or n_matches > 0, entry.name
    assert not entry.none or n_matches == 0, (entry.name, n_matches)
    if entry.name.startswith("A-"):
        assert after >= 100 and 0.1 * after <= failed <= 0.9 * after, (entry.name, after, failed)
