"""The pre-extension filter's yardstick and its edge cases, shared by tests/test_oracle.py (the oracle's lxo_seed_looks_promising) and
tests/test_gpu_prefilter.py (lx_prefilter_batch, lx_prefilter.hip).

model() is a restatement of seedLooksPromising written from the reference's text (src/search_algo.hpp:426-481) alone, in Python
integers with the reference's uint64_t / int64_t conversions spelled out; it shares no code with the oracle or the kernel, which are
line for line the same as each other.  cases() is a table of small (q, s, seed, seed_length, pre_scoring, thresh, scheme) inputs, each
aimed at one line of the kernel; where the answer follows from a few additions it is written down by hand (`expect`), and the tests
check the model against it as well."""
from collections import namedtuple

import numpy as np

from tests.test_oracle import SCHEMES

_M64 = (1 << 64) - 1


def _u64(x: int) -> int:
    return x & _M64


def _i64(x: int) -> int:
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def model(q, s, qry_start, qry_end, subj_start, seed_length, pre_scoring, thresh, matrix) -> bool:
    """seedLooksPromising (src/search_algo.hpp:426-481).  q, s: the whole (frame) sequences as ranks; matrix[query rank][subject rank]."""
    eff_q = _i64(qry_start)                                      # :429  int64_t  effectiveQBegin = m.qryStart
    eff_s = _i64(subj_start)                                     # :430  int64_t  effectiveSBegin = m.subjStart
    actual = _u64(qry_end - qry_start)                           # :431  uint64_t actualLength
    eff_len = max(_u64(seed_length * pre_scoring), actual)       # :432-433  static_cast<uint64_t>(size_t * int32_t), std::max
    if eff_len > actual:                                         # :435
        half = _u64(eff_len - actual) // 2
        eff_q = _i64(_u64(eff_q) - half)                         # :437  int64_t -= uint64_t: computed unsigned, stored signed
        eff_s = _i64(_u64(eff_s) - half)                         # :438
        mn = min(eff_q, eff_s)                                   # :440
        if mn < 0:                                               # :441
            eff_q = _i64(eff_q - mn)                             # :443
            eff_s = _i64(eff_s - mn)                             # :444
            eff_len = _u64(eff_len + mn)                         # :445  uint64_t += int64_t (negative: wraps to a subtraction)
        eff_len = min(_u64(len(q) - eff_q), _u64(len(s) - eff_s), eff_len)  # :448-451
    score = best = 0                                             # :459-460
    limit = int(thresh * eff_len)                                # :461  int = double * uint64_t: truncated towards zero
    for i in range(eff_len):                                     # :468
        score += int(matrix[int(q[eff_q + i])][int(s[eff_s + i])])  # :470
        if score < 0:                                            # :472
            score = 0
        elif score > best:                                       # :474
            best = score
        if best >= limit:                                        # :477
            return True
    return False                                                 # :480


Case = namedtuple("Case", "group name q s qry_start qry_end subj_start seed_length pre_scoring thresh scheme slot expect")

PROT = "ABCDEFGHIJKLMNOPQRSTUVWYZX*"  # the ranks of the BLOSUM tables


def matrix_of(scheme: str):
    return SCHEMES[scheme].matrix_np()


def _diagonal(rng, q_len, s_len, diag, spans, fill="x", alphabet=4):
    """A query of q_len random ranks below `alphabet` and a subject of s_len such that cell (i, i + diag) is an identity where the
    pattern says 'm' and a mismatch where it says 'x'.  spans: (first query index, pattern) pieces; `fill` everywhere else on the
    diagonal.  Subject positions off the diagonal's reach are random."""
    q = rng.integers(0, alphabet, q_len).astype(np.uint8)
    s = rng.integers(0, alphabet, s_len).astype(np.uint8)
    pat = [fill] * q_len
    for at, p in spans:
        pat[at:at + len(p)] = list(p)
    assert len(pat) == q_len
    for i in range(q_len):
        j = i + diag
        if 0 <= j < s_len:
            s[j] = q[i] if pat[i] == "m" else (q[i] + 1 + rng.integers(0, alphabet - 1)) % alphabet
    return q, s


def cases():
    """The table.  Scheme `nucl` is +2 / -3, so a region of L identities scores 2 L, a mismatch after k >= 2 identities leaves 2 k - 3."""
    rng = np.random.default_rng(20240607)
    out = []

    def add(group, name, q, s, qs, qe, ss, sl, pre, thr, scheme="nucl", slot=0, expect=None):
        assert 0 <= qs <= qe <= len(q) and ss + (qe - qs) <= len(s), name  # what lx_prefilter_batch accepts
        out.append(Case(group, name, np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(s, np.uint8), qs, qe, ss, sl, pre, thr, scheme, slot, expect))

    def nucl(group, name, q_len, s_len, qs, qe, ss, sl, pre, thr, spans, fill="x", expect=None):
        q, s = _diagonal(rng, q_len, s_len, ss - qs, spans, fill)
        add(group, name, q, s, qs, qe, ss, sl, pre, thr, expect=expect)

    # ---- clip at the starts: region 20, seed 10, so the begins move back by 5; the smaller one goes below 0 and both are shifted up
    # by it while effLen shrinks (the `mn < 0` branch, lx_prefilter.hip:36-42).  The region [first, first + effLen) of identities just
    # reaches 2.0 * effLen; the cells behind it are mismatches, so an effLen left at 20 (limit 40) would drop the keep cases.
    for qs, ss in ((2, 7), (4, 1), (0, 5), (5, 0), (0, 3), (3, 4), (1, 0)):
        mn = min(qs - 5, ss - 5)
        first, eff = qs - 5 - mn, 20 + mn  # the first query index of the clipped region, its length
        nucl("clip at the starts", f"qs {qs} ss {ss} keep: effQ -= mn, effS -= mn, effLen += mn", 60, 80, qs, qs + 10, ss, 10, 2, 2.0, [(first, "m" * eff)], expect=True)
        nucl("clip at the starts", f"qs {qs} ss {ss} drop: the region's first cell (query {first}) is a mismatch", 60, 80, qs, qs + 10, ss, 10, 2, 2.0,
             [(first, "x" + "m" * (eff - 1))], fill="m", expect=False)
    # an odd surplus: a seed of 9 in a region of 20 moves the begins back by 11 / 2 = 5, not 6 (lx_prefilter.hip:34-35), no clip
    nucl("clip at the starts", "seed of 9, surplus 11: the region starts 5 before the seed, keep", 60, 80, 30, 39, 40, 10, 2, 2.0, [(25, "m" * 20)], expect=True)
    nucl("clip at the starts", "seed of 9, surplus 11, drop: query 25, the region's first cell", 60, 80, 30, 39, 40, 10, 2, 2.0, [(25, "x")], fill="m", expect=False)
    # both clips at once on sequences shorter than the region: 30 wanted, begins -9 / -8 -> 0 / 1 and effLen 21, then min(12 - 0, 14 - 1)
    nucl("clip at the starts", "start and end clip, q 12 s 14, keep: effLen = min(a, b, effLen) = 12 after the shift", 12, 14, 1, 11, 2, 10, 3, 2.0, [(0, "m" * 12)], expect=True)
    nucl("clip at the starts", "start and end clip, q 12 s 14, drop: query 11, the last cell, is a mismatch", 12, 14, 1, 11, 2, 10, 3, 2.0, [(0, "m" * 11 + "x")], expect=False)

    # ---- clip at the ends: a = q_len - effQ and b = s_len - effS (lx_prefilter.hip:43-47)
    nucl("clip at the ends", "seed ends at q_len, keep: a = 15 < effLen", 40, 100, 30, 40, 50, 10, 2, 2.0, [(25, "m" * 15)], expect=True)
    nucl("clip at the ends", "seed ends at q_len, drop: the last residue of the query is a mismatch", 40, 100, 30, 40, 50, 10, 2, 2.0, [(25, "m" * 14 + "x")], expect=False)
    nucl("clip at the ends", "region ends at s_len, keep: b = 15 < effLen", 100, 60, 20, 30, 50, 10, 2, 2.0, [(15, "m" * 15)], expect=True)
    nucl("clip at the ends", "region ends at s_len, drop: the last residue of the subject is a mismatch", 100, 60, 20, 30, 50, 10, 2, 2.0, [(15, "m" * 14 + "x")], expect=False)
    # (seed 8 long: the begins move back by 6, to 17 and 31)
    nucl("clip at the ends", "both ends, a = 14 < b = 15, keep", 31, 46, 23, 31, 37, 10, 2, 2.0, [(17, "m" * 14)], expect=True)
    nucl("clip at the ends", "both ends, b = 14 < a = 18, keep", 35, 45, 23, 31, 37, 10, 2, 2.0, [(17, "m" * 14)], expect=True)
    nucl("clip at the ends", "both ends, b = 14 < a = 18, drop: the region's first cell", 35, 45, 23, 31, 37, 10, 2, 2.0, [(17, "x")], fill="m", expect=False)

    # ---- no widening: effLen == actual, so lx_prefilter.hip:32-48 is skipped and nothing is clipped, wherever the seed lies.  The keep
    # cases are identities on the seed only, the drop cases identities everywhere but on one cell of the seed.
    for name, qs, n, sl, pre in (("actual 14 > seed_length * pre_scoring 10", 0, 14, 5, 2), ("pre_scoring 1", 3, 10, 10, 1),
                                 ("actual == effLen 20 exactly", 40, 20, 10, 2), ("pre_scoring 1 at the ends of both", 50, 10, 10, 1)):
        ss = qs + 20 if qs != 50 else 70
        nucl("no widening", name + ", keep", 60, 80, qs, qs + n, ss, sl, pre, 2.0, [(qs, "m" * n)], expect=True)
        nucl("no widening", name + ", drop: identities around the seed do not count", 60, 80, qs, qs + n, ss, sl, pre, 2.0, [(qs + n // 2, "x")], fill="m", expect=False)

    # ---- the tail of the dword loop: effLen % 4 in 1, 2, 3 (`i + b < effLen`, lx_prefilter.hip:63).  Drop: the region's first cell is a
    # mismatch, so it reaches 2 (L - 1) < 2 L, and the 1 to 3 cells of the last dword beyond it are identities that would lift it over.
    # Keep, its twin: the last cell inside the region reaches 2 L and the cells beyond are mismatches.
    for L in (13, 14, 15, 17, 5, 2, 1):
        nucl("tail of the dword loop", f"effLen {L} (% 4 = {L % 4}), drop: identities beyond the region", 60, 80, 20, 20 + L, 31, L, 1, 2.0, [(20, "x")], fill="m", expect=False)
        nucl("tail of the dword loop", f"effLen {L} (% 4 = {L % 4}), keep: reached on the last cell inside", 60, 80, 20, 20 + L, 31, L, 1, 2.0, [(20, "m" * L)], expect=True)
    # the same through the widening and the start clip: effLen 17 and 18
    nucl("tail of the dword loop", "clipped to effLen 17, drop: identities beyond", 60, 80, 2, 12, 7, 10, 2, 2.0, [(0, "x")], fill="m", expect=False)
    nucl("tail of the dword loop", "clipped to effLen 18, drop: identities beyond", 60, 80, 3, 13, 9, 10, 2, 2.0, [(0, "x")], fill="m", expect=False)
    nucl("tail of the dword loop", "clipped to effLen 18, keep", 60, 80, 3, 13, 9, 10, 2, 2.0, [(0, "m" * 18)], expect=True)

    # ---- the threshold (`mx >= thresh`, `(int)(thresh * effLen)`, lx_prefilter.hip:52, :72)
    five_x_fourteen = [(30, "m" * 5 + "x" + "m" * 14)]  # 10, 7, then 14 identities: 35
    nucl("threshold", "mx 35 == thresh 1.75 * 20, keep", 80, 90, 35, 45, 40, 10, 2, 1.75, five_x_fourteen, expect=True)
    nucl("threshold", "mx 35 == thresh 1.8 * 20 - 1, drop", 80, 90, 35, 45, 40, 10, 2, 1.8, five_x_fourteen, expect=False)
    nucl("threshold", "1.4 * 17 = 23.8 truncates to 23 == mx (5 m, x, 8 m), keep", 80, 90, 30, 47, 33, 17, 1, 1.4, [(30, "m" * 5 + "x" + "m" * 8)], expect=True)
    nucl("threshold", "1.4 * 17 -> 23 > mx 22 (11 m), drop", 80, 90, 30, 47, 33, 17, 1, 1.4, [(30, "m" * 11)], expect=False)
    nucl("threshold", "1.4 * 14 = 19.6 truncates to 19 <= mx 20, keep", 80, 90, 30, 44, 33, 14, 1, 1.4, [(32, "m" * 10)], expect=True)
    nucl("threshold", "thresh 0.0 on a region of mismatches: 0 >= 0, keep", 80, 90, 35, 45, 40, 10, 2, 0.0, [], expect=True)
    nucl("threshold", "thresh -1.5 on a region of mismatches, keep", 80, 90, 35, 45, 40, 10, 2, -1.5, [], expect=True)
    nucl("threshold", "thresh -0.01 (truncates to -0) on a region of mismatches, keep", 80, 90, 35, 45, 40, 10, 2, -0.01, [], expect=True)
    nucl("threshold", "thresh 0.05 * 20 = 1 on a region of mismatches, drop", 80, 90, 35, 45, 40, 10, 2, 0.05, [], expect=False)
    nucl("threshold", "maximum 20 reached early, destroyed by 10 mismatches, keep", 80, 90, 35, 45, 40, 10, 2, 1.0, [(30, "m" * 10)], expect=True)
    nucl("threshold", "maximum 18 reached early, destroyed, drop", 80, 90, 35, 45, 40, 10, 2, 1.0, [(30, "m" * 9)], expect=False)
    nucl("threshold", "resets to 0 (mm xxx) and climbs to 24 == 1.2 * 20, keep", 80, 90, 35, 45, 40, 10, 2, 1.2, [(30, "mmxxx" + "m" * 12)], expect=True)
    nucl("threshold", "resets to 0 and climbs to 22 < 24, drop", 80, 90, 35, 45, 40, 10, 2, 1.2, [(30, "mmxxx" + "m" * 11)], expect=False)
    nucl("threshold", "no reset would give 4 - 9 + 26 = 21: 26 after the reset, thresh 1.3 * 20 = 26, keep", 80, 90, 35, 45, 40, 10, 2, 1.3, [(30, "mmxxx" + "m" * 13)], expect=True)

    # ---- a zero-length region (`effLen > 0 &&`, lx_prefilter.hip:74; the loop that never runs)
    for thr in (2.0, 0.0, -1.0):
        nucl("zero-length region", f"qry_end == qry_start, pre_scoring 0, thresh {thr}: drop", 60, 80, 20, 20, 30, 10, 0, thr, [], fill="m", expect=False)
    nucl("zero-length region", "qry_end == qry_start == 0, pre_scoring 0, thresh 0: drop", 60, 80, 0, 0, 0, 10, 0, 0.0, [], fill="m", expect=False)
    nucl("zero-length region", "qry_end == qry_start, pre_scoring 2: the region is 20 around it, keep", 60, 80, 20, 20, 30, 10, 2, 2.0, [(10, "m" * 20)], expect=True)
    nucl("zero-length region", "qry_end == qry_start, pre_scoring 2, drop: cell 19 of the region", 60, 80, 20, 20, 30, 10, 2, 2.0, [(29, "x")], fill="m", expect=False)
    nucl("zero-length region", "qry_end == qry_start == q_len, pre_scoring 2: clipped to the 10 before it, keep", 40, 80, 40, 40, 60, 10, 2, 2.0, [(30, "m" * 10)], expect=True)

    # ---- the schemes: the matrix row is the query's rank, the column the subject's (lx_prefilter.hip:65)
    A, Cc, G, T, N = 0, 1, 2, 3, 4
    base = rng.integers(0, 4, 60).astype(np.uint8)
    withn = base.copy()
    withn[[21, 24, 30, 37]] = N
    add("schemes", "nucl, N against N inside the region (by the matrix)", withn, withn.copy(), 25, 35, 25, 10, 2, 2.0, "nucl")
    s = withn.copy()
    s[[21, 24, 30, 37]] = A
    add("schemes", "nucl, N against A: drop", withn, s, 25, 35, 25, 10, 2, 2.0, "nucl", expect=False)
    add("schemes", "nucl, rank 3 against rank 4 everywhere: drop", np.full(40, 3, np.uint8), np.full(40, 4, np.uint8), 15, 25, 15, 10, 2, 0.1, "nucl", expect=False)
    add("schemes", "nucl, identities without N: keep", base, base.copy(), 25, 35, 25, 10, 2, 2.0, "nucl", expect=True)
    qt, sc_ = np.full(40, T, np.uint8), np.full(40, Cc, np.uint8)  # query T on subject C: a match on the forward strand only
    qa, sg = np.full(40, A, np.uint8), np.full(40, G, np.uint8)    # query A on subject G: a match on the reverse strand only
    add("schemes", "bs_fwd in slot 0, T on C: keep", qt, sc_, 15, 25, 15, 10, 2, 2.0, "bs_fwd", 0, expect=True)
    add("schemes", "bs_fwd in slot 0, C on T (the transpose): drop", sc_, qt, 15, 25, 15, 10, 2, 2.0, "bs_fwd", 0, expect=False)
    add("schemes", "bs_fwd in slot 0, A on G: drop", qa, sg, 15, 25, 15, 10, 2, 2.0, "bs_fwd", 0, expect=False)
    add("schemes", "bs_rev in slot 1, A on G: keep", qa, sg, 15, 25, 15, 10, 2, 2.0, "bs_rev", 1, expect=True)
    add("schemes", "bs_rev in slot 1, G on A (the transpose): drop", sg, qa, 15, 25, 15, 10, 2, 2.0, "bs_rev", 1, expect=False)
    add("schemes", "bs_rev in slot 1, T on C: drop", qt, sc_, 15, 25, 15, 10, 2, 2.0, "bs_rev", 1, expect=False)
    add("schemes", "bs_fwd, N on N is a mismatch: drop", np.full(40, N, np.uint8), np.full(40, N, np.uint8), 15, 25, 15, 10, 2, 0.1, "bs_fwd", 0, expect=False)
    star, x, w, a = (PROT.index(c) for c in "*XWA")
    stars = np.full(40, star, np.uint8)
    add("schemes", "blosum62, 20 cells * on * (1 each) reach 1.0 * 20 on the last one: keep", stars, stars.copy(), 15, 25, 15, 10, 2, 1.0, "blosum62", expect=True)
    q = stars.copy()
    q[20] = x
    add("schemes", "blosum62, X on X (-1) among * on *: 18 < 20, drop", q, q.copy(), 15, 25, 15, 10, 2, 1.0, "blosum62", expect=False)
    add("schemes", "blosum62, X on * against the transposed cell", q, stars.copy(), 15, 25, 15, 10, 2, 0.5, "blosum62")
    q = np.full(40, w, np.uint8)
    q[10:14] = star
    s = np.full(40, w, np.uint8)
    s[10:14] = a
    add("schemes", "blosum62, * on A (-4 each) four times, then W on W 11: keep", q, s, 15, 25, 15, 10, 2, 2.0, "blosum62", expect=True)
    add("schemes", "blosum62, W against A everywhere: drop", np.full(40, w, np.uint8), np.full(40, a, np.uint8), 15, 25, 15, 10, 2, 0.1, "blosum62", expect=False)
    prot = rng.integers(0, 27, 90).astype(np.uint8)
    add("schemes", "blosum62, all 27 ranks, identities", prot, prot.copy(), 40, 50, 40, 10, 2, 2.0, "blosum62")
    add("schemes", "blosum62, all 27 ranks against another diagonal", prot, prot.copy(), 40, 50, 47, 10, 2, 2.0, "blosum62")

    # ---- the buffer ends: the region ends on the last byte of the query and of the subject at once (effLen 15: the last dword reaches 1
    # byte into the slack behind each buffer, lx_prefilter.hip:59).  buffers() puts such a case last, so that these are the buffers' ends.
    nucl("buffer ends", "region ends at q_len and s_len, effLen 15, keep: reached on the very last byte", 33, 47, 23, 33, 37, 10, 2, 2.0, [(18, "m" * 15)], expect=True)
    nucl("buffer ends", "region ends at q_len and s_len, effLen 15, drop: 28 < 30 whatever lies behind the buffers", 33, 47, 23, 33, 37, 10, 2, 2.0, [(18, "x" + "m" * 14)], expect=False)
    nucl("buffer ends", "seed of 8, effLen 14 (2 bytes of slack), drop", 33, 47, 25, 33, 39, 10, 2, 2.0, [(19, "x" + "m" * 13)], expect=False)
    nucl("buffer ends", "seed of 8, effLen 14, keep", 33, 47, 25, 33, 39, 10, 2, 2.0, [(19, "m" * 14)], expect=True)
    nucl("buffer ends", "seed of 6, effLen 13 (3 bytes of slack), drop", 33, 47, 27, 33, 41, 10, 2, 2.0, [(20, "x" + "m" * 12)], expect=False)
    nucl("buffer ends", "seed of 6, effLen 13, keep", 33, 47, 27, 33, 41, 10, 2, 2.0, [(20, "m" * 13)], expect=True)
    return out


def expected(c: Case) -> bool:
    return model(c.q, c.s, c.qry_start, c.qry_end, c.subj_start, c.seed_length, c.pre_scoring, c.thresh, matrix_of(c.scheme))


def buffers(cs, seed_dtype, last=None):
    """The cases' sequences back to back, as lx_prefilter_batch takes them: (q_res, s_res, seeds).  `last`: the case whose sequences
    close both buffers (its region then ends on the buffers' last bytes)."""
    order = [c for c in cs if c is not last] + ([last] if last is not None else [])
    q_off = np.cumsum([0] + [len(c.q) for c in order])
    s_off = np.cumsum([0] + [len(c.s) for c in order])
    at = {id(c): k for k, c in enumerate(order)}
    seeds = np.zeros(len(cs), dtype=seed_dtype)
    for i, c in enumerate(cs):
        k = at[id(c)]
        seeds[i] = (q_off[k], s_off[k], len(c.q), len(c.s), c.qry_start, c.qry_end, c.subj_start, 0)
    return np.concatenate([c.q for c in order]), np.concatenate([c.s for c in order]), seeds
