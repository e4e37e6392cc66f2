"""The nucleotide masking rule, symmetric DUST (Morgulis et al. 2006), restated in Python, and the inputs of its tests
(tests/test_query_mask_dust*.py, tests/test_gpu_query_mask_dust*.py).  Nothing here calls the library: `dust_mask_definition` is the
rule word for word, `dust_mask` its sweep form for longer inputs; the host function and the kernels are held against them.

The rule, on alignment ranks A, C, G, T = 0 .. 3 (any other rank is a break: never masked, in no interval): inside a maximal stretch
of ranks 0 .. 3, letter i starts triplet 16 a[i] + 4 a[i + 1] + a[i + 2].  An interval of l consecutive triplets covers l + 2 letters
and scores r / (l - 1), r = sum over triplet kinds of c (c - 1) / 2 (0 for l = 1).  It is perfect when 10 r > level (l - 1) and no
sub-interval scores strictly higher.  A letter is masked exactly when it lies in a perfect interval of at most `window` letters."""
from collections import Counter
from fractions import Fraction

import numpy as np

from tests import level3_cases as l3

DNA = "ACGTN"
WINDOW, LEVEL = 64, 20


def ranks(text: str) -> np.ndarray:
    return np.array([DNA.index(c) for c in text], np.uint8)


def revcomp(seq) -> np.ndarray:
    seq = np.asarray(seq, np.uint8)[::-1]
    return np.where(seq < 4, 3 - seq, seq).astype(np.uint8)


def stretches(seq):
    """[a, b) of the maximal stretches of ranks 0 .. 3"""
    out, a = [], None
    for j, x in enumerate(list(map(int, seq)) + [4]):
        if x < 4 and a is None:
            a = j
        elif x >= 4 and a is not None:
            out.append((a, j))
            a = None
    return out


def _triplets(s):
    return [16 * s[i] + 4 * s[i + 1] + s[i + 2] for i in range(len(s) - 2)]


def dust_mask_definition(seq, window=WINDOW, level=LEVEL) -> np.ndarray:
    """0 / 1 per letter: all intervals, all sub-intervals, exact fractions (slow: sequences up to ~100 letters)"""
    seq = list(map(int, seq))
    mask = np.zeros(len(seq), np.uint8)
    for a, b in stretches(seq):
        t = _triplets(seq[a:b])
        n = len(t)
        score = {}
        for i in range(n):
            for l in range(1, min(window - 2, n - i) + 1):
                r = sum(c * (c - 1) // 2 for c in Counter(t[i:i + l]).values())
                score[i, l] = Fraction(r, l - 1) if l >= 2 else Fraction(0)
        for (i, l), s in score.items():
            if not s > Fraction(level, 10):
                continue
            if all(score[j, m] <= s for j in range(i, i + l) for m in range(1, i + l - j + 1)):
                mask[a + i:a + i + l + 2] = 1
    return mask


def dust_mask(seq, window=WINDOW, level=LEVEL) -> np.ndarray:
    """0 / 1 per letter, by the sweep: M[i][l] = max(S[i][l], M[i][l - 1], M[i + 1][l - 1]); (i, l) is perfect iff S > level / 10
    and S >= max(M[i][l - 1], M[i + 1][l - 1]).  Scores are pairs (r, l - 1) compared by cross-multiplication."""
    seq = list(map(int, seq))
    mask = np.zeros(len(seq), np.uint8)
    for a, b in stretches(seq):
        t = _triplets(seq[a:b])
        n = len(t)
        if n < 2:
            continue
        cnt = [[0] * 64 for _ in range(n)]
        for i in range(n):
            cnt[i][t[i]] = 1
        r, M, reach = [0] * n, [(0, 1)] * n, [0] * n
        for l in range(2, min(window - 2, n) + 1):
            for i in range(n - l + 1):  # ascending: M[i + 1] is still the step before's
                k = t[i + l - 1]
                r[i] += cnt[i][k]
                cnt[i][k] += 1
                top = M[i] if M[i][0] * M[i + 1][1] >= M[i + 1][0] * M[i][1] else M[i + 1]
                if r[i] * top[1] >= top[0] * (l - 1):
                    M[i] = (r[i], l - 1)
                    if 10 * r[i] > level * (l - 1):
                        reach[i] = l + 2
                else:
                    M[i] = top
        for i in range(n):
            mask[a + i:a + i + reach[i]] = 1
    return mask


def dust_mask_set(q_res, q_off, q_len, window=WINDOW, level=LEVEL, definition=False) -> np.ndarray:
    """the masks of a set's sequences, indexed like q_res up to the last sequence's end"""
    ends = [int(o) + int(n) for o, n in zip(q_off, q_len) if n]
    out = np.zeros(max(ends, default=0), np.uint8)
    f = dust_mask_definition if definition else dust_mask
    for o, n in zip(map(int, q_off), map(int, q_len)):
        out[o:o + n] = f(q_res[o:o + n], window, level)
    return out


def as_set(seqs):
    """(q_res, q_off, q_len) of sequences laid end to end"""
    seqs = [np.asarray(s, np.uint8) for s in seqs]
    off, ln = l3.offsets([len(s) for s in seqs]) if seqs else (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    return (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)), off, ln


def counts(mask, q_off, q_len):
    """(letters, masked letters, sequences with a masked letter)"""
    off, ln = np.asarray(q_off, np.int64), np.asarray(q_len, np.int64)
    before = np.concatenate([[0], np.cumsum(mask, dtype=np.int64)])
    per = np.where(ln > 0, before[np.minimum(off + ln, len(mask))] - before[np.minimum(off, len(mask))], 0)
    return int(ln.sum()), int(per.sum()), int((per > 0).sum())


def random_dna(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def repeat(unit: str, n: int) -> np.ndarray:
    return np.resize(ranks(unit), n)


def flanked_a():
    """40 random letters, twenty A, the 40 reversed (the flank ends in T: an A there would belong to the run)"""
    flank = random_dna(np.random.default_rng(7), 40)
    assert flank[-1] != 0
    return np.concatenate([flank, repeat("A", 20), flank[::-1]])


# name -> (sequences, window, what the issue states of the mask at level 20: "all", "none" or the masked [from, to) of sequence 0)
def named_cases():
    return {
        "six A": ([repeat("A", 6)], 64, "none"),
        "seven A": ([repeat("A", 7)], 64, "all"),
        "eight A": ([repeat("A", 8)], 64, "all"),
        "AC of 11": ([repeat("AC", 11)], 64, "none"),
        "AC of 12": ([repeat("AC", 12)], 64, "all"),
        "ACG of 16": ([repeat("ACG", 16)], 64, "none"),
        "ACG of 17": ([repeat("ACG", 17)], 64, "all"),
        "six A, N, six A": ([ranks("AAAAAANAAAAAA")], 64, "none"),
        "seven A between Ns": ([ranks("AAANAAAAAAANCG")], 64, (4, 11)),
        "flanked A": ([flanked_a()], 64, (40, 60)),
        "period 9, window 64": ([repeat("ACGTAGCTT", 120)], 64, "all"),
        "period 9, window 16": ([repeat("ACGTAGCTT", 120)], 16, "none"),
        "empty between": ([repeat("AC", 20), np.zeros(0, np.uint8), random_dna(np.random.default_rng(3), 30), np.zeros(0, np.uint8),
                           np.zeros(0, np.uint8), repeat("T", 15)], 64, None),
        "two times six A": ([repeat("A", 6), repeat("A", 6)], 64, None),
    }


def planted(rng, n):
    """n letters: random, with N now and then and, mostly, a repeat of a 1 .. 6 letter unit planted somewhere (uniform random letters
    are almost never masked)"""
    x = random_dna(rng, n)
    kind = int(rng.integers(0, 5))
    if kind >= 1 and n > 12:
        a = int(rng.integers(0, n - 8))
        b = min(n, a + int(rng.integers(6, 70)))
        x[a:b] = np.resize(rng.integers(0, 4, int(rng.integers(1, 7))).astype(np.uint8), b - a)
        if kind == 4:  # a point mutation inside it
            x[int(rng.integers(a, b))] = rng.integers(0, 4)
    if kind == 3 and n:
        x[rng.integers(0, n, int(rng.integers(1, 3)))] = 4
    return x


def random_reads(seed: int, longest=120):
    """a seeded set: 1 to 10 sequences of 0 to `longest` letters; sequence 0 is plain random and short (untouched at any setting tested)"""
    rng = np.random.default_rng(seed)
    return [random_dna(rng, 5)] + [planted(rng, int(rng.integers(0, longest + 1))) for _ in range(int(rng.integers(1, 10)))]
