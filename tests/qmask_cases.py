"""The query masking rule restated in Python, and the inputs of its tests (tests/test_query_mask.py, tests/test_gpu_query_mask.py).
Nothing here calls the library: `seg_mask` is the yardstick the host function and the kernels
are held against."""
import math
from collections import Counter

import numpy as np

from tests import level3_cases as l3

ALPHABET = "ABCDEFGHIJKLMNOPQRSTUVWYZX*"  # alignment ranks of the protein alphabet


def ranks(text: str) -> np.ndarray:
    return np.array([ALPHABET.index(c) for c in text], np.uint8)


def seg_tables(W=12, k1=2.2, k2=2.5):
    T = [0, 0] + [round(c * math.log2(c) * 65536) for c in range(2, 65)]
    return T, math.ceil(W * (math.log2(W) - k1) * 65536), math.ceil(W * (math.log2(W) - k2) * 65536)


def seg_mask(seq, W=12, k1=2.2, k2=2.5) -> np.ndarray:
    """0 / 1 per letter of one sequence: SEG's first two stages, in integers"""
    T, thr1, thr2 = seg_tables(W, k1, k2)
    seq, L = list(map(int, seq)), len(seq)
    mask = np.zeros(L, np.uint8)
    if L < W:
        return mask
    S = [sum(T[n] for n in Counter(seq[p:p + W]).values()) for p in range(L - W + 1)]
    p = 0
    while p < len(S):
        if S[p] < thr2:
            p += 1
            continue
        e = p
        while e + 1 < len(S) and S[e + 1] >= thr2:
            e += 1
        if any(s >= thr1 for s in S[p:e + 1]):
            mask[p:e + W] = 1
        p = e + 1
    return mask


def seg_mask_set(q_res, q_off, q_len, W=12, k1=2.2, k2=2.5) -> np.ndarray:
    """the masks of a set's sequences, indexed like q_res up to the last sequence's end"""
    ends = [int(o) + int(n) for o, n in zip(q_off, q_len) if n]
    out = np.zeros(max(ends, default=0), np.uint8)
    for o, n in zip(map(int, q_off), map(int, q_len)):
        out[o:o + n] = seg_mask(q_res[o:o + n], W, k1, k2)
    return out


def counts(mask, q_off, q_len):
    """(letters, masked letters, sequences with a masked letter)"""
    off, ln = np.asarray(q_off, np.int64), np.asarray(q_len, np.int64)
    before = np.concatenate([[0], np.cumsum(mask, dtype=np.int64)])
    per = np.where(ln > 0, before[np.minimum(off + ln, len(mask))] - before[np.minimum(off, len(mask))], 0)
    return int(ln.sum()), int(per.sum()), int((per > 0).sum())


def seed_starts_masked(res, mask, seed_length, seed_offset, unknown):
    """level3_cases.seed_starts with the blocked rule: a start whose seed_length letters hold a masked letter is passed over like the
    unknown letter; the loop stops at L - seed_length, and a start still blocked there ends the sequence"""
    L, out, b = len(res), [], 0
    if L < seed_length:
        return out

    def blocked(p):
        return bool(mask[p:p + seed_length].any())

    while True:
        while b < L - seed_length and (res[b] == unknown or res[b] == res[b + 1] or blocked(b)):
            b += 1
        if b > L - seed_length or blocked(b):
            return out
        out.append(b)
        b += seed_offset


def brute_exact_matches_masked(c, mask, seed_length, seed_offset):
    """level3_cases.brute_exact_matches over the masked starts"""
    words = {}
    for s, (o, n) in enumerate(zip(c["s_off"].astype(int), c["s_len"].astype(int))):
        for p in range(n - seed_length + 1):
            words.setdefault(c["s_red"][o + p:o + p + seed_length].tobytes(), []).append((s, p))
    out = []
    for i, (o, n) in enumerate(zip(c["q_off"].astype(int), c["q_len"].astype(int))):
        for b in seed_starts_masked(c["q_res"][o:o + n], mask[o:o + n], seed_length, seed_offset, c["unknown"]):
            for s, p in words.get(c["q_red"][o + b:o + b + seed_length].tobytes(), []):
                out.append((i, s, b, b + seed_length, p, p + seed_length))
    m = np.zeros(len(out), dtype=[(f, "<u8") for f in l3.MATCH_FIELDS])
    for k, f in enumerate(l3.MATCH_FIELDS):
        m[f] = [r[k] for r in out]
    return m


def as_set(seqs):
    """(q_res, q_off, q_len) of sequences laid end to end"""
    seqs = [np.asarray(s, np.uint8) for s in seqs]
    off, ln = l3.offsets([len(s) for s in seqs]) if seqs else (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    return (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)), off, ln


def partitions(n, largest=None):
    """the partitions of n, each as a descending tuple (77 of them for n = 12)"""
    largest = n if largest is None else largest
    if n == 0:
        yield ()
        return
    for first in range(min(n, largest), 0, -1):
        for rest in partitions(n - first, first):
            yield (first,) + rest


def composition_windows(W=12):
    """one window per composition of W letters: letter k repeated part[k] times, the letters interleaved round robin"""
    out = []
    for part in partitions(W):
        left, seq = list(part), []
        while len(seq) < W:
            for k in range(len(left)):
                if left[k]:
                    seq.append(k)
                    left[k] -= 1
        out.append(np.array(seq, np.uint8))
    return out


def random_protein(rng, n):
    return rng.integers(0, 20, n).astype(np.uint8)


def repeat(unit: str, n: int) -> np.ndarray:
    return ranks((unit * (n // len(unit) + 1))[:n])


def named_cases(W=12):
    """name -> list of sequences: the hand-made cases of the issue"""
    rng = np.random.default_rng(11)
    flank = lambda n: random_protein(rng, n)  # noqa: E731
    # five letters in equal parts hold 2.29 bits per window of twelve: under k2, not under k1.  Three of them next to an SP repeat make
    # one run with it: a window that takes SP letters in only loses entropy
    weak = repeat("SPACD", 30)
    strong = repeat("SP", 30)
    return {
        "length W - 1": [repeat("SP", W - 1)],
        "length W": [repeat("SP", W)],
        "length W + 1": [repeat("SP", W + 1)],
        "ASASASASASAS": [ranks("ASASASASASAS")],
        "eleven A": [ranks("A" * 11)],
        "weak before trigger": [np.concatenate([flank(20), weak, strong, flank(20)])],
        "weak behind trigger": [np.concatenate([flank(20), strong, weak, flank(20)])],
        "weak alone": [np.concatenate([flank(20), weak, flank(20)])],
        "two times six A": [ranks("AAAAAA"), ranks("AAAAAA")],
        "empty between": [repeat("SP", 20), np.zeros(0, np.uint8), flank(30), np.zeros(0, np.uint8), np.zeros(0, np.uint8), repeat("K", 15)],
        "flanked SP": [np.concatenate([ranks("MKVLAAGIVNGNW"), repeat("SP", 30), ranks("FRYTEELKKAG")])],
    }


def random_frames(seed: int):
    """a seeded set of frames: 1 to 12 sequences of 0 to 80 letters, each random, repetitive, or random with a repeat inside"""
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(int(rng.integers(1, 13))):
        n, kind = int(rng.integers(0, 81)), int(rng.integers(0, 4))
        x = random_protein(rng, n)
        if kind == 1 and n:
            unit = rng.integers(0, 25, int(rng.integers(1, 5))).astype(np.uint8)
            x = np.resize(unit, n)
        elif kind == 2 and n > 10:
            a, b = sorted(rng.integers(0, n, 2))
            x[a:b] = np.resize(rng.integers(0, 25, int(rng.integers(1, 4))).astype(np.uint8), b - a)
        elif kind == 3 and n:
            x = rng.integers(0, int(rng.integers(2, 7)), n).astype(np.uint8)
        seqs.append(x)
    return seqs
