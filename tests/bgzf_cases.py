"""Inputs that drive the BGZF encoder (lambda_amd/csrc/lx_bgzf.hip) to DEFLATE's limits, and two small references for its tests
(tests/test_bgzf_cases.py on the CPU, tests/test_gpu_bgzf_limits.py on the device).  Nothing here calls the library.

References:
    min_depth(freq)            the height of the shallowest Huffman tree: above the limit, the encoder must have limited the code
    limited_cost(freq, limit)  the bits of the optimal length-limited code (package-merge)

Inputs, each one block (<= 65 280 bytes), deterministic:
    dist_skew()   4-byte copies whose distances fill 17 distance symbols steeper than Fibonacci: the distance code must be
                  limited to 15 bits
    cl_skew(seed) literals whose designed code lengths give the header's run-length symbols a histogram that must be limited
                  to 7 bits
    window(P)     a random unit of P bytes, repeated: the distance P on either side of 32 768
    runs(n)       zeros: the match lengths 4, 257 / 258 and matches that end with the block
    few()         one or two distinct bytes, and all 256 once

`model_parse` restates the kernel's parse (one candidate per position from a 13-bit hash of four bytes, positions taken 256 at a
time, greedy).  It is the generators' aid -- dist_skew must know which earlier position the kernel will find -- and nothing compares
the device with it.
"""
from __future__ import annotations

import heapq
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests.deflate_craft import DBASE, DEXTRA

BLOCK = 65280
CHUNK = 256      # positions the kernel takes at a time: a position sees the hash heads as they stood before its chunk
HASH_BITS = 13
WINDOW = 32768


# ---- references

def min_depth(freq) -> int:
    """The height of a Huffman tree of the used symbols, ties broken towards the shallower subtree (a heap keyed by
    (weight, height)): the smallest height any optimal prefix code has.  One used symbol: 1; none: 0."""
    heap = [(int(f), 0) for f in freq if f]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    while len(heap) > 1:
        (w1, h1), (w2, h2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (w1 + w2, max(h1, h2) + 1))
    return heap[0][1]


def limited_cost(freq, limit: int) -> int:
    """sum(freq * length) of the optimal prefix code with no length above `limit`, by package-merge (Larmore & Hirschberg 1990):
    `limit` lists of the weights, each but the first merged with the pairs of the one before; the 2 m - 2 lightest items of the
    last list are the code, and a weight counts once per item it is part of, which is its length.  One used symbol: one bit each."""
    w = sorted(int(f) for f in freq if f)
    m = len(w)
    if m < 2:
        return sum(w)
    assert (1 << limit) >= m, "no prefix code that short"
    cur = w
    for _ in range(limit - 1):
        cur = sorted(w + [cur[i] + cur[i + 1] for i in range(0, len(cur) - 1, 2)])
    return sum(cur[:2 * m - 2])


# ---- the kernel's parse, restated

def _hashes(a):
    """the hash of the four bytes at every position p with p + 4 <= len(a)"""
    d = a.astype(np.uint32)
    w = d[:-3] | d[1:-2] << np.uint32(8) | d[2:-1] << np.uint32(16) | d[3:] << np.uint32(24)
    return ((w * np.uint32(2654435761)) >> np.uint32(32 - HASH_BITS)).astype(np.int64)


def model_parse(data: bytes):
    """The tokens (int literal or (length, distance)) the kernel's parse gives `data`, one block."""
    a = np.frombuffer(data, np.uint8)
    n = len(a)
    assert n <= BLOCK
    h = _hashes(a) if n >= 4 else np.zeros(0, np.int64)
    head = np.zeros(1 << HASH_BITS, np.int64)  # position + 1 of the last insert
    mlen, dist = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for c0 in range(0, len(h), CHUNK):
        hh = h[c0:c0 + CHUNK]
        cand = head[hh]
        np.maximum.at(head, hh, np.arange(c0, c0 + len(hh)) + 1)
        for i in np.nonzero(cand)[0]:
            p, q = c0 + int(i), int(cand[i]) - 1
            if p - q > WINDOW:
                continue
            lim = min(258, n - p)
            ne = np.nonzero(a[q:q + lim] != a[p:p + lim])[0]
            length = int(ne[0]) if ne.size else lim
            if length >= 4:
                mlen[p], dist[p] = length, p - q
    tokens, p = [], 0
    while p < n:
        if mlen[p]:
            tokens.append((int(mlen[p]), int(dist[p])))
            p += int(mlen[p])
        else:
            tokens.append(int(a[p]))
            p += 1
    return tokens


# ---- dist_skew

# a[k] = a[k-1] + a[k-2] + 1 over 17 distance symbols: every weight exceeds the sum of the two before it, so the Huffman tree is a
# chain of height 16.  The rarest go to the symbols 13..15 (distances 97..256, which a position reaches only early in its chunk:
# its source was inserted before the chunk), the heaviest to 23..25 (3 073..8 192: far enough to be in the table from any place in
# a chunk, near enough that most positions there still own their hash bucket), the far symbols 26..29 get middling counts (they
# are within reach only late in the block, and few positions that far back still own their bucket).
DIST_SKEW_COUNTS = {13: 1, 14: 2, 15: 4, 16: 7, 17: 12, 18: 20, 29: 33, 19: 54, 28: 88, 20: 143, 27: 232, 21: 376, 26: 609, 22: 986, 25: 1596,
                    23: 2583, 24: 4180}
DIST_SKEW_PREFIX = 2048
DIST_SKEW_COPIES = sum(DIST_SKEW_COUNTS.values())
assert DIST_SKEW_COPIES == 10926
_DHI = [DBASE[s] + (1 << DEXTRA[s]) - 1 for s in range(30)]


@lru_cache(maxsize=None)
def dist_skew(seed: int = 0) -> bytes:
    """2 048 random bytes, then 10 926 copies of exactly four bytes at distances drawn so that the distance symbols get
    DIST_SKEW_COUNTS, then one byte.  A copy's source is the owner of its hash bucket as of the start of the copy's chunk, so it
    is the one candidate the kernel looks at; the byte behind a copy differs from the byte behind its source, so the match is 4
    long.  The copies of a symbol are spread over the block by drawing symbols like balls from an urn (those within reach), but
    13..15 are taken at the first chance."""
    rng = np.random.default_rng(seed)
    total = DIST_SKEW_PREFIX + 4 * DIST_SKEW_COPIES + 1
    a = np.zeros(total, np.uint8)
    a[:DIST_SKEW_PREFIX] = rng.integers(0, 256, DIST_SKEW_PREFIX, dtype=np.uint8)
    n = DIST_SKEW_PREFIX
    hs = np.zeros(total, np.int64)              # the hash of every position below `hashed`
    head = np.zeros(1 << HASH_BITS, np.int64)   # the owners among the positions below `inserted`
    hashed = inserted = 0
    left = dict(DIST_SKEW_COUNTS)
    forbid = -1                                 # the byte behind the last source: the next copy must not start with it

    def source(s, p, c0):
        lo, hi = max(p - _DHI[s], 0), min(p - DBASE[s], c0 - 1, inserted - 1)
        if hi < lo:
            return -1
        for q in (rng.integers(lo, hi + 1, 64), np.arange(lo, hi + 1)):  # a sample first, the whole range if it holds none
            ok = (head[hs[q]] == q + 1) & (a[q] != forbid)
            if ok.any():
                return int(q[np.argmax(ok)])
        return -1

    for _ in range(DIST_SKEW_COPIES):
        p, c0 = n, n - n % CHUNK
        if hashed < n - 3:
            hs[hashed:n - 3] = _hashes(a[hashed:n])
            hashed = n - 3
        upto = min(c0, hashed)  # (the last three positions before the chunk wait for their bytes: one copy later)
        if inserted < upto:
            np.maximum.at(head, hs[inserted:upto], np.arange(inserted, upto) + 1)
            inserted = upto
        q = -1
        for s in (13, 14, 15):
            if left[s] and q < 0:
                q, sym = source(s, p, c0), s
        if q < 0:
            urn = [s for s in left if s > 15 and left[s] and p >= DBASE[s]]
            weights = np.array([left[s] for s in urn], float)
            first = urn[int(rng.choice(len(urn), p=weights / weights.sum()))]
            for s in [first] + sorted((s for s in urn if s != first), key=lambda s: -left[s]):
                q, sym = source(s, p, c0), s
                if q >= 0:
                    break
        assert q >= 0, "no source for a copy: another seed"
        left[sym] -= 1
        a[n:n + 4] = a[q:q + 4]
        n += 4
        forbid = int(a[q + 4])
    assert not any(left.values()), left
    a[n] = (forbid + 1) & 255
    return a.tobytes()


# ---- cl_skew

# (code length, how many byte values get it): the histogram of the header's code-length symbols follows it
CL_SKEW_PLAN = ((4, 2), (5, 4), (6, 7), (7, 12), (8, 90), (9, 56), (10, 34), (11, 21), (13, 1))
CL_SKEW_BYTES = 64000


@lru_cache(maxsize=None)
def cl_skew(seed: int) -> bytes:
    """About 64 000 shuffled bytes over the values 0..226, value v about N * 2^-len[v] times, so that the literal code comes out
    with the planned lengths and no copies; the lengths are shuffled over the values until no four neighbours are equal (a run of
    four would be written with symbol 16)."""
    rng = np.random.default_rng(seed)
    lens = np.repeat([l for l, _ in CL_SKEW_PLAN], [c for _, c in CL_SKEW_PLAN])
    while True:
        rng.shuffle(lens)
        if not ((lens[:-3] == lens[1:-2]) & (lens[1:-2] == lens[2:-1]) & (lens[2:-1] == lens[3:])).any():
            break
    share = 2.0 ** -lens
    counts = np.maximum(1, np.rint(CL_SKEW_BYTES / share.sum() * share)).astype(np.int64)
    data = np.repeat(np.arange(len(lens), dtype=np.uint8), counts)
    rng.shuffle(data)
    return data.tobytes()


# the seeds whose inputs gave, on the device, a header whose run-length symbols need a tree higher than 7
CL_SKEW_SEEDS = (0, 2)


# ---- window, runs, few

WINDOW_PERIODS = (32767, 32768, 32769)


@lru_cache(maxsize=None)
def _window_units():
    rng = np.random.default_rng(5)
    return {P: rng.integers(0, 256, P, dtype=np.uint8).tobytes() for P in WINDOW_PERIODS}


def window(P: int) -> bytes:
    """a random unit of P bytes repeated to one whole block"""
    unit = _window_units()[P]
    return (unit * (BLOCK // P + 1))[:BLOCK]


RUN_LENGTHS = (259, 260, 514, 515, 517, 518, 256 + 257, 256 + 258 + 257)
# the tokens behind the 256 literals of the first chunk, each match with the position it ends at; a literal is 0, None stands
# for a distance that is not pinned
RUN_TOKENS = {259: [0, 0, 0], 260: [(4, 1, 260)], 514: [(258, 1, 514)], 515: [(258, 1, 514), 0], 517: [(258, 1, 514), 0, 0, 0],
              518: [(258, 1, 514), (4, None, 518)], 256 + 257: [(257, 1, 513)], 256 + 258 + 257: [(258, 1, 514), (257, None, 771)]}


def runs(n: int) -> bytes:
    return bytes(n)


def few():
    """(name, bytes): one distinct byte at 1..5 bytes, two distinct bytes at 2, 4, 5, 256 and 300, every value once.  (The short
    ones come out stored; 256 bytes of two values are the dynamic block without a copy: the first 256 positions never have one.)"""
    out = [(f"one_value_{n}", b"\x07" * n) for n in range(1, 6)]
    rng = np.random.default_rng(11)
    for n in (2, 4, 5, 256, 300):
        x = rng.integers(0, 2, n, dtype=np.uint8)
        x[0], x[-1] = 0, 1  # (both values, whatever the draw)
        out.append((f"two_values_{n}", (x * 0x5A + 0x20).astype(np.uint8).tobytes()))
    out.append(("every_value_once", bytes(range(256))))
    return out


Case = namedtuple("Case", "name data")


@lru_cache(maxsize=None)
def all_cases():
    c = [Case("dist_skew", dist_skew())]
    c += [Case(f"cl_skew_{s}", cl_skew(s)) for s in CL_SKEW_SEEDS]
    c += [Case(f"window_{P}", window(P)) for P in WINDOW_PERIODS]
    c += [Case(f"runs_{n}", runs(n)) for n in RUN_LENGTHS]
    c += [Case(f"few_{name}", data) for name, data in few()]
    return tuple(c)
