"""Inputs and numpy restatements for the Level-3 tests (tests/test_level3_abi.py, tests/test_gpu_level3.py): the word table by
brute force, exact seeding by brute force, and the small protein / translated / nucleotide / bisulfite sets of the parity tests.
Nothing here calls the library."""
import numpy as np

from lambda_amd import synth

# lambda_amd/csrc/host/lx_seeding.hpp: kLi10 over the ranks "ABCDEFGHIJKLMNOPQRSTUVWYZX*", kDna4 over (A, C, G, N, T), the bisulfite pair over (A, C, G, T, N)
LI10 = np.array([0, 1, 2, 1, 1, 3, 4, 5, 6, 7, 8, 7, 7, 5, 8, 9, 1, 8, 0, 0, 2, 6, 3, 3, 1, 0, 3], np.uint8)
DNA4 = np.array([0, 1, 2, 0, 3], np.uint8)
BS_FWD = np.array([0, 1, 2, 1, 0], np.uint8)
BS_REV = np.array([3, 4, 3, 5, 3], np.uint8)
MATCH_FIELDS = ("qryId", "subjId", "qryStart", "qryEnd", "subjStart", "subjEnd")


def key_len(alph: int) -> int:
    """the largest k with (alph + 1)^k <= 2^63 - 1, as ReducedIndex counts it"""
    base, lim, p, k = alph + 1, (2 ** 64 - 1) // 2, 1, 0
    while p <= lim // base:
        p *= base
        k += 1
    return k


def offsets(lens):
    lens = np.asarray(lens, np.uint64)
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), lens


def brute_table(red, off, lens, alph):
    """every (key, seq, pos), sorted: key = the next key_len letters in base alph + 1, the digit alph behind the sequence's end"""
    kl, base = key_len(alph), np.uint64(alph + 1)
    rows = []
    for s, (o, n) in enumerate(zip(off.astype(int), lens.astype(int))):
        if n == 0:
            continue
        padded = np.concatenate([red[o:o + n], np.full(kl, alph, np.uint8)]).astype(np.uint64)
        key = np.zeros(n, np.uint64)
        for i in range(kl):
            key = key * base + padded[i:i + n]
        rows.append(np.stack([key, np.full(n, s, np.uint64), np.arange(n, dtype=np.uint64)], 1))
    t = np.concatenate(rows) if rows else np.zeros((0, 3), np.uint64)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def table_inputs(alph: int, seed: int = 5):
    """40 reduced sequences of 5 to 300 letters, one of them empty and one shorter than the key length"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(5, 301, 40)
    lens[7], lens[11] = 0, min(9, key_len(alph) - 1)
    off, lens = offsets(lens)
    return rng.integers(0, alph, int(lens.sum())).astype(np.uint8), off, lens


def seed_starts(res, seed_length, seed_offset, unknown):
    """where search() puts its seeds (src/search_algo.hpp:652-663): every seed_offset letters; a start on the unknown letter or on a
    letter equal to its successor moves right"""
    L, out, b = len(res), [], 0
    if L < seed_length:
        return out
    while True:
        while b < L - seed_length and (res[b] == unknown or res[b] == res[b + 1]):
            b += 1
        if b > L - seed_length:
            return out
        out.append(b)
        b += seed_offset


def brute_exact_matches(c, seed_length, seed_offset):
    """the matches of exact seeds without elongation and pre-scoring: every subject position whose reduced word equals the seed's"""
    words = {}
    for s, (o, n) in enumerate(zip(c["s_off"].astype(int), c["s_len"].astype(int))):
        for p in range(n - seed_length + 1):
            words.setdefault(c["s_red"][o + p:o + p + seed_length].tobytes(), []).append((s, p))
    out = []
    for i, (o, n) in enumerate(zip(c["q_off"].astype(int), c["q_len"].astype(int))):
        for b in seed_starts(c["q_res"][o:o + n], seed_length, seed_offset, c["unknown"]):
            for s, p in words.get(c["q_red"][o + b:o + b + seed_length].tobytes(), []):
                out.append((i, s, b, b + seed_length, p, p + seed_length))
    m = np.zeros(len(out), dtype=[(f, "<u8") for f in MATCH_FIELDS])
    for k, f in enumerate(MATCH_FIELDS):
        m[f] = [r[k] for r in out]
    return m


def sorted_matches(m):
    return np.sort(np.asarray(m), order=list(MATCH_FIELDS))


def max_word_count(c) -> int:
    """how often the most frequent word of key_len letters occurs in the subjects (the device declines beyond 32)"""
    t = brute_table(c["s_red"], c["s_off"], c["s_len"], c["alph"])
    return int(np.unique(t[:, 0], return_counts=True)[1].max())


def make_case(mode: str, n_reads: int, seed: int, n_subjects: int = 30):
    """A small search: mode 'protein' (Li-10, one frame), 'translated' (Li-10, six frames per read), 'nucleotide' (dna4, two frames),
    'bisulfite' (six letters, reduction alternating with the frame, two frames).  Reads: copies of subject pieces with substitutions,
    random ones, and -- where n_reads allows -- one shorter than any seed, one of the unknown letter only, one equal to a subject."""
    rng = np.random.default_rng(seed)
    prot = mode in ("protein", "translated")
    frames = {"protein": 1, "translated": 6, "nucleotide": 2, "bisulfite": 2}[mode]
    letters = synth.STD20.astype(np.uint8) if prot else np.arange(4, dtype=np.uint8) if mode == "bisulfite" else np.array([0, 1, 2, 4], np.uint8)
    unknown = 25 if prot else 4 if mode == "bisulfite" else 3
    alph = 10 if prot else 6 if mode == "bisulfite" else 4

    def reduce(res, frame):
        return LI10[res] if prot else DNA4[res] if mode == "nucleotide" else (BS_REV if frame & 1 else BS_FWD)[res]

    s_lens = rng.integers(60, 260, n_subjects)
    subjects = [letters[rng.integers(0, len(letters), n)] for n in s_lens]
    qlen = 45 if prot else 70
    reads = []
    for r in range(n_reads):
        fr = []
        for f in range(frames):
            if rng.random() < 0.6:
                # (bisulfite: a frame only ever matches subjects of its own parity, the reductions share no letter)
                j = int(rng.integers(0, n_subjects))
                a = int(rng.integers(0, len(subjects[j]) - qlen // 2))
                x = subjects[j][a:a + qlen].copy()
                sub = rng.random(len(x)) < 0.08
                x[sub] = letters[rng.integers(0, len(letters), int(sub.sum()))]
            else:
                x = letters[rng.integers(0, len(letters), qlen)]
            fr.append(x)
        reads.append(fr)
    if n_reads >= 1:
        reads[0][0] = subjects[3].copy()  # equal to a subject
    if n_reads >= 63:
        reads[5] = [letters[rng.integers(0, len(letters), 6)] for _ in range(frames)]  # shorter than any seed
        reads[9] = [np.full(qlen, unknown, np.uint8) for _ in range(frames)]          # the unknown letter only
    seqs = [x for fr in reads for x in fr]
    q_off, q_len = offsets([len(x) for x in seqs])
    s_off, s_len = offsets(s_lens)
    return dict(mode=mode, alph=alph, frames=frames, unknown=unknown,
                s_res=np.concatenate(subjects), s_red=np.concatenate([reduce(x, j) for j, x in enumerate(subjects)]), s_off=s_off, s_len=s_len,
                q_res=np.concatenate(seqs), q_red=np.concatenate([reduce(x, k % frames) for k, x in enumerate(seqs)]), q_off=q_off, q_len=q_len)
