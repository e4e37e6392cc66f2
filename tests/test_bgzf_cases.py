"""CPU checks of the BGZF encoder's test helpers: the token-level inflater (tests/deflate_tokens.py) against zlib and against what
tests/deflate_craft.py was asked to write, the two references of tests/bgzf_cases.py against brute force, and the generated inputs
themselves (deterministic, one block, and what they were built to be according to the restated parse)."""
import itertools
import zlib
from fractions import Fraction

import numpy as np
import pytest

from tests import bgzf_cases as B
from tests import deflate_craft as DC
from tests import deflate_tokens as DT


def _all_tokens(blocks):
    return [t for b in blocks for t in b.tokens]


# ---- the inflater

@pytest.mark.parametrize("case", DC.valid_cases(), ids=lambda c: c.name)
def test_tokens_of_the_crafted_streams_expand_to_zlibs_bytes(case):
    blocks = DT.blocks(case.raw, lenient=True)
    want = zlib.decompress(case.raw, -15)
    assert want == case.data and DT.expand(_all_tokens(blocks)) == want
    assert blocks[-1].final and not any(b.final for b in blocks[:-1])
    assert -(-blocks[-1].bits // 8) == len(case.raw)
    if len(case.raw) < 60000:  # (a member with other subfields and a name still fits into 64 KiB)
        member = DC.bgzf_member(case.raw, case.data, extra_before=b"XY\x01\x00z", fname=b"name")
        assert DT.member_stream(member) == case.raw


def _text(n):
    rng = np.random.default_rng(31)
    words = [b"read", b"subject", b"query", b"ACGTTGCA", b"score", b"evalue", b"\t", b"\n", b"0.001", b"identity", b"frame", b"lambda"]
    out = b" ".join(words[i] for i in rng.integers(0, len(words), n // 4))
    return out[:n]


@pytest.mark.parametrize("level", [1, 6, 9])
def test_tokens_of_zlibs_streams_expand_to_its_input(level):
    data = _text(6000)
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = c.compress(data) + c.flush()
    blocks = DT.blocks(raw)  # strict: zlib writes complete codes
    assert zlib.decompress(raw, -15) == data and DT.expand(_all_tokens(blocks)) == data
    assert any(not isinstance(t, int) for t in _all_tokens(blocks)) and blocks[0].btype == 2
    assert -(-blocks[-1].bits // 8) == len(raw)
    for b in blocks:
        assert DC.canonical(b.lit_lens)[1] == 1 and DC.canonical(b.cl_lens)[1] == 1


def _craft_header(header):
    """deflate_craft's header notation of the inflater's (symbol, extra) pairs"""
    return [s if s < 16 else (s, x + (11 if s == 18 else 3)) for s, x in header]


def test_header_fields_are_what_the_writer_was_asked_for():
    # repeats of every kind, a code-length code with lengths 1..7, HCLEN above what the lengths need, HDIST 2
    header = [(18, 138), 8, (16, 6), (17, 10), 8, (16, 3), (17, 3), (18, 11), 1, 2, 3, 4, 8, (16, 3), (18, 75), 8, 1, 1]
    lens = DC.expand_header(header)
    lit, dist = lens[:257], lens[257:]
    cl = [0] * 19
    for s, l in {8: 1, 16: 2, 18: 3, 17: 4, 1: 5, 2: 6, 3: 7, 4: 7}.items():
        cl[s] = l
    assert DC.canonical(cl)[1] == 1
    tokens = [173, 174, 175, 176, 138, 144, 155, 158, 177, 180, 173]
    s = DC.Stream().dynamic(tokens, lit, dist, final=True, header=header, cl_lens=cl, hclen=19)
    b = DT.member_block(DC.bgzf_member(s.getvalue(), bytes(s.data)))
    assert (b.btype, b.final, b.hlit, b.hdist, b.hclen) == (2, 1, 257, 2, 19)
    assert b.cl_lens == cl and _craft_header(b.header) == header
    assert b.lit_lens == lit and b.dist_lens == dist and b.tokens == tokens and b.bits == s.w.nbits()
    # HLIT 286, HDIST 30, one symbol per length, the default code-length code, copies of 258 and 257 bytes and the farthest distance
    lit, dist = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
    tokens = DC._ramp(32768) + [(258, 32768), 7, (257, 32768), 8, (3, 1), (4, 24577)]
    s = DC.Stream().dynamic(tokens, lit, dist, final=True)
    b = DT.member_block(DC.plain_member(s.getvalue(), bytes(s.data)))
    assert (b.hlit, b.hdist, b.hclen, b.cl_lens) == (286, 30, 19, DC.DEFAULT_CL)
    assert b.header == [(l, 0) for l in lit + dist]
    assert b.tokens == tokens and b.bits == s.w.nbits() and DT.expand(b.tokens) == bytes(s.data)
    # a fixed and a stored block
    s = DC.Stream().fixed(list(b"abc") + [(9, 3)], final=True)
    b = DT.member_block(DC.bgzf_member(s.getvalue(), bytes(s.data)))
    assert (b.btype, b.hlit, b.header, b.tokens, b.bits) == (1, None, None, list(b"abc") + [(9, 3)], s.w.nbits())
    s = DC.Stream().stored(b"stored", final=True)
    b = DT.member_block(DC.bgzf_member(s.getvalue(), bytes(s.data)))
    assert (b.btype, b.tokens, b.bits) == (0, list(b"stored"), 8 * (5 + 6))


@pytest.mark.parametrize("case", [c for c in DC.invalid_cases() if c.zlib_refuses], ids=lambda c: c.name)
def test_the_inflater_refuses_what_zlib_refuses(case):
    with pytest.raises(zlib.error):
        zlib.decompress(case.raw, -15)
    for lenient in (False, True):
        with pytest.raises(DT.DeflateError):
            DT.blocks(case.raw, lenient=lenient)


def test_strict_mode_wants_complete_codes():
    """zlib admits a distance code of no code or of one 1-bit code and a literal code of one 1-bit code; the strict reader does not."""
    by_name = {c.name: c for c in DC.valid_cases()}
    for name, what in [("dynamic_no_distance_code", "distance"), ("dynamic_one_distance_code_hdist1", "distance"),
                       ("dynamic_one_distance_code_hdist5", "distance"), ("dynamic_end_of_block_only", "literal / length")]:
        DT.blocks(by_name[name].raw, lenient=True)
        with pytest.raises(DT.DeflateError, match=f"incomplete {what} code"):
            DT.blocks(by_name[name].raw)
    with pytest.raises(DT.DeflateError, match="before the start"):
        DT.expand([65, (3, 2)])
    two = DC.Stream().fixed([65]).fixed([66], final=True)
    with pytest.raises(DT.DeflateError, match="2 blocks"):
        DT.member_block(DC.bgzf_member(two.getvalue(), bytes(two.data)))


# ---- the references

def _codes(m, longest=5):
    """every vector of m code lengths 1..longest with a Kraft sum of at most 1, and the sums"""
    v = [l for l in itertools.product(range(1, longest + 1), repeat=m) if sum(Fraction(1, 1 << x) for x in l) <= 1]
    return np.array(v), np.array([sum(Fraction(1, 1 << x) for x in l) == 1 for l in v])


def test_min_depth_and_limited_cost_against_brute_force():
    rng = np.random.default_rng(17)
    for m in range(2, 7):
        lens, complete = _codes(m)
        deepest = lens.max(axis=1)
        freqs = [rng.integers(1, 4, m) for _ in range(30)] + [rng.integers(1, 40, m) for _ in range(30)]
        freqs += [np.array([1, 1, 2, 3, 5, 8][:m]), np.array([1, 2, 4, 8, 16, 32][:m]), np.ones(m, np.int64)]
        for f in freqs:
            cost = lens @ f
            best = cost.min()
            # an optimal code is complete; the shallowest of them
            assert B.min_depth(f) == deepest[(cost == best) & complete].min(), f
            for limit in range(1, 6):
                if (1 << limit) < m:
                    continue
                assert B.limited_cost(f, limit) == cost[deepest <= limit].min(), (f, limit)
            assert B.limited_cost(f, 15) == best
            # (unused symbols do not count)
            g = np.concatenate([[0], f, [0]])
            assert B.min_depth(g) == B.min_depth(f) and B.limited_cost(g, 5) == B.limited_cost(f, 5)
    assert (B.min_depth([0, 0]), B.min_depth([0, 9]), B.limited_cost([0, 9], 7)) == (0, 1, 9)
    # the shapes the encoder's tests rely on: steeper than Fibonacci is a chain; limiting it costs bits
    chain = sorted(B.DIST_SKEW_COUNTS.values())
    assert B.min_depth(chain) == 16 and B.limited_cost(chain, 15) > B.limited_cost(chain, 16) == B.limited_cost(chain, 30)


# ---- the generated inputs

def test_inputs_are_deterministic_within_one_block_and_round_trip():
    assert B.dist_skew.__wrapped__(0) == B.dist_skew()
    for seed in B.CL_SKEW_SEEDS:
        assert B.cl_skew.__wrapped__(seed) == B.cl_skew(seed)
    assert B._window_units.__wrapped__() == B._window_units()
    assert [d for _, d in B.few()] == [d for _, d in B.few()]
    cases = B.all_cases()
    assert len({c.name for c in cases}) == len(cases) == 1 + len(B.CL_SKEW_SEEDS) + 3 + 8 + 11
    for c in cases:
        assert 0 < len(c.data) <= B.BLOCK, c.name
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        assert zlib.decompress(z.compress(c.data) + z.flush(), -15) == c.data, c.name
    assert len(B.dist_skew()) == B.DIST_SKEW_PREFIX + 4 * B.DIST_SKEW_COPIES + 1
    assert [len(B.window(P)) for P in B.WINDOW_PERIODS] == [B.BLOCK] * 3
    assert [len(set(d)) for _, d in B.few()] == [1] * 5 + [2] * 5 + [256]


def _distance_histogram(tokens):
    hist = [0] * 30
    for t in tokens:
        if not isinstance(t, int):
            hist[DC.distance_symbol(t[1])[0]] += 1
    return hist


def test_inputs_are_what_they_were_built_to_be_by_the_restated_parse():
    """(the generators' own aim, on the CPU; what the device makes of the inputs is tests/test_gpu_bgzf_limits.py's business)"""
    tokens = B.model_parse(B.dist_skew())
    assert DT.expand(tokens) == B.dist_skew()
    hist = _distance_histogram(tokens)
    assert B.min_depth(hist) > 15 and sum(1 for h in hist if h) >= 17
    assert all(t[0] == 4 for t in tokens if not isinstance(t, int))
    for seed in B.CL_SKEW_SEEDS:
        tokens = B.model_parse(B.cl_skew(seed))
        assert DT.expand(tokens) == B.cl_skew(seed)
        assert sum(not isinstance(t, int) for t in tokens) <= len(tokens) // 1000
    for P in B.WINDOW_PERIODS:
        dists = {t[1] for t in B.model_parse(B.window(P)) if not isinstance(t, int)}
        assert dists == ({P} if P <= B.WINDOW else set()), P
    for n, want in B.RUN_TOKENS.items():
        tokens = B.model_parse(B.runs(n))
        assert tokens[:256] == [0] * 256 and len(tokens) == 256 + len(want)
        at = 256
        for t, w in zip(tokens[256:], want):
            at += 1 if isinstance(t, int) else t[0]
            if w == 0:
                assert t == 0
            else:
                assert t[0] == w[0] and at == w[2] and w[1] in (None, t[1]), (n, t, w)
        assert at == n
