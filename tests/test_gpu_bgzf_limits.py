"""GPU tests of the BGZF encoder (lx_bgzf.hip) at DEFLATE's code-length and window limits: the inputs of tests/bgzf_cases.py, each
member read back token by token with tests/deflate_tokens.py (which refuses an over-subscribed or incomplete code), gzip as the
reference of the round trip, min_depth / limited_cost as the references of the length limit and of what limiting may cost.

The 15-bit limit of the literal / length code is not reached by any input here (the first 256 positions of a block are always
literals, which leaves too few bytes for a chain that deep); the same huffman_lengths routine is driven past its limit through
the distance code (30 symbols, 15 bits) and the code-length code (19 symbols, 7 bits)."""
import gzip
import re
from pathlib import Path

import pytest

from tests import bgzf_cases as B
from tests import deflate_craft as DC
from tests import deflate_tokens as DT
from tests.test_gpu_bgzf import BLOCK, EOF_MEMBER, _contents, _members

pytestmark = pytest.mark.gpu

CASES = {c.name: c.data for c in B.all_cases()}
_HOST = (Path(__file__).resolve().parents[1] / "lambda_amd" / "csrc" / "lx_bgzf_host.cpp").read_text()
CHUNK_BLOCKS = int(re.search(r"kChunkBlocks = (\d+)", _HOST).group(1))  # blocks per launch of lx_bgzf_compress

_encoded = {}


def _encode(handle, name):
    """(the member, its DEFLATE block) of a case, made once"""
    if name not in _encoded:
        out = handle.bgzf_compress(CASES[name])
        _encoded[name] = (out, DT.member_block(out))
    return _encoded[name]


def _copies(block):
    return [t for t in block.tokens if not isinstance(t, int)]


def _distance_histogram(block):
    hist = [0] * 30
    for _, d in _copies(block):
        hist[DC.distance_symbol(d)[0]] += 1
    return hist


def _header_histogram(block):
    hist = [0] * 19
    for s, _ in block.header:
        hist[s] += 1
    return hist


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_round_trips_with_a_valid_code_and_the_size_it_states(handle, name):
    data = CASES[name]
    n = len(data)
    out, block = _encode(handle, name)
    with_eof = handle.bgzf_compress(data, eof=True)
    assert gzip.decompress(out) == data and gzip.decompress(with_eof) == data
    sizes = _members(out, data, False)
    assert _members(with_eof, data, True) == sizes and with_eof == out + EOF_MEMBER
    (size,) = sizes
    assert size == len(out)
    # the strict reader: complete codes (the distance code too), no bits without a symbol, no distance before the start
    assert DT.expand(block.tokens) == data
    assert size <= n + 31  # never larger than stored
    # the bytes one lane counted are the bits 256 lanes wrote: the block ends in the last byte before the trailer
    assert -(-block.bits // 8) == size - 26, (block.bits, size)
    assert handle.bgzf_compress(data) == out


def test_dist_skew_reaches_the_15_bit_limit_of_the_distance_code(handle):
    _, block = _encode(handle, "dist_skew")
    hist = _distance_histogram(block)
    print("dist_skew: distance histogram", hist, "min_depth", B.min_depth(hist), "lengths", block.dist_lens)
    assert block.btype == 2
    assert B.min_depth(hist) > 15  # every optimal code is deeper than 15: the encoder had to limit (else the input is wrong)
    assert max(block.dist_lens) == 15
    assert sum(1 for h in hist if h) >= 17
    assert all((l != 0) == (h != 0) for l, h in zip(block.dist_lens + [0] * 30, hist))


@pytest.mark.parametrize("seed", B.CL_SKEW_SEEDS)
def test_cl_skew_reaches_the_7_bit_limit_of_the_code_length_code(handle, seed):
    _, block = _encode(handle, f"cl_skew_{seed}")
    hist = _header_histogram(block)
    print(f"cl_skew_{seed}: header histogram", hist, "min_depth", B.min_depth(hist), "lengths", block.cl_lens, "copies", len(_copies(block)),
          "of", len(block.tokens))
    assert block.btype == 2
    assert B.min_depth(hist) > 7
    assert max(block.cl_lens) == 7
    assert len(_copies(block)) <= len(block.tokens) // 100


# What the Kraft-sum repair (miniz's heuristic) spends beyond the optimal length-limited code (package-merge) on the limited
# alphabet.  Measured on the device: dist_skew 0 % (28 448 bits, the optimum), cl_skew seed 0 0 % (623 bits), cl_skew seed 2
# 0.161 % (624 bits against 623).  The margin is the next half percent above the measured excess; the encoder is deterministic, so
# the margin only leaves room for a later legitimate change.
SIZE_MARGIN = {"dist_skew": 0.005, "cl_skew_0": 0.005, "cl_skew_2": 0.005}


@pytest.mark.parametrize("name", list(SIZE_MARGIN))
def test_limiting_a_code_costs_little_more_than_package_merge(handle, name):
    _, block = _encode(handle, name)
    if name == "dist_skew":
        hist, lens, limit = _distance_histogram(block), block.dist_lens, 15
    else:
        hist, lens, limit = _header_histogram(block), block.cl_lens, 7
    coded = sum(h * l for h, l in zip(hist, lens))
    best = B.limited_cost(hist, limit)
    print(f"{name}: coded {coded} bits, package-merge {best} bits, excess {100 * (coded / best - 1):.3f} %")
    assert best <= coded <= best * (1 + SIZE_MARGIN[name])


@pytest.mark.parametrize("P", B.WINDOW_PERIODS)
def test_the_window_ends_at_32768(handle, P):
    out, block = _encode(handle, f"window_{P}")
    dists = [d for _, d in _copies(block)]
    print(f"window_{P}: {len(dists)} copies, distances {sorted(set(dists))}")
    if P <= B.WINDOW:
        assert block.btype == 2 and dists and max(dists) == P
    else:
        assert not [d for d in dists if d > B.WINDOW]
        assert block.btype == 0 and len(out) == BLOCK + 31  # nothing within reach repeats: stored, like random bytes


@pytest.mark.parametrize("n", list(B.RUN_TOKENS))
def test_match_lengths_at_258_and_at_the_end_of_the_block(handle, n):
    _, block = _encode(handle, f"runs_{n}")
    want = B.RUN_TOKENS[n]
    assert block.btype == 2 and block.tokens[:256] == [0] * 256
    tail = block.tokens[256:]
    assert len(tail) == len(want), tail
    at = 256
    for t, w in zip(tail, want):
        at += 1 if isinstance(t, int) else t[0]
        if w == 0:
            assert t == 0, tail
        else:
            length, distance, end = w
            assert not isinstance(t, int) and t[0] == length and at == end and distance in (None, t[1]), tail
    assert at == n
    # 258 is symbol 285 without extra bits, 257 symbol 284 with extra bits 30: both must be in the code when they occur
    for length, symbol in ((258, 285), (257, 284)):
        if any(t[0] == length for t in _copies(block)):
            assert block.hlit > symbol and block.lit_lens[symbol] > 0


@pytest.mark.parametrize("name", ["runs_259", "few_two_values_256", "runs_260"])
def test_a_distance_code_of_fewer_than_two_symbols_gets_company(handle, name):
    """No copy at all (259 zeros, 256 bytes: all within the first 256 positions but the unhashed tail) or copies at one distance:
    the dynamic block still states a complete distance code."""
    _, block = _encode(handle, name)
    assert block.btype == 2 and len(set(DC.distance_symbol(d)[0] for _, d in _copies(block))) == (1 if name == "runs_260" else 0)
    assert DC.canonical(block.dist_lens)[1] == 1 and DC.canonical(block.lit_lens)[1] == 1


@pytest.mark.parametrize("extra", [0, 1])
def test_an_input_that_ends_on_the_border_of_a_launch(handle, extra):
    """kChunkBlocks whole blocks are one launch; one byte more is a second launch of one block of one byte."""
    n = CHUNK_BLOCKS * BLOCK + extra
    data = _contents("period", n)
    out = handle.bgzf_compress(data, eof=True)
    ms, launches = handle.last_phase_ms(4)
    assert launches == 1 + extra
    assert gzip.decompress(out) == data
    sizes = _members(out, data, True)
    assert len(sizes) == CHUNK_BLOCKS + extra
    if extra:
        assert sizes[-1] == 1 + 31
