"""A test-side DEFLATE (RFC 1951) writer: streams built on purpose, bit by bit, for the decoder's tests.  It never calls the library.

`Stream` writes stored, fixed and dynamic blocks from explicit tokens, code lengths and code-length symbols, and keeps the bytes the
tokens stand for, so that every case carries its expectation; tests/test_inflate_cases.py holds each VALID case against
`zlib.decompress(raw, -15)`, which is the reference.  `bgzf_member` / `plain_member` wrap one stream as one gzip member.
`VALID` and `INVALID` are the corpora, lists of named cases; `mutants()` is the
deterministic differential corpus: zlib streams with one or two flipped bits.

Tokens of a fixed or dynamic block:
    65                        a literal
    (length, distance)        a copy, in the usual (smallest) symbols
    ("L", lsym, lextra, dsym, dextra)   a copy in explicit symbols and extra-bit values (284 + extra 31 = length 258)
    ("sym", s) / ("dsym", s)  a raw symbol of the literal / length code or of the distance code (nothing is added to the output)
    ("bits", value, count)    raw bits
"""
from __future__ import annotations

import struct
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# a complete code-length code over all 19 symbols: 13 of 4 bits, 6 of 5 bits
DEFAULT_CL = [4] * 13 + [5] * 6

# the decoder's texts (lx::inflate::status_text and the device path's wrapper checks in lx_gunzip_host.cpp)
TRUNCATED = "truncated DEFLATE stream"
BAD_TYPE = "reserved block type"
BAD_STORED = "stored block length does not match its complement"
BAD_LENGTHS = "invalid code lengths"
BAD_CODE = "invalid Huffman code"
BAD_SYMBOL = "invalid length or distance symbol"
TOO_FAR = "distance before the start of the output"
FULL = "more output than the member's ISIZE"
W_ISIZE = "ISIZE mismatch (the DEFLATE stream ends early)"
W_TRAILING = "BSIZE does not match the member's DEFLATE stream"
W_CRC = "CRC32 mismatch"
STATUS_TEXTS = [None, TRUNCATED, BAD_TYPE, BAD_STORED, BAD_LENGTHS, BAD_CODE, BAD_SYMBOL, TOO_FAR, FULL]  # by inflate::Status


class BitWriter:
    """Bits into bytes, least significant bit first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        assert 0 <= value < (1 << count) or count == 0
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code: its most significant bit goes first."""
        for b in range(length - 1, -1, -1):
            self.bits((code >> b) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def nbits(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        """The bytes so far, the last one padded with zero bits."""
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """The canonical codes of a list of code lengths (0 = no code): ({symbol: (code, length)}, Kraft sum).  The sum is 1 for a
    complete code, above 1 for an over-subscribed one; the codes of such a set are still written as the counts give them."""
    kraft = sum((Fraction(1, 1 << l) for l in lengths if l), Fraction(0))
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = {}
    for s, l in enumerate(lengths):
        if l:
            codes[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return codes, kraft


def length_symbol(length):
    s = max(i for i in range(29) if LBASE[i] <= length) if length < 258 else 28
    return 257 + s, length - LBASE[s]


def distance_symbol(dist):
    s = max(i for i in range(30) if DBASE[i] <= dist)
    return s, dist - DBASE[s]


def plain_header(lit_lens, dist_lens):
    """The code lengths as header symbols, one per length, no repeats."""
    return list(lit_lens) + list(dist_lens)


def expand_header(header):
    """The code lengths a header sequence stands for: n, (16, times), (17, times), (18, times)."""
    out = []
    for h in header:
        if isinstance(h, int):
            out.append(h)
        elif h[0] == 16:
            out += [out[-1]] * h[1]
        else:
            out += [0] * h[1]
    return out


class Stream:
    """One DEFLATE stream in the making; .data is what its tokens stand for so far."""

    def __init__(self):
        self.w = BitWriter()
        self.data = bytearray()

    def getvalue(self):
        return self.w.getvalue()

    # ---- raw hooks
    def bits(self, value, count):
        self.w.bits(value, count)
        return self

    def block_header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)
        return self

    # ---- blocks
    def stored(self, payload, final=False, len_=None, nlen=None):
        self.block_header(final, 0)
        self.w.align()
        n = len(payload) if len_ is None else len_
        self.w.bits(n, 16)
        self.w.bits((~n & 0xFFFF) if nlen is None else nlen, 16)
        self.w.raw(payload)
        self.data += payload
        return self

    def _tokens(self, tokens, lit, dist, eob):
        w = self.w
        for t in tokens:
            if isinstance(t, int):
                w.code(*lit[t])
                self.data.append(t)
                continue
            if t[0] == "sym":
                w.code(*lit[t[1]])
            elif t[0] == "dsym":
                w.code(*dist[t[1]])
            elif t[0] == "bits":
                w.bits(t[1], t[2])
            else:
                if t[0] == "L":
                    _, ls, lx, ds, dx = t
                else:
                    (ls, lx), (ds, dx) = length_symbol(t[0]), distance_symbol(t[1])
                length, d = LBASE[ls - 257] + lx, DBASE[ds] + dx
                w.code(*lit[ls])
                w.bits(lx, LEXTRA[ls - 257])
                w.code(*dist[ds])
                w.bits(dx, DEXTRA[ds])
                assert 1 <= d <= len(self.data), "a copy from before the output: write it with raw symbols"
                for _ in range(length):
                    self.data.append(self.data[-d])
        if eob:
            w.code(*lit[256])

    def fixed(self, tokens, final=False, eob=True):
        self.block_header(final, 1)
        self._tokens(tokens, canonical(FIXED_LIT)[0], canonical(FIXED_DIST)[0], eob)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, cl_lens=None, header=None, hlit=None, hdist=None, hclen=None, eob=True):
        """lit_lens / dist_lens give the codes the tokens are written in.  `header` is the sequence of code-length symbols that
        states them: a length 0..15, or (16, times), (17, times), (18, times), or ("raw", symbol, extra value, extra bits); the
        default is one symbol per length.  cl_lens are the 19 lengths of the code-length code (by symbol, not in transmission
        order); hlit / hdist / hclen are the counts as the header states them (257.., 1.., 4..)."""
        cl_lens = list(DEFAULT_CL if cl_lens is None else cl_lens)
        header = plain_header(lit_lens, dist_lens) if header is None else header
        hlit = len(lit_lens) if hlit is None else hlit
        hdist = len(dist_lens) if hdist is None else hdist
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        w = self.w
        self.block_header(final, 2)
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lens[s], 3)
        cl = canonical(cl_lens)[0]
        for h in header:
            if isinstance(h, int):
                w.code(*cl[h])
            elif h[0] == "raw":
                w.code(*cl[h[1]])
                w.bits(h[2], h[3])
            else:
                sym, times = h
                w.code(*cl[sym])
                w.bits(times - (11 if sym == 18 else 3), 7 if sym == 18 else 3 if sym == 17 else 2)
        self._tokens(tokens, canonical(lit_lens)[0], canonical(dist_lens)[0], eob)
        return self


# ---- members

def _gzip_header(flg, extra, fname):
    h = struct.pack("<BBBBIBB", 0x1F, 0x8B, 8, flg | (4 if extra else 0) | (8 if fname else 0), 0, 0, 0xFF)
    if extra:
        h += struct.pack("<H", len(extra)) + extra
    if fname:
        h += fname + b"\0"
    return h


def bgzf_member(raw, data, isize=None, crc=None, extra_before=b"", extra_after=b"", fname=b""):
    """One DEFLATE stream as one BGZF member: the BC subfield (with other subfields before and after it, given whole) states the
    member's size; the trailer is the CRC32 and length of `data` unless given."""
    xlen = len(extra_before) + 6 + len(extra_after)
    total = 10 + 2 + xlen + (len(fname) + 1 if fname else 0) + len(raw) + 8
    assert total <= 65536, total
    extra = extra_before + struct.pack("<BBHH", ord("B"), ord("C"), 2, total - 1) + extra_after
    m = _gzip_header(0, extra, fname) + raw + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)
    assert len(m) == total
    return m


def plain_member(raw, data, isize=None, crc=None):
    return _gzip_header(0, b"", b"") + raw + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


Valid = namedtuple("Valid", "name raw data")
# raw: the DEFLATE stream; data / isize / crc: what the member's trailer is made from (isize is the device sink's capacity);
# texts: what the device path must say (exactly one, two only in the truncation group); zlib_refuses: zlib refuses `raw` itself;
# group: a block type / stored, b truncation, c lengths, d codes, e symbols, f distances, g output past ISIZE, h wrapper
class Invalid(namedtuple("Invalid", "name group raw data isize crc texts zlib_refuses")):
    def member(self, **kw):
        """The case as one BGZF member."""
        return bgzf_member(self.raw, self.data, isize=self.isize, crc=self.crc, **kw)


def _rng_bytes(n, seed):
    return np.random.default_rng(seed).bytes(n)


def _ramp(upto):
    """Tokens for `upto` bytes of period 256 (0, 1, .. 255, 0, ..): 256 literals, then copies at distance 256."""
    assert upto >= 256
    t, n = list(range(256)), 256
    while upto - n >= 3:
        k = min(258, upto - n)
        if upto - n - k in (1, 2):
            k -= 3
        t.append((k, 256))
        n += k
    assert n == upto
    return t


def _lens(n, pairs):
    v = [0] * n
    for s, l in pairs.items():
        v[s] = l
    return v


STAIRS = list(range(1, 15)) + [15, 15]  # 1, 2, .. 14, 15, 15: complete, with two 15-bit codes


def _build_valid():
    V = []

    def add(name, s):
        V.append(Valid(name, s.getvalue(), bytes(s.data)))

    # ---- stored blocks
    add("stored_len0_final", Stream().stored(b"", final=True))
    add("stored_len0_then_fixed", Stream().stored(b"").fixed(list(b"sync"), final=True))
    # 3 + 2 * 8 + 7 bits of fixed block: it ends on bit 2 of byte 3; the decoder's bit buffer then holds the bytes that follow
    add("stored_after_fixed_mid_byte", Stream().fixed(list(b"ab")).stored(b"whole bytes wait in the bit buffer", final=True))
    add("stored_len65505", Stream().stored(_rng_bytes(65505, 1), final=True))
    # ---- fixed blocks
    add("fixed_every_literal", Stream().fixed(list(range(256)), final=True))
    t = list(b"xyz")
    for ls in range(257, 286):
        for lx in sorted({0, (1 << LEXTRA[ls - 257]) - 1}):
            t += [("L", ls, lx, 0, 0), ord("a") + ls % 26]  # (a fresh literal after each, so that a wrong length shows)
    add("fixed_every_length_symbol", Stream().fixed(t, final=True))
    t = _ramp(32768)
    for ds in range(30):
        for dx in sorted({0, (1 << DEXTRA[ds]) - 1}):
            t += [("L", 257, 0, ds, dx), (ds * 7 + dx) & 0xFF]
    add("fixed_every_distance_symbol", Stream().fixed(t, final=True))
    add("fixed_distance_32768_at_32768", Stream().fixed(_ramp(32768) + [(3, 32768), 33, (4, 32768)], final=True))
    # ---- copies
    add("copy_distance1_length258", Stream().fixed([ord("a"), (258, 1), ord("b")], final=True))
    add("copy_distance2_length3", Stream().fixed([ord("a"), ord("b"), (3, 2)], final=True))
    add("copy_distance_equals_position", Stream().fixed(list(b"abcdefg") + [(5, 7), (12, 12)], final=True))
    s = Stream().fixed(_ramp(65536 - 258) + [(258, 255)], final=True)
    assert len(s.data) == 65536
    add("copy_258_ends_on_65536", s)
    # ---- dynamic blocks: code lengths
    lit_syms = [ord("e"), ord("t"), ord("a"), 256, 257, ord("o"), ord("n"), 258, ord("i"), ord("s"), ord("r"), ord("h"), 285, ord("l"),
                ord("d"), ord("u")]  # lengths 1, 2, .. 14, 15, 15 in this order
    lit = _lens(286, dict(zip(lit_syms, STAIRS)))
    dist = STAIRS[:]  # distance symbols 0..15
    t = [ord("e")] * 300 + [s_ for s_ in lit_syms if s_ < 256]
    for ds in range(16):
        t += [("L", 257, 0, ds, 0), ord("d"), ("L", 258, 0, ds, (1 << DEXTRA[ds]) - 1), ord("u")]
    t += [("L", 285, 0, 15, 63), ord("d"), ord("u")]
    add("dynamic_lengths_1_to_15", Stream().dynamic(t, lit, dist, final=True))
    ten = list(range(1, 11)) + [11, 11]  # 1 .. 10, 11, 11
    lit = _lens(258, dict(zip([ord(c) for c in "abcdefgh"] + [256, 257, ord("y"), ord("z")], ten)))
    dist = ten[:]
    t = list(b"abcdefghyz" * 8) + [("L", 257, 0, 9, 0), ord("y"), ("L", 257, 0, 10, 0), ord("z"), ("L", 257, 0, 11, 0), ("L", 257, 0, 8, 0)]
    add("dynamic_codes_of_10_and_11_bits", Stream().dynamic(t, lit, dist, final=True))
    lit = _lens(257, {ord("a"): 1, ord("b"): 2, 256: 2})
    add("dynamic_hlit257_hdist1", Stream().dynamic(list(b"abba"), lit, [0], final=True))
    lit = [8] * 226 + [9] * 60
    dist = [4] * 2 + [5] * 28
    t = _ramp(24577 + 300) + [("L", 285, 0, 29, 0), 7, ("L", 284, 31, 29, 300), 8, ("L", 280, 15, 0, 0)] + list(range(200, 256))
    add("dynamic_hlit286_hdist30", Stream().dynamic(t, lit, dist, final=True))
    cl = _lens(19, {0: 1, 3: 2, 1: 3, 2: 4, 4: 5, 5: 6, 6: 7, 7: 7})
    lit = _lens(258, {ord("a"): 1, ord("b"): 2, ord("c"): 3, ord("d"): 4, ord("e"): 5, ord("f"): 6, 256: 7, 257: 7})
    add("dynamic_code_length_code_of_7_bits", Stream().dynamic(list(b"fedcbaabcdef") + [(3, 2)], lit, [1, 1], final=True, cl_lens=cl))
    # ---- dynamic blocks: distance and literal trees
    lit = _lens(257, {ord("n"): 1, ord("o"): 2, 256: 2})
    add("dynamic_no_distance_code", Stream().dynamic(list(b"noon"), lit, [0], final=True))
    lit = _lens(258, {ord("a"): 1, 257: 2, 256: 2})
    add("dynamic_one_distance_code_hdist1", Stream().dynamic([ord("a"), (3, 1), ord("a"), (3, 1)], lit, [1], final=True))
    add("dynamic_one_distance_code_hdist5",
        Stream().dynamic(list(b"aaaaaa") + [("L", 257, 0, 4, 0), ord("a"), ("L", 257, 0, 4, 1)], lit, [0, 0, 0, 0, 1], final=True))
    add("dynamic_end_of_block_only", Stream().dynamic([], _lens(257, {256: 1}), [0], final=True))
    add("dynamic_one_literal_and_end_of_block", Stream().dynamic(list(b"xxxxx"), _lens(257, {ord("x"): 1, 256: 1}), [0], final=True))
    # ---- dynamic blocks: repeats.  16 x3 and x6, 17 x3 and x10, 18 x11 and x138, all in the literal lengths:
    header = [(18, 138), 8, (16, 6), (17, 10), 8, (16, 3), (17, 3), (18, 11), 1, 2, 3, 4, 8, (16, 3), (18, 75), 8, 1, 1]
    lens = expand_header(header)
    lit, dist = lens[:257], lens[257:]
    t = [173, 174, 175, 176, 138, 144, 155, 158, 177, 180, 173]
    add("dynamic_repeats_16_17_18_smallest_and_largest", Stream().dynamic(t, lit, dist, final=True, header=header))
    # a 16 that starts in the literal lengths (255, 256, 257), runs on into the distance lengths, and a second one that ends exactly
    # on the last of them (258 + 8 lengths)
    header = [(18, 65), 1, (18, 138), (18, 50), 3, (16, 6), (16, 5)]
    lens = expand_header(header)
    lit, dist = lens[:258], lens[258:]
    assert len(dist) == 8
    t = [65, 254, 255, 65] * 4 + [("L", 257, 0, 0, 0), ("L", 257, 0, 7, 1), ("L", 257, 0, 3, 0)]
    add("dynamic_repeat_from_literal_into_distance_lengths", Stream().dynamic(t, lit, dist, final=True, header=header))
    # an 18 that covers the unused length symbols 257..261 and the first six distance lengths
    header = [(18, 97), 1, 2, (18, 137), (18, 20), 2, (18, 11), 1]
    lens = expand_header(header)
    lit, dist = lens[:262], lens[262:]
    assert len(dist) == 7
    add("dynamic_zero_repeat_from_literal_into_distance_lengths", Stream().dynamic([97, 98, 97], lit, dist, final=True, header=header))
    # ---- several blocks in one stream
    s = Stream().stored(b">seq1 several blocks\n").fixed(list(b"ACGTACGT") + [(8, 4), ord("\n")])
    lit = [8] * 226 + [9] * 60
    dist = [4] * 2 + [5] * 28
    s.dynamic(list(range(32, 127)) + [(20, 30), (258, 95), 285 - 256, ("L", 285, 0, 11, 3)], lit, dist)
    # the second dynamic block: 1-, 2- and 3-bit codes over fewer symbols; its copies reach into the blocks before it
    lit = _lens(258, {ord("A"): 1, ord("C"): 2, 257: 3, 256: 3})
    n0 = len(s.data)
    s.dynamic([ord("A"), ord("C"), ("L", 257, 0, 1, 0), ord("A"), ("L", 257, 0, 0, 0)], lit, [1, 1])
    assert n0 > 100
    s.fixed([(30, n0), (5, len(s.data) + 30 - 3)])
    s.fixed([], final=True)
    add("several_blocks_stored_fixed_dynamic_dynamic_empty", s)
    return V


def _build_invalid():
    I = []

    def add(name, group, s, texts, zlib_refuses=True, isize=None, crc=None, raw=None, slack=3):
        raw = s.getvalue() if raw is None else raw
        data = bytes(s.data)
        # (cases refused inside the stream: room for what was written so far and a little more, so that the sink is not the one
        # that refuses)
        I.append(Invalid(name, group, raw, data, len(data) + slack if isize is None else isize, crc,
                         (texts,) if isinstance(texts, str) else tuple(texts), zlib_refuses))

    pad = ("bits", 0, 24)  # bits behind the point of failure: the decoder's answer must not depend on the stream ending there
    ok_lit = _lens(258, {ord("a"): 1, 257: 2, 256: 2})
    # ---- a: block type and stored blocks
    add("block_type_3", "a", Stream().fixed(list(b"ab")).block_header(True, 3).bits(0, 21), BAD_TYPE)
    add("stored_len_not_complement_of_nlen", "a", Stream().stored(b"abcd", final=True, nlen=0xFFFA), BAD_STORED, slack=0)
    add("stored_len_past_the_input", "a", Stream().stored(b"abcde", final=True, len_=6), TRUNCATED, isize=6)
    # ---- b: truncation (two texts allowed: the bits that are missing may read as a code that does not exist)
    either = (TRUNCATED, BAD_CODE)
    lit = [8] * 226 + [9] * 60
    dist = [4] * 2 + [5] * 28
    whole = Stream().dynamic(list(b"hello, hello") + [(5, 7)], lit, dist, final=True)
    add("cut_after_the_block_header", "b", whole, either, raw=whole.getvalue()[:1])
    add("cut_inside_the_dynamic_header", "b", whole, either, raw=whole.getvalue()[:40])
    s = Stream().fixed([ord("a"), 200], final=True, eob=False)  # 3 + 8 + 9 bits: two bytes hold five bits of the last code
    add("cut_inside_a_symbol", "b", s, either, raw=s.getvalue()[:2])
    # 3 + 3 * 9 + 8 bits up to the end of length symbol 284: five bytes hold two of its five extra bits
    s = Stream().fixed([200, 201, 202, ("sym", 284), ("bits", 0, 5)], final=True, eob=False)
    assert s.w.nbits() == 43
    add("cut_inside_extra_bits", "b", s, either, raw=s.getvalue()[:5])
    add("no_final_block", "b", Stream().fixed(list(b"abc")).stored(b"def"), either, slack=0)
    # ---- c: bad lengths
    add("hlit_287", "c", Stream().dynamic([], [8] * 226 + [9] * 60, [1, 1], final=True, hlit=287), BAD_LENGTHS)
    add("hdist_31", "c", Stream().dynamic([], ok_lit, [5] * 30, final=True, hdist=31), BAD_LENGTHS)
    add("repeat_16_as_the_first_length", "c", Stream().dynamic([], ok_lit, [1], final=True, header=[(16, 3)] + [0] * 300), BAD_LENGTHS)
    header = [(18, 97), 1, (18, 138), (18, 20), 2, (16, 3)]  # 258 + 1 lengths stated; the last repeat would end on 260
    add("repeat_overruns_by_one", "c", Stream().dynamic([], ok_lit, [1], final=True, header=header + [0] * 8), BAD_LENGTHS)
    # ---- d: bad codes
    cl = _lens(19, {0: 1, 1: 1, 2: 1})
    assert canonical(cl)[1] > 1
    add("code_length_code_over_subscribed", "d", Stream().dynamic([], ok_lit, [1], final=True, cl_lens=cl, header=[0] * 300), BAD_CODE)
    cl = _lens(19, {0: 1, 1: 2, 2: 3})
    assert canonical(cl)[1] < 1
    header = [0] * 97 + [1] + [0] * 158 + [2, 2, 1]
    add("code_length_code_incomplete", "d", Stream().dynamic([pad], ok_lit, [1], final=True, cl_lens=cl, header=header), BAD_CODE)
    lit = _lens(257, {ord("a"): 1, ord("b"): 1, 256: 1})
    add("literal_code_over_subscribed", "d", Stream().dynamic([pad], lit, [1], final=True, eob=False), BAD_CODE)
    add("distance_code_over_subscribed", "d", Stream().dynamic([pad], ok_lit, [1, 1, 1], final=True, eob=False), BAD_CODE)
    lit = _lens(257, {ord("a"): 2, 256: 2})
    add("literal_code_incomplete_two_codes", "d", Stream().dynamic([pad], lit, [1], final=True, eob=False), BAD_CODE)
    lit = _lens(257, {ord("a"): 1, ord("b"): 2, 256: 3})
    add("literal_code_incomplete_three_codes", "d", Stream().dynamic([pad], lit, [1], final=True, eob=False), BAD_CODE)
    lit = _lens(257, {ord("a"): 1})
    add("literal_code_incomplete_one_literal_no_end_of_block", "d", Stream().dynamic([pad], lit, [1], final=True, eob=False), BAD_CODE)
    add("distance_code_incomplete_two_codes", "d", Stream().dynamic([pad], ok_lit, [2, 2], final=True, eob=False), BAD_CODE)
    lit = _lens(257, {ord("a"): 1, ord("b"): 1})
    add("no_end_of_block_code", "d", Stream().dynamic([pad], lit, [1], final=True, eob=False), BAD_CODE)
    add("unused_half_of_a_one_code_distance_tree", "d",
        Stream().dynamic([ord("a"), ("sym", 257), ("bits", 1, 1), pad], ok_lit, [1], final=True), BAD_CODE)
    add("unused_half_of_a_one_code_literal_tree", "d", Stream().dynamic([("bits", 1, 1), pad], _lens(257, {256: 1}), [0], final=True, eob=False),
        BAD_CODE)
    add("length_symbol_with_an_empty_distance_tree", "d", Stream().dynamic([ord("a"), ("sym", 257), pad], ok_lit, [0], final=True), BAD_CODE)
    # ---- e: bad symbols
    for sym in (286, 287):
        add(f"fixed_symbol_{sym}", "e", Stream().fixed(list(b"ab") + [("sym", sym), pad], final=True), BAD_SYMBOL)
    for sym in (30, 31):
        add(f"distance_symbol_{sym}", "e", Stream().fixed(list(b"ab") + [("sym", 257), ("dsym", sym), pad], final=True), BAD_SYMBOL)
    # ---- f: distances before the start of the output
    add("distance_1_at_position_0", "f", Stream().fixed([("sym", 257), ("dsym", 0), pad], final=True), TOO_FAR)
    d, x = distance_symbol(1001)
    add("distance_1001_at_position_1000", "f",
        Stream().fixed(_ramp(1000) + [("sym", 257), ("dsym", d), ("bits", x, DEXTRA[d]), pad], final=True), TOO_FAR)
    add("distance_32768_at_position_32767", "f",
        Stream().fixed(_ramp(32767) + [("sym", 257), ("dsym", 29), ("bits", 8191, 13), pad], final=True), TOO_FAR)
    # ---- g: output past ISIZE (the streams are valid: zlib accepts them)
    s = Stream().fixed(list(b"abcdef"), final=True)
    add("literal_past_isize", "g", s, FULL, zlib_refuses=False, isize=len(s.data) - 1)
    s = Stream().fixed(list(b"abc") + [(9, 3)], final=True)
    add("copy_one_byte_too_long", "g", s, FULL, zlib_refuses=False, isize=len(s.data) - 1)
    s = Stream().fixed(_ramp(65536 - 258) + [(258, 255)], final=True)
    add("copy_258_one_byte_past_65535", "g", s, FULL, zlib_refuses=False, isize=65535)
    s = Stream().stored(b"a stored block", final=True)
    add("stored_block_past_isize", "g", s, FULL, zlib_refuses=False, isize=len(s.data) - 1)
    s = Stream().fixed(list(b"ab")).stored(b"a stored block from the bit buffer", final=True)
    add("stored_block_from_the_bit_buffer_past_isize", "g", s, FULL, zlib_refuses=False, isize=4)
    # ---- h: the wrapper
    s = Stream().fixed(list(b"abc") + [(9, 3)], final=True)
    add("output_one_byte_short_of_isize", "h", s, W_ISIZE, zlib_refuses=False, isize=len(s.data) + 1)
    add("spare_byte_before_the_trailer", "h", s, W_TRAILING, zlib_refuses=False, isize=len(s.data), raw=s.getvalue() + b"\0")
    add("right_length_wrong_crc", "h", s, W_CRC, zlib_refuses=False, isize=len(s.data), crc=zlib.crc32(bytes(s.data)) ^ 0x80000000)
    return I


VALID = _build_valid()
INVALID = _build_invalid()
_cache = {}


def valid_cases():
    return VALID


def invalid_cases():
    return INVALID


# ---- the differential corpus: zlib's own streams with one or two flipped bits

Mutant = namedtuple("Mutant", "raw true_len accepted data consumed")  # data / consumed: zlib's, when it accepts

N_MUTANTS = 30000


def _fasta(n, rng):
    out = []
    while sum(map(len, out)) < n:
        out.append(b">s%d\n" % len(out) + bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), 48).tolist()) + b"\n")
    return b"".join(out)[:n]


def seeds():
    """35 zlib streams: five inputs by seven level / strategy settings, each with a full flush in the middle."""
    rng = np.random.default_rng(20240607)
    inputs = [_fasta(700, rng), rng.bytes(200), b"ACGT" * 150 + b"N" * 300, bytes(rng.choice(list(b"ab"), 400).tolist()),
              _fasta(120, rng) + rng.bytes(60) + b"\0" * 100]
    settings = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)]
    out = []
    for data in inputs:
        for level, strategy in settings:
            c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
            raw = c.compress(data[:len(data) // 2]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[len(data) // 2:]) + c.flush()
            out.append((raw, data))
    return out


def zlib_verdict(raw):
    """(accepted, zlib's bytes, bytes it consumed) of one raw stream."""
    d = zlib.decompressobj(-15)
    try:
        data = d.decompress(raw)
    except zlib.error:
        return False, None, None
    if not d.eof:
        return False, None, None
    return True, data, len(raw) - len(d.unused_data)


def mutants():
    """The 35 seeds and N_MUTANTS streams with one or two flipped bits (60 % of the flips in the first 40 bytes), with zlib's
    verdict on each.  Deterministic: fixed numpy seeds."""
    if "M" in _cache:
        return _cache["M"]
    S = seeds()
    rng = np.random.default_rng(977)
    out = []
    for raw, data in S:
        out.append(Mutant(raw, len(data), *zlib_verdict(raw)))
        assert out[-1].accepted and out[-1].data == data
    for _ in range(N_MUTANTS):
        raw, data = S[int(rng.integers(len(S)))]
        b = bytearray(raw)
        for _k in range(int(rng.integers(1, 3))):
            span = min(40, len(b)) if rng.random() < 0.6 else len(b)
            b[int(rng.integers(span))] ^= 1 << int(rng.integers(8))
        out.append(Mutant(bytes(b), len(data), *zlib_verdict(bytes(b))))
    _cache["M"] = out
    return out
