"""A test-side DEFLATE (RFC 1951) reader that keeps what a decompressor throws away: per block the header fields, the code-length
code, the run-length symbols of the header, the two codes' lengths, the tokens and the number of bits read.  It never calls the
library; tests/test_bgzf_cases.py holds it against `zlib.decompress(raw, -15)` and against what tests/deflate_craft.py was asked to
write.  The encoder's tests (tests/test_gpu_bgzf_limits.py) read the device's members with it.

Strict by default: every Huffman code must be complete (Kraft sum exactly 1), the distance code too, also in a block without a
copy.  `lenient=True` admits the two incomplete codes zlib admits: a literal / length or distance code of a single 1-bit code, and
a distance code without any code.  Either way it raises DeflateError on an over-subscribed or incomplete code, on bits that are no
code of a symbol, on a symbol that stands for nothing (286, 287, 30, 31), on a distance that reaches before the start of the
output, and on a stream that ends early.
"""
from __future__ import annotations

import struct
from collections import namedtuple

from tests.deflate_craft import CL_ORDER, DBASE, DEXTRA, FIXED_DIST, FIXED_LIT, LBASE, LEXTRA, canonical

# btype 0 / 1: hlit, hdist, hclen, cl_lens, header are None (lit_lens / dist_lens too for a stored block, whose tokens are its bytes).
# header: (symbol, extra) pairs, extra as the bits state it (16: times - 3, 17: times - 3, 18: times - 11, a length: 0).
# tokens: an int literal or (length, distance).  bits: read from the start of the stream up to the end of this block.
Block = namedtuple("Block", "btype final hlit hdist hclen cl_lens header lit_lens dist_lens tokens bits")


class DeflateError(ValueError):
    pass


class _Bits:
    def __init__(self, raw):
        self.raw = bytes(raw)
        self.pos = 0
        self.end = 8 * len(self.raw)

    def peek(self, count):
        """the next `count` (<= 24) bits, zeros behind the end"""
        p = self.pos
        return (int.from_bytes(self.raw[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << count) - 1)

    def skip(self, count):
        self.pos += count
        if self.pos > self.end:
            raise DeflateError("the stream ends inside a block")

    def take(self, count):
        v = self.peek(count)
        self.skip(count)
        return v


class _Code:
    """A canonical Huffman code as a table over the next `width` bits (LSB first)."""

    def __init__(self, lengths, what, lenient=False):
        codes, kraft = canonical(list(lengths))
        self.what = what
        if kraft > 1:
            raise DeflateError(f"over-subscribed {what} code")
        if kraft < 1:
            one_bit = len(codes) == 1 and next(iter(codes.values()))[1] == 1
            if not (lenient and (one_bit or (not codes and what == "distance"))):
                raise DeflateError(f"incomplete {what} code")
        self.width = max([l for _, l in codes.values()], default=1)
        self.table = [None] * (1 << self.width)
        for s, (c, l) in codes.items():
            rev = int(format(c, f"0{l}b")[::-1], 2)
            for j in range(rev, 1 << self.width, 1 << l):
                self.table[j] = (s, l)

    def read(self, b):
        e = self.table[b.peek(self.width)]
        if e is None:
            raise DeflateError(f"bits that are no code of the {self.what} code")
        b.skip(e[1])
        return e[0]


def _read_tokens(b, lit, dist, tokens, produced):
    while True:
        s = lit.read(b)
        if s < 256:
            tokens.append(s)
            produced += 1
            continue
        if s == 256:
            return produced
        if s > 285:
            raise DeflateError(f"length symbol {s}")
        length = LBASE[s - 257] + b.take(LEXTRA[s - 257])
        d = dist.read(b)
        if d > 29:
            raise DeflateError(f"distance symbol {d}")
        distance = DBASE[d] + b.take(DEXTRA[d])
        if distance > produced:
            raise DeflateError(f"distance {distance} at position {produced}: before the start of the output")
        tokens.append((length, distance))
        produced += length


def _dynamic_header(b, lenient):
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if hlit > 286 or hdist > 30:
        raise DeflateError(f"HLIT {hlit} / HDIST {hdist}")
    cl_lens = [0] * 19
    for s in CL_ORDER[:hclen]:
        cl_lens[s] = b.take(3)
    cl = _Code(cl_lens, "code-length")  # (zlib admits no incomplete code here)
    header, lens = [], []
    while len(lens) < hlit + hdist:
        s = cl.read(b)
        if s < 16:
            header.append((s, 0))
            lens.append(s)
            continue
        x = b.take(2 if s == 16 else 3 if s == 17 else 7)
        header.append((s, x))
        if s == 16 and not lens:
            raise DeflateError("a repeat of the previous length as the first length")
        times = x + (11 if s == 18 else 3)
        if len(lens) + times > hlit + hdist:
            raise DeflateError("a repeat runs beyond the stated lengths")
        lens += [lens[-1] if s == 16 else 0] * times
    lit_lens, dist_lens = lens[:hlit], lens[hlit:]
    if lit_lens[256] == 0:
        raise DeflateError("no code for the end of the block")
    return hlit, hdist, hclen, cl_lens, header, lit_lens, dist_lens


def blocks(raw, lenient=False):
    """The blocks of one raw DEFLATE stream, up to and including its final block."""
    b, out, produced = _Bits(raw), [], 0
    while True:
        final, btype = b.take(1), b.take(2)
        if btype == 3:
            raise DeflateError("reserved block type")
        if btype == 0:
            b.skip(-b.pos % 8)
            n, nn = b.take(16), b.take(16)
            if n != (~nn & 0xFFFF):
                raise DeflateError("stored block length does not match its complement")
            at = b.pos // 8
            b.skip(8 * n)
            out.append(Block(0, final, None, None, None, None, None, None, None, list(b.raw[at:at + n]), b.pos))
            produced += n
        else:
            if btype == 1:
                fields = (None, None, None, None, None, list(FIXED_LIT), list(FIXED_DIST))
                lit, dist = _Code(FIXED_LIT, "literal / length"), _Code(FIXED_DIST, "distance")
            else:
                fields = _dynamic_header(b, lenient)
                lit, dist = _Code(fields[5], "literal / length", lenient), _Code(fields[6], "distance", lenient)
            tokens = []
            produced = _read_tokens(b, lit, dist, tokens, produced)
            out.append(Block(btype, final, *fields, tokens, b.pos))
        if final:
            return out


def expand(tokens) -> bytes:
    """What a token list stands for (of one block that starts the output, or of several blocks' lists joined)."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        length, d = t
        if d > len(out):
            raise DeflateError(f"distance {d} at position {len(out)}: before the start of the output")
        if d >= length:
            out += out[len(out) - d:len(out) - d + length]
        else:
            for _ in range(length):
                out.append(out[-d])
    return bytes(out)


def member_stream(member: bytes) -> bytes:
    """The raw DEFLATE stream of one gzip member: what stands between its header (RFC 1952: FEXTRA, FNAME, FCOMMENT, FHCRC) and its
    trailer of eight bytes."""
    if member[:3] != b"\x1f\x8b\x08":
        raise DeflateError("no gzip member")
    flg, p = member[3], 10
    if flg & 4:
        p += 2 + struct.unpack_from("<H", member, p)[0]
    for bit in (8, 16):
        if flg & bit:
            p = member.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    return member[p:len(member) - 8]


def member_block(member: bytes, lenient=False) -> Block:
    """The single DEFLATE block of one gzip / BGZF member."""
    bl = blocks(member_stream(member), lenient)
    if len(bl) != 1:
        raise DeflateError(f"{len(bl)} blocks in one member")
    return bl[0]
