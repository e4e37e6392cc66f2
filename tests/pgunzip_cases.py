"""Streams for the parallel decode of plain gzip members, shared by tests/test_pgunzip_cases.py (the algorithm on the CPU under the
sanitizers) and tests/test_gpu_pgunzip.py (lx_gunzip with a handle).  Everything here is made by zlib / gzip or written bit by bit
with tests/deflate_craft.py, and zlib says what each stream decodes to."""
import functools
import gzip
import struct
import zlib

import numpy as np

from tests import deflate_craft as dc
from tests.test_gzip_input import fasta_text

HEADER = 10  # gzip.compress / plain_member: no optional header field


@functools.lru_cache(maxsize=None)
def text(n):
    return fasta_text(n)


@functools.lru_cache(maxsize=None)
def gz(n, level):
    return gzip.compress(text(n), level)


def member_of(raw, data):
    """A raw DEFLATE stream as one plain gzip member; zlib is asked what it decodes to."""
    assert zlib.decompress(raw, -15) == data
    return dc.plain_member(raw, data)


@functools.lru_cache(maxsize=None)
def marker_stream():
    """Four dynamic blocks written by hand for chunks of 32 KiB.  A: 35 000 literals (8 / 9-bit codes, ~35.4 KB), so block B is
    the first block start in the second chunk.  B opens with a copy of length 258 at distance 32 768, a copy at distance 1 whose
    source is that copy's last symbol (a marker copied from a marker), one at distance 32 767, one from the markers made so far;
    then 31 000 literals and three length-258 copies in front of its end-of-block.  B is fewer than 32 768 symbols and ends beyond
    byte 65 536, so block C is found in the third chunk, and the window in front of C is part B, part the window in front of B.
    C opens with length-258 copies at distances 32 768 and 32 767 and one that overlaps itself; D is the final block."""
    rng = np.random.default_rng(5)
    lit = [8] * 226 + [9] * 60  # complete: 226 / 256 + 60 / 512 = 1
    dist = [4, 4] + [5] * 28    # complete: 2 / 16 + 28 / 32 = 1
    s = dc.Stream()
    s.dynamic([int(b) for b in rng.integers(0, 256, 35_000)], lit, dist)
    a_end = s.w.nbits()
    b_tokens = [(258, 32768), (20, 1), (100, 32767), (258, 300)] + [int(b) for b in rng.integers(0, 256, 31_000)] + \
               [(258, 32768), (258, 20000), (258, 258)]
    s.dynamic(b_tokens, lit, dist)
    b_end = s.w.nbits()
    b_symbols = 258 + 20 + 100 + 258 + 31_000 + 3 * 258
    s.dynamic([(258, 32768), (258, 32767), (258, 1), (258, 257)] + [int(b) for b in rng.integers(0, 256, 3_000)], lit, dist)
    s.dynamic([(258, 32768), 65, 66, 67], lit, dist, final=True)
    assert 32768 * 8 < a_end < 65536 * 8 < b_end < 98304 * 8 and b_symbols < 32768
    return member_of(s.getvalue(), bytes(s.data)), bytes(s.data)


@functools.lru_cache(maxsize=None)
def flushed():
    """One compressobj, Z_FULL_FLUSH every 100 KB: an empty stored block between the dynamic ones (pigz's shape)."""
    data = text(600_000)
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    out = b"".join(c.compress(data[i:i + 100_000]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(data), 100_000)) + c.flush()
    return out, data


@functools.lru_cache(maxsize=None)
def fixed_only():
    data = text(600_000)
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 9, zlib.Z_FIXED)
    return c.compress(data) + c.flush(), data


@functools.lru_cache(maxsize=None)
def random_stored():
    data = np.random.default_rng(3).bytes(300_000)
    return gzip.compress(data, 6), data


@functools.lru_cache(maxsize=None)
def false_positives():
    """Stored blocks whose payload is a gzip file: genuine dynamic block headers that are no block starts of this stream."""
    data = gz(600_000, 6)
    return gzip.compress(data, 0), data


@functools.lru_cache(maxsize=None)
def false_positives_behind_text():
    """The same payload behind ~210 KB of ordinary dynamic blocks: one DEFLATE stream put together from a level-6 piece that ends
    in a full flush (byte-aligned, not final) and a level-0 piece (stored blocks, the last one final)."""
    a, b = text(400_000), gz(600_000, 6)
    c6, c0 = zlib.compressobj(6, zlib.DEFLATED, -15), zlib.compressobj(0, zlib.DEFLATED, -15)
    raw = c6.compress(a) + c6.flush(zlib.Z_FULL_FLUSH) + c0.compress(b) + c0.flush()
    return member_of(raw, a + b), a + b


@functools.lru_cache(maxsize=None)
def zeros():
    data = bytes(3_000_000)
    return gzip.compress(data, 6), data


def deflate_len(stream):
    """Bytes of the DEFLATE stream of a one-member file without optional header fields."""
    return len(stream) - HEADER - 8


def corrupt(stream):
    """(name, stream) of a valid member damaged four ways; zlib must refuse each."""
    mid = bytearray(stream)
    mid[HEADER + deflate_len(stream) // 2] ^= 0x10
    crc = bytearray(stream)
    crc[-8] ^= 1
    isz = bytearray(stream)
    isz[-1] ^= 1
    return [("flip", bytes(mid)), ("cut", stream[:len(stream) // 2]), ("crc", bytes(crc)), ("isize", bytes(isz))]


def zlib_refuses(stream):
    try:
        d = zlib.decompressobj(31)
        d.decompress(stream)
        return not d.eof
    except zlib.error:
        return True


def edge_chunks(stream):
    """Chunk sizes that put the chunk starts on every edge of a ~320 KB stream: thirds, a start inside the final block, on the
    stream's last byte, in the trailer behind it (nothing there to find: the chunk merges), and one chunk for all of it."""
    n = deflate_len(stream)
    return [n // 3 - 1, n // 3, n // 3 + 1, n - 5000, n - 1, n + 4, n + 8]


def pack_corpus(records):
    """The stand-alone program's corpus: (chunk, wave, bytes behind the gzip header)."""
    return b"LXPG" + struct.pack("<I", len(records)) + b"".join(struct.pack("<III", c, w, len(d)) + d for c, w, d in records)
