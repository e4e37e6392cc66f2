"""Files for the tests of a plain gzip member decoded wave by wave inside lx_gunzip_stream: tests/test_gunzip_stream_parallel.py
(the stream's walk on the CPU under the sanitizers) and tests/test_gpu_gunzip_stream_parallel.py (the library with a handle).
Everything is made by zlib / gzip from the texts of tests/pgunzip_cases.py, and zlib says what each file decodes to."""
import functools
import gzip
import struct
import zlib

import numpy as np

from tests import pgunzip_cases as pc
from tests.test_gzip_input import bgzf, fasta_text

FROM = 4096  # LX_OPT_GUNZIP_PARALLEL_FROM of these tests: every member but the small ones is one for the device


def _late(tail_raw, a, b):
    """Dynamic-Huffman blocks of `a` (level 6, closed by a full flush: byte-aligned, not final) and then `tail_raw`, the raw
    DEFLATE stream of `b`, as one member."""
    c6 = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c6.compress(a) + c6.flush(zlib.Z_FULL_FLUSH) + tail_raw
    return pc.member_of(raw, a + b), a + b


@functools.lru_cache(maxsize=None)
def late_fixed():
    """~290 KB of dynamic blocks, then ~330 KB of fixed-Huffman blocks: with chunks of 32 KiB in waves of 8 the first wave is all
    dynamic blocks, and a later wave begins where no block start can be found in more than four chunks on end: 'no boundary'."""
    a, b = pc.text(1_000_000), fasta_text(600_000, 41)
    cf = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    return _late(cf.compress(b) + cf.flush(), a, b)


@functools.lru_cache(maxsize=None)
def late_stored():
    """The same with 400 000 random bytes in stored blocks behind the dynamic ones."""
    a, b = pc.text(1_000_000), np.random.default_rng(43).bytes(400_000)
    c0 = zlib.compressobj(0, zlib.DEFLATED, -15)
    return _late(c0.compress(b) + c0.flush(), a, b)


@functools.lru_cache(maxsize=None)
def members():
    """A plain member for the device, a second one, a run of BGZF members, a small plain member."""
    a, b, c, d = pc.text(600_000), fasta_text(400_000, 47), fasta_text(150_000, 53), b">small\nACGT\n"
    return pc.gz(600_000, 6) + gzip.compress(b, 1) + bgzf(c) + bgzf(b"") + gzip.compress(d), a + b + c + d


@functools.lru_cache(maxsize=None)
def mixed():
    """BGZF members, a plain member, BGZF members."""
    a, b, c = fasta_text(200_000, 59), pc.text(2_000_000), fasta_text(100_000, 61)
    return bgzf(a) + pc.gz(2_000_000, 6) + bgzf(c), a + b + c, (len(a) + 65279) // 65280 + (len(c) + 65279) // 65280


@functools.lru_cache(maxsize=None)
def damaged():
    """name -> (file, member number and byte offset lx_gunzip's message must name): a member damaged the four ways of
    pgunzip_cases.corrupt, the trailer cut, and the flipped bit inside a second member."""
    good, lead = pc.gz(1_000_000, 6), pc.gz(600_000, 1)
    out = {name: (bad, 0, 0) for name, bad in pc.corrupt(good)}
    out["trailer_cut"] = (good[:-3], 0, 0)
    out["flip_in_second_member"] = (lead + dict(pc.corrupt(good))["flip"], 1, len(lead))
    return out


def zlib_refuses(raw):
    """zlib, member by member, does not get to the end of the file."""
    rest = raw
    while rest:
        if pc.zlib_refuses(rest):
            return True
        d = zlib.decompressobj(31)
        d.decompress(rest)
        rest = d.unused_data
    return False


def pack_corpus(records):
    """The stand-alone program's corpus: (chunk, wave knob, piece, device, parallel_from, file)."""
    return b"LXGS" + struct.pack("<I", len(records)) + b"".join(struct.pack("<IIIIQI", c, w, p, dev, frm, len(d)) + d for c, w, p, dev, frm, d in records)
