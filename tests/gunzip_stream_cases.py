"""Inputs of the lx_gunzip_stream tests (tests/test_gunzip_stream.py on the host, tests/test_gpu_gunzip_stream.py with a handle) and
the one check both make: the pieces of the stream against zlib's bytes, lx_gunzip's bytes and the bound on a piece's size."""
import gzip
import zlib

import numpy as np

from lambda_amd import capi
from tests import deflate_craft as dc
from tests.test_gzip_input import bgzf, fasta_text, gz_with_fields

PIECES = [4096, 65536, 1 << 30]  # the last one is larger than every file here


def far_copies():
    """One member (fixed Huffman) of 40 000 random bytes and then 300 copies of length 258 from distance 32 768: with pieces of
    4 096 bytes nearly every copy's source lies in an earlier piece, and copies straddle the cuts."""
    s = dc.Stream()
    s.fixed(list(np.random.default_rng(5).bytes(40000)) + [(258, 32768)] * 300, final=True)
    return dc.plain_member(s.getvalue(), bytes(s.data)), bytes(s.data)


def stored_member(n=200_000):
    data = np.random.default_rng(6).bytes(n)
    return gzip.compress(data, 0), data


def bgzf_cases():
    """name -> (file bytes, text): BGZF files, and BGZF runs between other members."""
    text = fasta_text(300_000, 11)
    rnd = np.random.default_rng(12).bytes(150_000)
    small = b"".join(bgzf(text[i:i + 1000]) for i in range(0, 40_000, 1000))  # 40 members of 1 000 bytes
    return {
        "bgzf_text": (bgzf(text), text),
        "bgzf_random_level0": (bgzf(rnd, 0), rnd),
        "bgzf_with_eof_member": (bgzf(text) + bgzf(b""), text),
        "bgzf_small_members": (small, text[:40_000]),
        "bgzf_between_plain": (gzip.compress(text[:70_000]) + bgzf(text[70_000:200_000]) + gzip.compress(text[200_000:]) + bgzf(b"") + bgzf(rnd),
                               text + rnd),
    }


def plain_cases():
    text = fasta_text(300_000, 13)
    far, far_data = far_copies()
    st, st_data = stored_member()
    return {
        "one_member": (gzip.compress(text), text),  # larger than three pieces of 4 096 and of 65 536
        "members": (b"".join(gzip.compress(text[i:i + 50_000], 1 + i % 9) for i in range(0, len(text), 50_000)), text),
        "empty_members": (gzip.compress(b"") + gzip.compress(text[:5000]) + gzip.compress(b"") * 3 + gzip.compress(text[5000:9000]) + gzip.compress(b""),
                          text[:9000]),
        "only_empty_members": (gzip.compress(b"") * 2, b""),
        "stored": (st, st_data),
        "far_copies": (far, far_data),
        "header_fields": (gz_with_fields(text[:100_000], fname=b"x", comment=b"y", hcrc=True, extra=b"AB\x00\x00"), text[:100_000]),
    }


def check_stream(handle, path, raw, text, piece):
    """The stream over `path` (which holds `raw`): zlib's bytes, lx_gunzip's bytes, every piece inside the bound."""
    path.write_bytes(raw)
    pieces = list(capi.gunzip_stream(handle, path, piece))
    assert b"".join(pieces) == text
    if raw[:2] == b"\x1f\x8b":
        d, got, rest = zlib.decompressobj(31), [], raw
        while rest:  # member by member: what zlib itself makes of the file
            got.append(d.decompress(rest))
            rest, d = d.unused_data, zlib.decompressobj(31)
        assert b"".join(got) == text
        assert capi.gunzip(handle, raw) == text
    assert all(1 <= len(p) <= piece + 65536 for p in pieces[:-1]) and (not pieces or 1 <= len(pieces[-1]) <= piece + 65536)
    return pieces
