"""GPU tests of the BGZF decoder (lx_gunzip.hip) on streams built on purpose: the DEFLATE constructs and every refusal of
tests/deflate_craft.py, the zlib mutants of the differential run, and BGZF members of the sizes real files have -- any size, so
every residue of the output offset, both copy-out paths with head and tail, the CRC slices around 256 bytes, ISIZE 65 536, empty
members, members with other header fields, runs split by a member the host decodes, and runs of several chunks.

Every expectation is zlib's (or `gzip.decompress` of the very stream); every assertion is byte equality or an error text."""
import gzip
import zlib

import numpy as np
import pytest

from lambda_amd import capi
from tests import deflate_craft as dc

pytestmark = pytest.mark.gpu

GOOD_DATA = b">good\nACGT\n"
GOOD = dc.bgzf_member(zlib.compress(GOOD_DATA, 6)[2:-4], GOOD_DATA)
INVALID_NAMES = [c.name for c in dc.invalid_cases()]


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


def _launches(handle):
    return handle.last_phase_ms(5)[1]


def _decodes(handle, stream, want, launches):
    assert gzip.decompress(stream) == want  # the stream itself, before the decoder under test sees it
    got = capi.gunzip(handle, stream)
    assert len(got) == len(want)
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"first difference at byte {at} of {len(want)}: {got[at:at + 16]!r} for {want[at:at + 16]!r}")
    assert _launches(handle) == launches


# ---- constructs

@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_device_decodes_every_construct(handle, order):
    """All VALID cases as the members of one stream in one call (one launch); in reverse, each lands on another output offset."""
    V = dc.valid_cases() if order == "forward" else dc.valid_cases()[::-1]
    for v in V:  # each alone first, so that a failure names its case
        try:
            got = capi.gunzip(handle, dc.bgzf_member(v.raw, v.data))
        except capi.LambdaExtError as e:
            raise AssertionError(f"{v.name}: {e}") from e
        assert got == v.data, v.name
    _decodes(handle, b"".join(dc.bgzf_member(v.raw, v.data) for v in V), b"".join(v.data for v in V), 1)


# ---- statuses

@pytest.mark.parametrize("name", INVALID_NAMES)
def test_device_refuses_invalid_case_by_its_text(handle, name):
    c = next(c for c in dc.invalid_cases() if c.name == name)
    with pytest.raises(capi.LambdaExtError) as e:
        capi.gunzip(handle, GOOD + c.member() + GOOD)
    msg = str(e.value)
    assert e.value.code == capi.LX_EINVAL and "lx_gunzip: member 1 " in msg and any(msg.endswith(": " + t) for t in c.texts), (name, msg)
    assert capi.gunzip(handle, GOOD + GOOD) == GOOD_DATA * 2  # the handle goes on working


def test_device_decodes_the_mutants_zlib_accepts(handle):
    M = [m for m in dc.mutants() if m.accepted]
    assert len(M) > 5000
    stream = b"".join(dc.bgzf_member(m.raw[:m.consumed], m.data) for m in M)
    _decodes(handle, stream, b"".join(m.data for m in M), (len(M) + 511) // 512)


def test_device_refuses_the_mutants_zlib_refuses(handle):
    M = [m for m in dc.mutants() if not m.accepted][:300]
    assert len(M) == 300
    for i, m in enumerate(M):
        with pytest.raises(capi.LambdaExtError) as e:
            capi.gunzip(handle, GOOD + dc.bgzf_member(m.raw, b"", isize=m.true_len, crc=i) + GOOD)
        assert e.value.code == capi.LX_EINVAL and "lx_gunzip: member 1 " in str(e.value), (i, str(e.value))
    assert capi.gunzip(handle, GOOD + GOOD) == GOOD_DATA * 2


# ---- member sizes

def _text(n, rng):
    """n bytes of FASTA-like text (compressible: a member of 65 536 of them stays within BSIZE)."""
    rows = []
    while sum(map(len, rows)) < n:
        rows.append(b">r%d\n" % len(rows) + bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), 60).tolist()) + b"\n")
    return b"".join(rows)[:n]


def _member(data, **kw):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return dc.bgzf_member(c.compress(data) + c.flush(), data, **kw)


SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 65535, 65536, 7, 6, 5, 9]


def _parts(seed):
    rng = np.random.default_rng(seed)
    return [_text(n, rng) for n in SIZES]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_members_of_any_size(handle, shift):
    """The members' output offsets are the prefix sums of SIZES (0, 0, 1, 3, 6, 10, 15, 270, 526, 783, 1806, 67341, 132877, ..):
    those of 4 bytes and more start on all four residues, so both copy-out paths run with body and tail; 255 / 256 / 257 bytes
    are CRC slices of 1, 1 and 2 bytes per lane.  A member of `shift` bytes in front moves every member to the next residue."""
    off = shift + np.concatenate([[0], np.cumsum(SIZES)[:-1]])
    assert {int(o) & 3 for o, n in zip(off, SIZES) if n >= 4} == {0, 1, 2, 3}
    parts = ([b"#" * shift] if shift else []) + _parts(5)
    _decodes(handle, b"".join(_member(p) for p in parts), b"".join(parts), 1)


def test_device_run_split_by_a_member_for_the_host(handle):
    parts = _parts(6)
    big = _text(65537, np.random.default_rng(7))  # ISIZE beyond the kernel's LDS: decoded on the host, between two device runs
    members = [_member(p) for p in parts]
    stream = b"".join(members[:8]) + _member(big) + b"".join(members[8:])
    _decodes(handle, stream, b"".join(parts[:8]) + big + b"".join(parts[8:]), 2)


def test_device_members_with_other_header_fields(handle):
    parts = _parts(8)[:11]
    kws = [dict(fname=b"reads.fastq"), dict(extra_before=b"XY\x03\x00abc"), dict(extra_after=b"ZZ\x00\x00"),
           dict(extra_before=b"AB\x01\x00q", extra_after=b"CB\x02\x00\x01\x02", fname=b"n")]
    members = [_member(p, **kws[i % 4]) for i, p in enumerate(parts)]
    _decodes(handle, b"".join(members), b"".join(parts), 1)


def test_device_1030_small_members_in_three_chunks(handle):
    rng = np.random.default_rng(9)
    parts = [_text(int(n), rng) for n in rng.integers(0, 41, 1030)]
    _decodes(handle, b"".join(_member(p) for p in parts), b"".join(parts), 3)


def test_device_512_empty_members_then_one(handle):
    last = _text(1000, np.random.default_rng(10))
    _decodes(handle, _member(b"") * 512 + _member(last), last, 2)  # (the first chunk has no output at all)
