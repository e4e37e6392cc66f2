"""lx_gunzip_stream_* without a GPU (h = NULL): the pieces of a file, concatenated, are zlib's bytes and lx_gunzip's, no piece is
longer than piece_bytes + 65536, and damage is refused with the text lx_gunzip gives for the whole file."""
import ctypes as C
import gzip

import pytest

from lambda_amd import capi
from tests import gunzip_stream_cases as gc
from tests.test_gzip_input import bgzf, fasta_text

CASES = {**gc.plain_cases(), **gc.bgzf_cases()}


@pytest.mark.parametrize("piece", gc.PIECES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_pieces_are_the_whole(tmp_path, name, piece):
    raw, text = CASES[name]
    pieces = gc.check_stream(None, tmp_path / "in.gz", raw, text, piece)
    if piece > len(text):
        assert len(pieces) == (1 if text else 0)


def test_one_member_larger_than_three_pieces_is_cut(tmp_path):
    raw, text = CASES["one_member"]
    pieces = gc.check_stream(None, tmp_path / "in.gz", raw, text, 65536)
    assert len(pieces) >= 3 and all(65536 <= len(p) <= 65536 + 257 for p in pieces[:-1])  # (a copy ends at most 257 bytes behind the cut)
    raw, text = CASES["far_copies"]
    pieces = gc.check_stream(None, tmp_path / "in.gz", raw, text, 4096)
    assert len(pieces) >= 25 and all(4096 <= len(p) <= 4096 + 257 for p in pieces[:-1])
    raw, text = CASES["stored"]  # (a stored block is handed on whole: up to 65 535 bytes behind the cut)
    pieces = gc.check_stream(None, tmp_path / "in.gz", raw, text, 4096)
    assert len(pieces) >= 3 and all(4096 <= len(p) < 4096 + 65536 for p in pieces[:-1])


def test_bgzf_groups_are_whole_members(tmp_path):
    raw, text = CASES["bgzf_small_members"]
    pieces = gc.check_stream(None, tmp_path / "in.gz", raw, text, 4096)
    assert [len(p) for p in pieces] == [5000] * 8  # members of 1 000 bytes until 4 096 are reached
    raw, text = CASES["bgzf_text"]
    pieces = gc.check_stream(None, tmp_path / "in.gz", raw, text, 65536)
    assert [len(p) for p in pieces[:-1]] == [2 * 65280] * (len(pieces) - 1)


@pytest.mark.parametrize("piece", gc.PIECES)
def test_plain_file_and_empty_file(tmp_path, piece):
    text = fasta_text(150_001, 3)
    pieces = gc.check_stream(None, tmp_path / "in.fasta", text, text, piece)
    assert [len(p) for p in pieces[:-1]] == [piece] * (len(pieces) - 1)
    assert gc.check_stream(None, tmp_path / "empty", b"", b"", piece) == []
    assert gc.check_stream(None, tmp_path / "one", b"\x1f", b"\x1f", piece) == [b"\x1f"]


def _damaged():
    text = fasta_text(200_000, 17)
    plain, members, bz = gzip.compress(text), gzip.compress(text[:90_000]) + gzip.compress(text[90_000:]), bgzf(text)
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]
    return {
        "plain_truncated_stream": plain[:len(plain) // 2],
        "plain_truncated_trailer": plain[:-3],
        "plain_bad_crc": flip(plain, len(plain) - 6),
        "plain_bad_isize": flip(plain, len(plain) - 2),
        "plain_damaged_stream": flip(plain, len(plain) // 2),
        "plain_trailing_garbage": plain + b"garbage behind the member",
        "second_member_bad_crc": flip(members, len(members) - 6),
        "second_member_truncated": members[:-40_00],
        "bgzf_truncated": bz[:-100],
        "bgzf_bad_crc": flip(bz, len(bz) - 6),
        "bgzf_bad_crc_first_member": flip(bz, len(bgzf(text[:65280])) - 6),
        "bgzf_damaged_stream": flip(bz, len(bz) - 3000),
        "bgzf_trailing_garbage": bz + b"\x00" * 30,
        "bgzf_trailing_short": bz + b"\x1f\x8b\x08",
    }


DAMAGED = _damaged()


@pytest.mark.parametrize("piece", gc.PIECES)
@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_damage_gets_the_text_of_the_whole_file(tmp_path, name, piece):
    raw = DAMAGED[name]
    with pytest.raises(capi.LambdaExtError) as whole:
        capi.gunzip(None, raw)
    path = tmp_path / "in.gz"
    path.write_bytes(raw)
    got = []
    with pytest.raises(capi.LambdaExtError) as e:
        for p in capi.gunzip_stream(None, path, piece):
            got.append(p)
    assert e.value.code == whole.value.code == capi.LX_EINVAL
    assert str(e.value) == str(whole.value) and "lx_gunzip: member " in str(e.value) and " at byte " in str(e.value)
    # what came before is in pieces inside the bound; and it is the text's beginning, unless the flipped bit still decodes (a
    # member's CRC32 is known only at its trailer: pieces of a member that fails later may hold what the damaged bits say)
    assert all(1 <= len(p) <= piece + 65536 for p in got)
    if not name.endswith("damaged_stream"):
        assert fasta_text(200_000, 17).startswith(b"".join(got))


def test_refusals(tmp_path, lx_lib):
    s, piece = C.c_void_p(), C.c_void_p()
    assert lx_lib.lx_gunzip_stream_open(None, None, 0, C.byref(s)) == capi.LX_EINVAL and "NULL" in capi.last_output_error()
    assert lx_lib.lx_gunzip_stream_open(None, b"x", 0, None) == capi.LX_EINVAL and "NULL" in capi.last_output_error()
    missing = tmp_path / "no" / "such.gz"
    assert lx_lib.lx_gunzip_stream_open(None, bytes(missing), 0, C.byref(s)) == capi.LX_EINVAL and not s
    assert "cannot open" in capi.last_output_error() and str(missing) in capi.last_output_error()
    assert lx_lib.lx_gunzip_stream_next(None, C.byref(piece)) == capi.LX_EINVAL and "NULL" in capi.last_output_error()
    with pytest.raises(capi.LambdaExtError, match="cannot open"):
        list(capi.gunzip_stream(None, missing))
    # a stream that has failed stays failed, and the end is reported again and again
    bad = tmp_path / "bad.gz"
    bad.write_bytes(gzip.compress(b"ACGT" * 100)[:-3])
    assert lx_lib.lx_gunzip_stream_open(None, bytes(bad), 0, C.byref(s)) == capi.LX_OK
    assert lx_lib.lx_gunzip_stream_next(s, None) == capi.LX_EINVAL
    assert lx_lib.lx_gunzip_stream_next(s, C.byref(piece)) == capi.LX_EINVAL and "truncated gzip trailer" in capi.last_output_error()
    assert lx_lib.lx_gunzip_stream_next(s, C.byref(piece)) == capi.LX_EINVAL and "has failed" in capi.last_output_error() and not piece
    lx_lib.lx_gunzip_stream_close(s)
    lx_lib.lx_gunzip_stream_close(None)
    good = tmp_path / "good.gz"
    good.write_bytes(gzip.compress(b"ACGT" * 100))
    assert lx_lib.lx_gunzip_stream_open(None, bytes(good), 0, C.byref(s)) == capi.LX_OK  # (0 = the default piece)
    assert lx_lib.lx_gunzip_stream_next(s, C.byref(piece)) == capi.LX_OK and lx_lib.lx_bytes_size(piece) == 400
    lx_lib.lx_bytes_free(piece)
    for _ in range(2):
        assert lx_lib.lx_gunzip_stream_next(s, C.byref(piece)) == capi.LX_OK and not piece
    lx_lib.lx_gunzip_stream_close(s)
