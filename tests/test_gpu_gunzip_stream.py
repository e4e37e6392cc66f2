"""lx_gunzip_stream_* with a handle: the groups of BGZF members are decoded by the BGZF kernel (lx_gunzip.hip), the pieces are those
of the host stream (tests/test_gunzip_stream.py), and damage gets the text lx_gunzip gives with the same handle."""
import gzip

import pytest

from lambda_amd import capi
from tests import gunzip_stream_cases as gc
from tests.test_gzip_input import bgzf, fasta_text

pytestmark = pytest.mark.gpu

CASES = gc.bgzf_cases()


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


@pytest.mark.parametrize("name", sorted(CASES))
def test_bgzf_groups_on_the_device(handle, tmp_path, name):
    raw, text = CASES[name]
    for piece in gc.PIECES:
        pieces = gc.check_stream(handle, tmp_path / "in.gz", raw, text, piece)
        assert [len(p) for p in pieces] == [len(p) for p in capi.gunzip_stream(None, tmp_path / "in.gz", piece)], piece
        st = handle.last_gunzip_stats()  # (of the whole-file call check_stream ends with: the same members went to the kernel)
        assert st.bgzf_members >= 3 and st.plain_parallel == 0


def test_the_kernel_decodes_the_groups(handle, tmp_path):
    """The stream's own counts: every BGZF member went through the kernel, in one launch per group, and no plain member took the
    parallel path -- also not one that is large enough for it in lx_gunzip."""
    text = fasta_text(1_000_000, 23)
    path = tmp_path / "in.gz"
    path.write_bytes(bgzf(text))
    n_members = (len(text) + 65279) // 65280
    handle.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, 1)
    try:
        pieces = list(capi.gunzip_stream(handle, path, 4 * 65280))
        st = handle.last_gunzip_stats()
        assert b"".join(pieces) == text and [len(p) for p in pieces[:-1]] == [4 * 65280] * (len(pieces) - 1)
        assert st.bgzf_members == n_members and st.plain_host == 0 and st.plain_parallel == 0
        assert handle.last_phase_ms(5)[0] > 0  # the last group's launch
        path.write_bytes(gzip.compress(text, 1))
        assert b"".join(capi.gunzip_stream(handle, path, 65536)) == text
        st = handle.last_gunzip_stats()
        assert st.plain_host == 1 and st.plain_parallel == 0 and st.waves == 0
    finally:
        handle.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, 0)


def test_damage_gets_the_text_of_the_whole_file(handle, tmp_path):
    text = fasta_text(400_000, 29)
    bz = bgzf(text)
    first = len(bgzf(text[:65280]))
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]
    for name, raw in {"crc_first": flip(bz, first - 6), "crc_last": flip(bz, len(bz) - 6), "stream": flip(bz, first + 3000),
                      "truncated": bz[:-100], "garbage": bz + b"\0" * 30}.items():
        with pytest.raises(capi.LambdaExtError) as whole:
            capi.gunzip(handle, raw)
        path = tmp_path / "in.gz"
        path.write_bytes(raw)
        for piece in gc.PIECES:
            with pytest.raises(capi.LambdaExtError) as e:
                list(capi.gunzip_stream(handle, path, piece))
            assert e.value.code == capi.LX_EINVAL and "lx_gunzip: member " in str(e.value), (name, piece)
            assert str(e.value) == str(whole.value), (name, piece)
    # the handle still works
    path.write_bytes(bz)
    assert b"".join(capi.gunzip_stream(handle, path, 65536)) == text
