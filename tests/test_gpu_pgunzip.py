"""GPU tests of the parallel decode of plain gzip members (lx_pgunzip.hip behind lx_gunzip): every case asserts zlib's bytes and
what lx_last_gunzip_stats says about the path.  LX_OPT_GUNZIP_CHUNK and _PARALLEL_FROM (and the library's test knob for the chunks per wave) move work between the device and the
host and never change a byte, so a megabyte of input reaches every chunk and wave edge.  The streams (tests/pgunzip_cases.py)
have run through the same algorithm on the CPU under the sanitizers in tests/test_pgunzip_cases.py."""
import gzip
import zlib

import numpy as np
import pytest

from lambda_amd import capi
from tests import pgunzip_cases as pc
from tests.test_gzip_input import bgzf

pytestmark = pytest.mark.gpu

FROM = 4096  # the threshold of the cases below: everything but the small members goes to the device


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


def _decode(h, stream, chunk=65536, wave=0, frm=FROM):
    h.set_option(capi.LX_OPT_GUNZIP_CHUNK, chunk)
    h.set_option(capi.OPT_GUNZIP_WAVE_TEST, wave)
    h.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, frm)
    out = capi.gunzip(h, stream)
    return out, h.last_gunzip_stats()


def _line(st):
    return {f: getattr(st, f) for f, _ in capi.GunzipStats._fields_} | {"why": st.decline_text}


@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("n", [600_000, 2_000_000])
def test_round_trip(handle, n, level):
    stream = pc.gz(n, level)
    assert zlib.decompress(stream, 31) == pc.text(n)
    out, st = _decode(handle, stream)
    assert out == pc.text(n)
    assert (st.plain_parallel, st.plain_host, st.declined, st.chunks_dropped, st.bgzf_members) == (1, 0, 0, 0, 0), _line(st)
    assert st.chunks >= 4 and st.waves >= 1 and st.bytes_down == n, _line(st)
    assert handle.last_phase_ms(10)[1] >= 1 and handle.last_phase_ms(5)[1] == 0
    assert sum(handle.last_phase_ms(p)[1] for p in (101, 102, 103)) == handle.last_phase_ms(10)[1]


def test_options_are_checked(handle):
    for opt, bad in ((capi.LX_OPT_GUNZIP_CHUNK, 32767), (capi.LX_OPT_GUNZIP_CHUNK, (4 << 20) + 1), (capi.OPT_GUNZIP_WAVE_TEST, 1), (capi.OPT_GUNZIP_WAVE_TEST, 513)):
        with pytest.raises(capi.LambdaExtError):
            handle.set_option(opt, bad)
    handle.set_option(capi.LX_OPT_GUNZIP_CHUNK, 32768)
    assert handle.get_option(capi.LX_OPT_GUNZIP_CHUNK) == 32768
    handle.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, capi.LX_GUNZIP_NEVER)
    assert handle.get_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM) == capi.LX_GUNZIP_NEVER
    out, st = _decode(handle, pc.gz(600_000, 6), frm=capi.LX_GUNZIP_NEVER)
    assert out == pc.text(600_000) and (st.plain_parallel, st.plain_host, st.declined, st.waves) == (0, 1, 0, 0), _line(st)


def test_chunk_edges(handle):
    stream, data = pc.gz(600_000, 6), pc.text(600_000)
    n = pc.deflate_len(stream)
    for chunk, chunks in zip(pc.edge_chunks(stream), (3, 3, 3, 1, 1, 1, 1)):
        out, st = _decode(handle, stream, chunk=chunk)
        assert out == data, chunk
        assert (st.plain_parallel, st.declined, st.chunks_dropped, st.chunks) == (1, 0, 0, chunks), (chunk, _line(st))
    # the threshold counts the bytes behind the header: the DEFLATE stream and the trailer
    out, st = _decode(handle, stream, frm=n + 8)
    assert out == data and (st.plain_parallel, st.plain_host) == (1, 0), _line(st)
    out, st = _decode(handle, stream, frm=n + 9)
    assert out == data and (st.plain_parallel, st.plain_host, st.waves) == (0, 1, 0), _line(st)


def test_two_waves(handle):
    out, st = _decode(handle, pc.gz(600_000, 6), chunk=32768, wave=4)
    assert out == pc.text(600_000)
    assert st.waves >= 2 and st.chunks >= 8 and (st.plain_parallel, st.declined, st.chunks_dropped) == (1, 0, 0), _line(st)
    # waves of two chunks: one from a known bit, one found.  A wave sees three chunks of input at most (its last chunk may run on
    # to the end of a block), so it takes at least this many
    stream = pc.gz(2_000_000, 1)
    out, st = _decode(handle, stream, chunk=32768, wave=2)
    assert out == pc.text(2_000_000) and st.waves >= pc.deflate_len(stream) // (3 * 32768) >= 11 and st.plain_parallel == 1, _line(st)


def test_markers(handle):
    stream, data = pc.marker_stream()
    assert zlib.decompress(stream, 31) == data
    out, st = _decode(handle, stream, chunk=32768)
    assert out == data
    assert (st.plain_parallel, st.declined, st.chunks, st.waves) == (1, 0, 3, 1), _line(st)
    out, st = _decode(handle, stream, chunk=32768, wave=2)  # the window in front of the last chunk comes over from the wave before
    assert out == data and (st.plain_parallel, st.chunks, st.waves) == (1, 3, 2), _line(st)


def test_other_block_types(handle):
    stream, data = pc.flushed()
    out, st = _decode(handle, stream)
    assert out == data and (st.plain_parallel, st.declined) == (1, 0) and st.chunks >= 4, _line(st)
    stream, data = pc.fixed_only()
    assert zlib.decompress(stream, 31) == data
    out, st = _decode(handle, stream)
    assert out == data and (st.plain_parallel, st.plain_host, st.declined) == (0, 1, 1), _line(st)
    assert st.last_decline == 1 and st.decline_text == "no boundary", _line(st)
    stream, data = pc.random_stored()
    out, st = _decode(handle, stream)
    assert out == data and st.plain_parallel + st.plain_host == 1 and st.declined == st.plain_host, _line(st)


@pytest.mark.parametrize("case", ["false_positives", "false_positives_behind_text"])
def test_false_positives(handle, case):
    stream, data = getattr(pc, case)()
    assert zlib.decompress(stream, 31) == data
    out, st = _decode(handle, stream)
    assert out == data
    assert st.chunks_dropped > 0 or st.declined == 1, _line(st)
    assert st.plain_parallel + st.plain_host == 1 and st.declined == st.plain_host, _line(st)


def test_room(handle):
    stream, data = pc.zeros()  # (3 KB of DEFLATE)
    out, st = _decode(handle, stream, frm=64)
    assert out == data and st.plain_parallel + st.plain_host == 1 and st.waves == 1, _line(st)
    if st.declined:
        assert st.decline_text == "room", _line(st)
    assert b"lx_gunzip" not in (handle.lib.lx_last_error(handle.h) or b"")  # a decline leaves no status on the handle
    out, st = _decode(handle, pc.gz(600_000, 6))  # and the handle goes on
    assert out == pc.text(600_000) and st.plain_parallel == 1, _line(st)


def test_members_of_every_kind(handle):
    a, b, c, d = pc.text(2_000_000), b">small\nACGT\n", np.random.default_rng(8).bytes(200_000), pc.text(600_000)
    stream = gzip.compress(a, 6) + gzip.compress(b) + bgzf(c) + bgzf(b"") + gzip.compress(d, 1)
    out, st = _decode(handle, stream)
    assert out == a + b + c + d
    assert (st.plain_parallel, st.plain_host, st.declined) == (2, 1, 0), _line(st)
    assert st.bgzf_members == len(c) // 65280 + 1 + 1, _line(st)
    assert handle.last_phase_ms(10)[1] >= 2 and handle.last_phase_ms(5)[1] >= 1


def test_corrupt_input(handle):
    good = pc.gz(1_000_000, 6)
    for name, bad in pc.corrupt(good):
        assert pc.zlib_refuses(bad), name
        with pytest.raises(capi.LambdaExtError) as host:
            capi.gunzip(None, bad)
        handle.set_option(capi.LX_OPT_GUNZIP_CHUNK, 65536)
        handle.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, FROM)
        with pytest.raises(capi.LambdaExtError) as dev:
            capi.gunzip(handle, bad)
        assert dev.value.code == capi.LX_EINVAL and str(dev.value) == str(host.value), (name, str(dev.value), str(host.value))
        st = handle.last_gunzip_stats()
        assert (st.declined, st.plain_parallel) == (1, 0) and st.waves >= 1, (name, _line(st))
        out, st = _decode(handle, good)
        assert out == pc.text(1_000_000) and (st.plain_parallel, st.declined) == (1, 0), (name, _line(st))
