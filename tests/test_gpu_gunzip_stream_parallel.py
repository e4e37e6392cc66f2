"""lx_gunzip_stream_* with a handle and a plain member large enough for the device: the member is decoded wave by wave by the
kernels of lx_pgunzip.hip (find, decode, chain, resolve as one submission per wave), the pieces are zlib's bytes and lx_gunzip's,
and lx_last_gunzip_stats after a piece says what that call did (after the end: what all of them did).  The files
(tests/gunzip_stream_parallel_cases.py) have run through the same walk on the CPU under the sanitizers in
tests/test_gunzip_stream_parallel.py."""
import zlib

import pytest

from lambda_amd import capi
from tests import gunzip_stream_parallel_cases as sc
from tests import pgunzip_cases as pc

pytestmark = pytest.mark.gpu

COUNTS = ("bgzf_members", "plain_parallel", "plain_host", "chunks", "chunks_dropped", "waves", "declined", "bytes_up", "bytes_down", "waits")


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h
        for opt in (capi.LX_OPT_GUNZIP_CHUNK, capi.OPT_GUNZIP_WAVE_TEST, capi.LX_OPT_GUNZIP_PARALLEL_FROM):
            h.set_option(opt, 0)


def _options(h, chunk=65536, wave=0, frm=sc.FROM):
    h.set_option(capi.LX_OPT_GUNZIP_CHUNK, chunk)
    h.set_option(capi.OPT_GUNZIP_WAVE_TEST, wave)
    h.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, frm)


def _stream(h, path, raw, piece, **options):
    """The pieces of the file; per call of the stream that made one, its counts, its last_decline and the launches of phase 10 and
    of phases 101 to 103; and the counts summed over those calls.  Behind the call that reports the end the handle has the counts
    of the whole file: they must be those sums."""
    _options(h, **options)
    path.write_bytes(raw)
    pieces, calls = [], []

    def note():
        st = h.last_gunzip_stats()
        calls.append({f: getattr(st, f) for f in COUNTS} | {"last_decline": st.last_decline, "why": st.decline_text, "p10": h.last_phase_ms(10)[1],
                                                            "p10x": sum(h.last_phase_ms(p)[1] for p in (101, 102, 103))})

    for p in capi.gunzip_stream(h, path, piece):
        pieces.append(p)
        note()
    total = {f: sum(c[f] for c in calls) for f in COUNTS}
    end = h.last_gunzip_stats()
    assert {f: getattr(end, f) for f in COUNTS} == total, (total, {f: getattr(end, f) for f in COUNTS})
    assert end.last_decline == max([c["last_decline"] for c in calls if c["declined"]] + [0])
    return pieces, calls, total


def _contract(pieces, piece):
    assert all(1 <= len(p) <= piece + 65536 for p in pieces)


@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("n", [600_000, 2_000_000])
def test_round_trip(handle, tmp_path, n, level):
    raw, text = pc.gz(n, level), pc.text(n)
    assert zlib.decompress(raw, 31) == text
    for piece in (65536, 1 << 20):
        pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, piece)
        assert b"".join(pieces) == text, piece
        _contract(pieces, piece)
        assert (t["plain_parallel"], t["plain_host"], t["declined"], t["chunks_dropped"], t["bgzf_members"]) == (1, 0, 0, 0, 0), (piece, t)
        assert t["chunks"] >= 4 and t["bytes_down"] == n and t["waits"] == t["waves"] >= 1, (piece, t)
        assert max(c["p10"] for c in calls) >= 1 and all(c["p10"] == c["p10x"] == 3 * c["waves"] for c in calls), calls
    assert capi.gunzip(handle, raw) == text


def test_chunk_and_wave_edges(handle, tmp_path):
    raw, text = pc.gz(600_000, 6), pc.text(600_000)
    for i, chunk in enumerate(pc.edge_chunks(raw)):
        for wave in (2, 4):
            pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, 65536, chunk=chunk, wave=wave)
            assert b"".join(pieces) == text, (chunk, wave)
            _contract(pieces, 65536)
            assert (t["plain_parallel"], t["declined"], t["chunks_dropped"]) == (1, 0, 0), (chunk, wave, t)
            # (a piece of 64 KiB holds a wave to two chunks: the thirds take two waves, the chunks as long as the stream one)
            assert t["waves"] >= 2 if i < 3 else t["waves"] == 1, (chunk, wave, t)
    for wave in (2, 4):  # chunks of 32 KiB, pieces of four chunks' input: the knob is what cuts the waves
        pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, 131072, chunk=32768, wave=wave)
        assert b"".join(pieces) == text and t["waves"] >= 2 and t["waits"] == t["waves"] and t["plain_parallel"] == 1, (wave, t)
    m, data = pc.marker_stream()  # the window in front of the second wave is text the stream handed out many pieces ago
    pieces, calls, t = _stream(handle, tmp_path / "in.gz", m, 4096, chunk=32768, wave=2)
    assert b"".join(pieces) == data and (t["plain_parallel"], t["chunks"], t["waves"]) == (1, 3, 2), t
    assert all(len(p) == 4096 for p in pieces[:-1])


@pytest.mark.parametrize("case", ["late_fixed", "late_stored"])
def test_a_decline_in_a_later_wave(handle, tmp_path, case):
    raw, text = getattr(sc, case)()
    # (pieces and waves of several sizes: where the host's bytes land in the stream's buffer behind what the waves left differs)
    for wave, piece in ((8, 262144), (6, 300_000), (8, 524288), (16, 600_000)):
        pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, piece, chunk=32768, wave=wave)
        assert b"".join(pieces) == text, (wave, piece)
        _contract(pieces, piece)
        assert (t["plain_parallel"], t["plain_host"], t["declined"]) == (0, 1, 1) and t["waves"] >= 2, (wave, piece, t)
        k = next(i for i, c in enumerate(calls) if c["declined"])
        assert calls[k]["last_decline"] == 1 and calls[k]["why"] == "no boundary", calls[k]
        assert sum(c["chunks"] for c in calls[:k + 1]) == t["chunks"] > 0 and sum(c["bytes_down"] for c in calls[:k + 1]) >= len(b"".join(pieces[:k]))
    assert capi.gunzip(handle, raw) == text


def test_mixed_file(handle, tmp_path):
    raw, text, n_bgzf = sc.mixed()
    for piece in (65536, 1 << 20):
        pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, piece)
        assert b"".join(pieces) == text, piece
        _contract(pieces, piece)
        assert (t["bgzf_members"], t["plain_parallel"], t["plain_host"], t["declined"]) == (n_bgzf, 1, 0, 0), (piece, t)
    raw, text = sc.members()
    pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, 65536)
    assert b"".join(pieces) == text and (t["plain_parallel"], t["plain_host"], t["declined"]) == (2, 1, 0), t
    assert capi.gunzip(handle, raw) == text


def test_threshold(handle, tmp_path):
    raw, text = pc.gz(600_000, 6), pc.text(600_000)
    pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, 65536, frm=capi.LX_GUNZIP_NEVER)
    assert b"".join(pieces) == text and (t["plain_parallel"], t["plain_host"], t["waves"], t["waits"]) == (0, 1, 0, 0), t
    assert [len(p) for p in pieces] == [len(p) for p in capi.gunzip_stream(None, tmp_path / "in.gz", 65536)]  # the host path's own pieces
    n = pc.deflate_len(raw)  # the threshold counts the bytes behind the header: the DEFLATE stream and the trailer
    pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, 65536, frm=n + 8)
    assert b"".join(pieces) == text and (t["plain_parallel"], t["plain_host"]) == (1, 0), t
    pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, 65536, frm=n + 9)
    assert b"".join(pieces) == text and (t["plain_parallel"], t["plain_host"], t["waves"]) == (0, 1, 0), t
    # below 10 bytes there is nothing the host could try first, and a stream, which cannot take pieces back, stays on the host
    pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, 65536, frm=9)
    assert b"".join(pieces) == text and (t["plain_parallel"], t["plain_host"], t["waves"]) == (0, 1, 0), t
    pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, 65536, frm=10)
    assert b"".join(pieces) == text and (t["plain_parallel"], t["plain_host"]) == (1, 0), t


def test_damage(handle, tmp_path):
    """Ordinary error returns: the text is lx_gunzip's for the whole file, and the call is the one in which the host path fails."""
    for name, (raw, k, at) in sorted(sc.damaged().items()):
        assert sc.zlib_refuses(raw), name
        with pytest.raises(capi.LambdaExtError) as whole:
            capi.gunzip(None, raw)
        path = tmp_path / "in.gz"
        path.write_bytes(raw)
        host = []
        with pytest.raises(capi.LambdaExtError):
            for p in capi.gunzip_stream(None, path, 65536):
                host.append(p)
        _options(handle, chunk=32768, wave=4)
        dev = []
        with pytest.raises(capi.LambdaExtError) as e:
            for p in capi.gunzip_stream(handle, path, 65536):
                dev.append(p)
        assert e.value.code == capi.LX_EINVAL and str(e.value) == str(whole.value), (name, str(e.value), str(whole.value))
        assert f"lx_gunzip: member {k} at byte {at}: " in str(e.value), (name, str(e.value))
        assert len(dev) == len(host) >= 1, (name, len(dev), len(host))
    raw, text = pc.gz(600_000, 6), pc.text(600_000)  # the handle goes on
    pieces, calls, t = _stream(handle, tmp_path / "in.gz", raw, 65536)
    assert b"".join(pieces) == text and t["plain_parallel"] == 1


def test_one_shot_through_the_one_submission_wave(handle):
    """What tests/test_gpu_pgunzip.py::test_round_trip expects of lx_gunzip, and one synchronisation per wave."""
    for n, level in ((600_000, 6), (2_000_000, 1)):
        _options(handle)
        out = capi.gunzip(handle, pc.gz(n, level))
        st = handle.last_gunzip_stats()
        assert out == pc.text(n)
        assert (st.plain_parallel, st.plain_host, st.declined, st.chunks_dropped, st.bgzf_members) == (1, 0, 0, 0, 0)
        assert st.chunks >= 4 and st.waves >= 1 and st.bytes_down == n and st.waits == st.waves
        assert sum(handle.last_phase_ms(p)[1] for p in (101, 102, 103)) == handle.last_phase_ms(10)[1] == 3 * st.waves
    _options(handle, chunk=32768, wave=2)
    out = capi.gunzip(handle, pc.gz(2_000_000, 1))
    st = handle.last_gunzip_stats()
    assert out == pc.text(2_000_000) and st.waves >= 11 and st.waits == st.waves and st.plain_parallel == 1
