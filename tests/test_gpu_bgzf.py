"""GPU tests of the BGZF encoder (lx_bgzf.hip): round trips through zlib, the member framing, determinism, the ratio against zlib
level 1, lx_write_records_bgzf, and the lambda3 front end's .bam / .gz outputs."""
import gzip
import struct
import subprocess
import zlib

import numpy as np
import pytest

from lambda_amd import build, capi
from tests import bam_decode
from tests.test_bam_encoding import ALL_TAGS, PROGRAMS, _case, _options, _render

pytestmark = pytest.mark.gpu
BLOCK = 65280
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


def _members(out: bytes, data: bytes, eof: bool):
    """Walks the members: BC / SLEN 2, BSIZE + 1 = member length, ISIZE <= 65 280, CRC = zlib.crc32 of the block."""
    p, k, sizes = 0, 0, []
    body = out[:-28] if eof else out
    if eof:
        assert out[-28:] == EOF_MEMBER
    while p < len(body):
        assert body[p:p + 4] == b"\x1f\x8b\x08\x04" and body[p + 10:p + 12] == b"\x06\x00"
        assert body[p + 12:p + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", body, p + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", body, p + size - 8)
        block = data[k * BLOCK:(k + 1) * BLOCK]
        assert isize == len(block) <= BLOCK and crc == zlib.crc32(block)
        sizes.append(size)
        p += size
        k += 1
    assert p == len(body) and k == (len(data) + BLOCK - 1) // BLOCK
    return sizes


def _sam_text(n):
    m, ops, names, qa, qoff = _case("blastn", seed=5, nq=400, ns=30)
    opt, _ = _options("blastn", ALL_TAGS, capi.LX_SAM_SEQ_ALWAYS, 1, False, m, 30)
    t = _render(capi.LX_OUT_SAM, "blastn", m, ops, names, qa, qoff, opt)
    return (t * (n // len(t) + 1))[:n]


def _m8_text(n):
    m, ops, names, qa, qoff = _case("blastx", seed=6, nq=400, ns=30)
    t = _render(capi.LX_OUT_BLAST_TAB, "blastx", m, ops, names, qa, qoff, None)
    return (t * (n // len(t) + 1))[:n]


def _contents(kind, n):
    rng = np.random.default_rng(n)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "zeros":
        return bytes(n)
    if kind == "period":
        unit = rng.integers(0, 256, 32768 - 5, dtype=np.uint8).tobytes()
        return (unit * (n // len(unit) + 1))[:n]
    if kind == "sam":
        return _sam_text(n)
    m, ops, names, qa, qoff = _case("blastn", seed=8, nq=300, ns=20)
    t = _render(capi.LX_OUT_BAM, "blastn", m, ops, names, qa, qoff, None)
    return (t * (n // len(t) + 1))[:n]


@pytest.mark.parametrize("n", [0, 1, 65279, 65280, 65281, 3 * 65280 + 7])
@pytest.mark.parametrize("kind", ["random", "zeros", "period", "sam", "bam"])
def test_round_trip_and_framing(handle, kind, n):
    data = _contents(kind, n)
    for eof in (False, True):
        out = handle.bgzf_compress(data, eof=eof)
        assert gzip.decompress(out) == data
        sizes = _members(out, data, eof)
        if kind == "random":  # stored blocks: header, stored-block header and trailer only
            assert all(s == min(BLOCK, n - i * BLOCK) + 31 for i, s in enumerate(sizes))
        if kind == "zeros" and n >= 65280:
            assert sizes[0] < 1024


def test_round_trip_50_mb_through_several_chunks(handle):
    rng = np.random.default_rng(9)
    parts = [_sam_text(20_000_000), rng.integers(0, 256, 10_000_000, dtype=np.uint8).tobytes(), _m8_text(20_000_000), bytes(123_457)]
    data = b"".join(parts)
    out = handle.bgzf_compress(data, eof=True)
    assert gzip.decompress(out) == data
    _members(out, data, True)
    ms, launches = handle.last_phase_ms(4)
    assert launches >= 2 and ms > 0


def test_deterministic_across_calls_and_handles(handle):
    data = _sam_text(5_000_000) + _contents("period", 700_000)
    a = handle.bgzf_compress(data)
    assert handle.bgzf_compress(data) == a
    with capi.Handle(0) as h2:
        assert h2.bgzf_compress(data) == a


@pytest.mark.parametrize("text", [_sam_text, _m8_text])
def test_ratio_against_zlib_level_1(handle, text):
    data = text(4_000_000)
    out = handle.bgzf_compress(data)
    z1 = 0
    for i in range(0, len(data), BLOCK):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z1 += len(c.compress(data[i:i + BLOCK]) + c.flush())
    assert len(out) <= 1.05 * z1, (len(out), z1)


@pytest.mark.parametrize("program", PROGRAMS)
def test_write_records_bgzf_every_format(handle, tmp_path, program):
    m, ops, names, qa, qoff = _case(program, seed=21)
    opt, keep = _options(program, ALL_TAGS, capi.LX_SAM_SEQ_UNIQ, 1, True, m, 4)
    args = (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"])
    for fmt in (capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS, capi.LX_OUT_SAM, capi.LX_OUT_BAM):
        p = tmp_path / f"o{fmt}.gz"
        handle.write_records_bgzf(p, fmt, *args, program=program, q_ascii=qa, q_ascii_off=qoff, options=opt, footer_records=6)
        raw = p.read_bytes()
        assert raw.endswith(EOF_MEMBER)
        assert gzip.decompress(raw) == _render(fmt, program, m, ops, names, qa, qoff, opt, footer=6)
    sam = tmp_path / "o.sam"
    capi.write_records(sam, capi.LX_OUT_SAM, *args, program=program, q_ascii=qa, q_ascii_off=qoff, options=opt)
    assert bam_decode.to_sam(gzip.decompress((tmp_path / f"o{capi.LX_OUT_BAM}.gz").read_bytes())) == sam.read_text().splitlines()


def test_compress_refuses_a_short_buffer(handle):
    import ctypes as C
    buf = np.zeros(100, np.uint8)
    got = C.c_uint64(0)
    rc = handle.lib.lx_bgzf_compress(handle.h, buf.ctypes.data, 100, buf.ctypes.data, 100, C.byref(got), 0)
    assert rc == capi.LX_EINVAL
    rc = handle.lib.lx_bgzf_compress(handle.h, buf.ctypes.data, 1, buf.ctypes.data, 100, C.byref(got), 2)
    assert rc == capi.LX_EINVAL


def _small(tmp):
    from tests.test_cli import _small_dbs
    _small_dbs(tmp)


@pytest.mark.parametrize("cmd,q,d", [("searchn", "r.fasta", "g.fasta"), ("searchp", "pq.fasta", "db.fasta")])
def test_cli_bam_and_gz_outputs(tmp_path, cmd, q, d):
    _small(tmp_path)
    cli = build.build_cli()

    def run(name, *extra):
        r = subprocess.run([str(cli), cmd, "-q", str(tmp_path / q), "-d", str(tmp_path / d), "-o", str(tmp_path / name),
                            "--version-to-outputfile", "0", *extra], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stderr

    err = run("x.bam")
    assert "BGZF compression on the GPU" in err, err
    run("x.sam", "--sam-with-refheader", "on")
    bam = gzip.decompress((tmp_path / "x.bam").read_bytes())
    assert bam_decode.to_sam(bam) == (tmp_path / "x.sam").read_text().splitlines()
    for ext in ("m9", "m8"):
        run(f"x.{ext}")
        run(f"x.{ext}.gz")
        assert gzip.decompress((tmp_path / f"x.{ext}.gz").read_bytes()) == (tmp_path / f"x.{ext}").read_bytes()
