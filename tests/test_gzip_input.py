"""lx_gunzip on the host (h = NULL) and the front end's compressed / FASTQ inputs without a GPU: streams made by Python's gzip and
zlib decode to exactly their bytes, corrupt ones are refused with LX_EINVAL and a message, and mkindex* writes the same index from
db.fasta.gz, BGZF, FASTQ and FASTQ+gzip as from the plain FASTA."""
import gzip
import struct
import subprocess
import zlib

import numpy as np
import pytest

from lambda_amd import build, capi
from tests.test_cli import _fasta, _small_dbs

BLOCK = 65280


def fasta_text(n, seed=0):
    rng = np.random.default_rng(seed)
    out, size = [], 0
    k = 0
    while size < n:
        rec = f">seq{k} protein {k}\n" + "".join("ACDEFGHIKLMNPQRSTVWY"[i] for i in rng.integers(0, 20, 60)) + "\n"
        out.append(rec)
        size += len(rec)
        k += 1
    return "".join(out).encode()[:n]


def bgzf(data: bytes, level=6) -> bytes:
    """BGZF made in Python: raw DEFLATE per 65 280-byte block behind the BC header, CRC32 + ISIZE trailer."""
    out = []
    for i in range(0, max(len(data), 1), BLOCK):
        blk = data[i:i + BLOCK]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        d = c.compress(blk) + c.flush()
        out.append(struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, ord("B"), ord("C"), 2, len(d) + 25) + d +
                   struct.pack("<II", zlib.crc32(blk), len(blk)))
    return b"".join(out)


def gz_with_fields(data: bytes, fname=b"", comment=b"", hcrc=False, extra=b"") -> bytes:
    flg = (8 if fname else 0) | (16 if comment else 0) | (2 if hcrc else 0) | (4 if extra else 0)
    h = struct.pack("<BBBBIBB", 0x1F, 0x8B, 8, flg, 0, 0, 3)
    if extra:
        h += struct.pack("<H", len(extra)) + extra
    if fname:
        h += fname + b"\0"
    if comment:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return h + c.compress(data) + c.flush() + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


SIZES = [0, 1, 65280, 65536, 65537]


def _inputs(n):
    return {"fasta": fasta_text(n, n), "random": np.random.default_rng(n).bytes(n)}


@pytest.mark.parametrize("n", SIZES)
def test_host_levels_strategies_bgzf(n):
    for kind, data in _inputs(n).items():
        for level in (0, 1, 6, 9):
            assert capi.gunzip(None, gzip.compress(data, level)) == data, (kind, level)
        for st in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
            c = zlib.compressobj(6, zlib.DEFLATED, 31, 9, st)
            assert capi.gunzip(None, c.compress(data) + c.flush()) == data, (kind, st)
        assert capi.gunzip(None, bgzf(data)) == data, kind


def test_host_header_fields_and_members():
    data = fasta_text(100_000, 3)
    for kw in ({"fname": b"db.fasta"}, {"comment": b"a comment"}, {"hcrc": True}, {"extra": b"XY\x03\x00abc"},
               {"fname": b"x", "comment": b"y", "hcrc": True, "extra": b"AB\x00\x00"}):
        assert capi.gunzip(None, gz_with_fields(data, **kw)) == data, kw
    assert capi.gunzip(None, gzip.compress(b"")) == b""
    parts = [fasta_text(70_000, 5), b"", np.random.default_rng(2).bytes(1000), fasta_text(10, 6)]
    assert capi.gunzip(None, b"".join(gzip.compress(p) for p in parts)) == b"".join(parts)
    # BGZF followed by plain members
    assert capi.gunzip(None, bgzf(parts[0]) + gzip.compress(parts[2]) + bgzf(parts[3])) == parts[0] + parts[2] + parts[3]
    # a wrong header CRC16
    bad = bytearray(gz_with_fields(data, hcrc=True))
    bad[10] ^= 1
    with pytest.raises(capi.LambdaExtError, match="CRC16"):
        capi.gunzip(None, bytes(bad))


def _refused(stream: bytes, what: str):
    with pytest.raises(capi.LambdaExtError) as e:
        capi.gunzip(None, stream)
    assert e.value.code == capi.LX_EINVAL and "lx_gunzip: member" in str(e.value), (what, str(e.value))
    return str(e.value)


def corrupt_cases():
    """(name, stream, member that is bad): the corrupt inputs both paths must refuse."""
    data = fasta_text(200_000, 9)
    good = bgzf(data)
    sizes = []
    p = 0
    while p < len(good):
        sizes.append(struct.unpack_from("<H", good, p + 16)[0] + 1)
        p += sizes[-1]
    m1 = sizes[0]  # member 1 starts here
    cases = []
    # a flipped bit in a dynamic block header (HCLEN / code lengths of member 1)
    b = bytearray(good)
    b[m1 + 18 + 2] ^= 0x10
    cases.append(("dynamic header bit", bytes(b), 1))
    # a truncated member (the last one cut short: BSIZE then points past the end)
    cases.append(("truncated", good[:-100], len(sizes) - 1))
    # a wrong CRC
    b = bytearray(good)
    b[m1 + sizes[1] - 8] ^= 0xFF
    cases.append(("crc", bytes(b), 1))
    # a wrong ISIZE
    b = bytearray(good)
    b[m1 + sizes[1] - 4] ^= 0x01
    cases.append(("isize", bytes(b), 1))
    # a distance before the start of the output: a fixed block whose first symbol is a match
    bits = [1, 1, 0]  # BFINAL, BTYPE 01 (LSB first)
    bits += [0, 0, 0, 0, 0, 0, 1]  # length symbol 257 (code 0000001), length 3
    bits += [0, 0, 0, 0, 0]  # distance symbol 0: distance 1, with no output yet
    bits += [0] * 7  # end of block
    raw = bytes(sum(bit << i for i, bit in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))
    member = struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, ord("B"), ord("C"), 2, len(raw) + 25) + raw + struct.pack("<II", 0, 3)
    cases.append(("distance", good[:m1] + member, 1))
    # BSIZE past the end of the data
    b = bytearray(good[:m1 + sizes[1]])
    struct.pack_into("<H", b, m1 + 16, sizes[1] + 500)
    cases.append(("bsize", bytes(b), 1))
    return cases


@pytest.mark.parametrize("case", range(6))
def test_host_refuses_corrupt(case):
    name, stream, member = corrupt_cases()[case]
    msg = _refused(stream, name)
    assert f"member {member} " in msg, (name, msg)


def test_host_refuses_corrupt_plain():
    g = gzip.compress(fasta_text(100_000, 4))
    _refused(g[:-20], "truncated plain")
    b = bytearray(g)
    b[-8] ^= 1
    assert "CRC32" in _refused(bytes(b), "crc plain")
    b = bytearray(g)
    b[-1] ^= 1
    assert "ISIZE" in _refused(bytes(b), "isize plain")
    _refused(g + b"junk", "trailing junk")


def _fastq(path, ids, seqs, qual_len=None):
    with open(path, "w") as f:
        for i, s in zip(ids, seqs):
            q = "I" * (len(s) if qual_len is None else qual_len)
            f.write(f"@{i}\n{s[:len(s) // 2]}\n{s[len(s) // 2:]}\n+\n{q[:7]}\n{q[7:]}\n")


def _read_fasta(path):
    ids, seqs = [], []
    for line in open(path):
        line = line.rstrip("\n")
        if line.startswith(">"):
            ids.append(line[1:])
            seqs.append("")
        elif line:
            seqs[-1] += line
    return ids, seqs


def compressed_variants(tmp, name):
    """name.fasta -> name.fasta.gz (plain gzip), name.bgzf.fasta.gz, name.fastq, name.fastq.gz (BGZF); returns the paths."""
    src = tmp / f"{name}.fasta"
    data = src.read_bytes()
    ids, seqs = _read_fasta(src)
    out = {"fasta": src}
    (tmp / f"{name}.fasta.gz").write_bytes(gzip.compress(data, 6))
    out["gzip"] = tmp / f"{name}.fasta.gz"
    (tmp / f"{name}.bgzf.fasta.gz").write_bytes(bgzf(data) + bgzf(b""))
    out["bgzf"] = tmp / f"{name}.bgzf.fasta.gz"
    _fastq(tmp / f"{name}.fastq", ids, seqs)
    out["fastq"] = tmp / f"{name}.fastq"
    (tmp / f"{name}.fastq.gz").write_bytes(bgzf((tmp / f"{name}.fastq").read_bytes()))
    out["fastq_bgzf"] = tmp / f"{name}.fastq.gz"
    return out


@pytest.mark.parametrize("cmd,name", [("mkindexp", "db"), ("mkindexn", "g"), ("mkindexbs", "g")])
def test_mkindex_from_compressed_and_fastq(tmp_path, cmd, name):
    _small_dbs(tmp_path)
    cli = str(build.build_cli())
    variants = compressed_variants(tmp_path, name)
    index = {}
    for kind, path in variants.items():
        out = tmp_path / f"{kind}.{cmd}.lba"
        r = subprocess.run([cli, cmd, "-d", str(path), "-i", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, (kind, r.stderr)
        if kind in ("gzip", "bgzf", "fastq_bgzf"):
            assert "gzip decompression on the host" in r.stderr, r.stderr
        index[kind] = out.read_bytes()
    for kind, b in index.items():
        assert b == index["fasta"], kind


def test_fastq_quality_length_and_bzip2_refused(tmp_path):
    cli = str(build.build_cli())
    _fastq(tmp_path / "bad.fastq", ["r1", "r2"], ["ACDEFGHIKLMNPQRSTVWY" * 3] * 2, qual_len=59)
    r = subprocess.run([cli, "mkindexp", "-d", str(tmp_path / "bad.fastq")], capture_output=True, text=True)
    assert r.returncode != 0 and "FASTQ record 'r1'" in r.stderr and "quality" in r.stderr, r.stderr
    import bz2

    _fasta(tmp_path / "d.fasta", ["s"], ["ACDEFGHIKLMNPQRSTVWY" * 5])
    (tmp_path / "d.fasta.bz2").write_bytes(bz2.compress((tmp_path / "d.fasta").read_bytes()))
    r = subprocess.run([cli, "mkindexp", "-d", str(tmp_path / "d.fasta.bz2")], capture_output=True, text=True)
    assert r.returncode != 0 and "bzip2" in r.stderr, r.stderr
    # a corrupt gzip database is refused with the decoder's message
    (tmp_path / "c.fasta.gz").write_bytes(gzip.compress((tmp_path / "d.fasta").read_bytes())[:-5])
    r = subprocess.run([cli, "mkindexp", "-d", str(tmp_path / "c.fasta.gz")], capture_output=True, text=True)
    assert r.returncode != 0 and "lx_gunzip: member 0" in r.stderr, r.stderr
