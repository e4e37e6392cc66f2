"""GPU tests of the BGZF decoder (lx_gunzip.hip): BGZF made by Python and by lx_bgzf_compress (past several streaming chunks),
BGZF followed by plain members, corrupt members refused by name with the handle still usable after, and the lambda3 front end on
plain-gzip, BGZF, FASTQ and FASTQ+BGZF inputs giving the same output as on plain FASTA."""
import gzip
import shutil
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests.test_cli import _small_dbs
from tests.test_gzip_input import bgzf, compressed_variants, corrupt_cases, fasta_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


@pytest.mark.parametrize("n", [0, 1, 65280, 65536, 65537, 3_000_000])
def test_device_python_bgzf(handle, n):
    for data in (fasta_text(n, n), np.random.default_rng(n).bytes(n)):
        stream = bgzf(data) + bgzf(b"")
        assert capi.gunzip(handle, stream) == data
        if n > 65536:
            assert handle.last_phase_ms(5)[1] >= 1  # the kernel ran


@pytest.mark.parametrize("n", [1, 65280 * 3 + 17, 40_000_000, 100_000_000])
def test_device_own_bgzf(handle, n):
    rng = np.random.default_rng(n)
    unit = fasta_text(1 << 20, 7)
    data = (unit * (n // len(unit) + 1))[:n]
    if n < 1_000_000:
        data = rng.bytes(n)
    assert capi.gunzip(handle, handle.bgzf_compress(data, eof=True)) == data


def test_device_bgzf_then_plain(handle):
    a, b, c = fasta_text(500_000, 1), np.random.default_rng(3).bytes(70_000), fasta_text(200_000, 2)
    stream = bgzf(a) + gzip.compress(b) + bgzf(c) + bgzf(b"")
    assert capi.gunzip(handle, stream) == a + b + c


def test_device_refuses_corrupt_then_recovers(handle):
    # (the same cases pass the host path in tests/test_gzip_input.py first)
    for name, stream, member in corrupt_cases():
        with pytest.raises(capi.LambdaExtError) as e:
            capi.gunzip(handle, stream)
        assert e.value.code == capi.LX_EINVAL and f"lx_gunzip: member {member} " in str(e.value), (name, str(e.value))
    data = fasta_text(1_000_000, 11)
    assert capi.gunzip(handle, bgzf(data)) == data


def _run(cli, cwd, *args):
    r = subprocess.run([cli, *args], capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("cmd,q,d", [("searchp", "pq", "db"), ("searchn", "r", "g"), ("searchbs", "bs", "g")])
def test_cli_compressed_inputs_give_the_same_output(tmp_path, cmd, q, d):
    _small_dbs(tmp_path)
    cli = str(build.build_cli())
    qv, dv = compressed_variants(tmp_path, q), compressed_variants(tmp_path, d)
    outs = {}
    for kind in qv:
        # the same relative names in a directory per variant: the command line (SAM @PG) is the same
        w = tmp_path / kind
        w.mkdir()
        shutil.copy(qv[kind], w / "q.in")
        shutil.copy(dv[kind], w / "d.in")
        for ext in ("m8", "sam"):
            r = _run(cli, w, cmd, "-q", "q.in", "-d", "d.in", "-o", f"o.{ext}", "-e", "10")
            if kind in ("gzip", "bgzf", "fastq_bgzf"):
                assert "gzip decompression" in r.stderr, r.stderr
            if kind in ("bgzf", "fastq_bgzf"):
                assert "of BGZF on the GPU" in r.stderr, r.stderr
            outs[kind, ext] = (w / f"o.{ext}").read_bytes()
    for (kind, ext), b in outs.items():
        assert len(b) > 0 and b == outs["fasta", ext], (kind, ext)


def test_cli_blastx_from_gz_and_index_from_gz(tmp_path):
    _small_dbs(tmp_path)
    cli = str(build.build_cli())
    rv = compressed_variants(tmp_path, "r")
    (tmp_path / "x").mkdir()
    (tmp_path / "y").mkdir()
    shutil.copy(rv["fasta"], tmp_path / "x" / "q.in")
    shutil.copy(rv["gzip"], tmp_path / "y" / "q.in")
    for w in ("x", "y"):
        shutil.copy(tmp_path / "db.fasta", tmp_path / w / "d.in")
        r = _run(cli, tmp_path / w, "searchp", "-q", "q.in", "-d", "d.in", "-o", "o.m8", "-e", "10")
        assert "blastx" in r.stderr, r.stderr
    assert (tmp_path / "x" / "o.m8").read_bytes() == (tmp_path / "y" / "o.m8").read_bytes()
    # search -i on an index made from db.fasta.gz equals search -d db.fasta
    dv = compressed_variants(tmp_path, "db")
    _run(cli, tmp_path, "mkindexp", "-d", str(dv["gzip"]), "-i", str(tmp_path / "gz.lba"))
    _run(cli, tmp_path, "searchp", "-q", str(tmp_path / "pq.fasta"), "-i", str(tmp_path / "gz.lba"), "-o", str(tmp_path / "i.m8"), "-e", "10")
    _run(cli, tmp_path, "searchp", "-q", str(tmp_path / "pq.fasta"), "-d", str(tmp_path / "db.fasta"), "-o", str(tmp_path / "d.m8"), "-e", "10")
    assert (tmp_path / "i.m8").read_bytes() == (tmp_path / "d.m8").read_bytes() and (tmp_path / "d.m8").stat().st_size > 0
