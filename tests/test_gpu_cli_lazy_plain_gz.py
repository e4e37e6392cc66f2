"""`lambda3 searchn --lazy-query 1` on a plain-gzip FASTQ (one member, as gzip and pigz write it): the reader's stream decodes the
member on the device, wave by wave, and the run writes the bytes of the eager run and of the run on the uncompressed file.  The
front end has no switch for LX_OPT_GUNZIP_PARALLEL_FROM, so the file is made larger than the default threshold of 8 MiB: 20 000
reads of 150 bp whose header lines carry a comment of random letters, which gzip cannot shrink much.  The database is three
contigs of 20 000 bp.  Every process runs alone, under a time limit."""
import gzip
import re
import subprocess

import numpy as np
import pytest

from lambda_amd import build
from tests.test_cli import _fasta

pytestmark = pytest.mark.gpu
READS, LEN, COMMENT = 20_000, 150, 340
COMP = str.maketrans("ACGT", "TGCA")


def _run(cwd, *args, timeout=120):
    return subprocess.run([str(build.build_cli()), *map(str, args)], capture_output=True, text=True, cwd=cwd, timeout=timeout)


@pytest.fixture(scope="module")
def world_dir(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lazy_plain_gz")
    rng = np.random.default_rng(17)
    genome = ["".join("ACGT"[i] for i in rng.integers(0, 4, 20000)) for _ in range(3)]
    _fasta(tmp / "g.fasta", [f"chr{i}" for i in range(3)], genome)
    letters = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/", np.uint8)
    comments = letters[rng.integers(0, 64, (READS, COMMENT))]
    quals = (rng.integers(0, 41, (READS, LEN)) + 33).astype(np.uint8)
    where, starts = rng.integers(0, 3, READS), rng.integers(0, 20000 - LEN, READS)
    out = []
    for k in range(READS):
        r = list(genome[where[k]][starts[k]:starts[k] + LEN])
        for p in rng.integers(0, LEN, 3):
            r[p] = "ACGT"[int(rng.integers(0, 4))]
        r = "".join(r)
        r = r.translate(COMP)[::-1] if k % 2 else r
        out.append(b"@read%d %s\n%s\n+\n%s\n" % (k, comments[k].tobytes(), r.encode(), quals[k].tobytes()))
    text = b"".join(out)
    (tmp / "r.fastq").write_bytes(text)
    raw = gzip.compress(text, 6)
    assert len(raw) - 18 >= 8 << 20  # LX_OPT_GUNZIP_PARALLEL_FROM's default, counted from behind the header
    (tmp / "r.fastq.gz").write_bytes(raw)
    return tmp


def test_lazy_search_of_a_plain_gzip_fastq(world_dir):
    base = ["searchn", "-d", "g.fasta", "--version-to-outputfile", "0"]
    plain = _run(world_dir, *base, "-q", "r.fastq", "-o", "plain.m8")
    eager = _run(world_dir, *base, "-q", "r.fastq.gz", "-o", "eager.m8")
    lazy = _run(world_dir, *base, "-q", "r.fastq.gz", "--lazy-query", "1", "--query-block", "4096", "-o", "lazy.m8")
    assert plain.returncode == eager.returncode == lazy.returncode == 0, (plain.stderr, eager.stderr, lazy.stderr)
    want = (world_dir / "plain.m8").read_bytes()
    assert len(want.splitlines()) >= READS // 2
    assert (world_dir / "eager.m8").read_bytes() == want
    assert (world_dir / "lazy.m8").read_bytes() == want
    note = re.search(r"query stream: (\d+) plain member\(s\) in (\d+) chunks on the GPU", lazy.stderr)
    assert note and int(note.group(1)) == 1 and int(note.group(2)) >= 64 and "decline" not in lazy.stderr, lazy.stderr
    assert re.search(r"1 plain member\(s\) in \d+ chunks on the GPU", eager.stderr), eager.stderr  # the eager path's own note
    line = next(l for l in lazy.stderr.splitlines() if l.startswith("lambda3 query blocks: "))
    assert line.startswith("lambda3 query blocks: 5 block(s) of at most 4096 read(s), 4096 read(s) in the largest"), line
