"""`lambda3 search* --lazy-query 1 / --query-block N`: the query file searched block by block writes the bytes the eager run writes.
The eager output is the yardstick throughout.  One base configuration (searchp, .m8, 300 reads against 800 subjects) takes every
block size of {1, 7, n-1, n, n+1}; every other axis -- program, output format, --render, --records, --search0, --devices 0,0,
taxonomy columns with the LCA, FASTQ / BGZF / plain-gzip query files -- is varied against it with blocks of 7 (and 1 where the
groups matter most), and one case combines them.  The last test holds the peak memory of a lazy run of a 64 MB query file against
the eager run's.  Every process runs alone, under a time limit."""
import gzip
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from lambda_amd import build
from tests.test_cli import CODONS, _fasta, _make_config1
from tests.test_gzip_input import bgzf
from tests.test_taxonomy import world

pytestmark = pytest.mark.gpu
N = 300
BLOCKS = [1, 7, N - 1, N, N + 1]
COMP = str.maketrans("ACGT", "TGCA")


def _run(cwd, *args, timeout=120):
    r = subprocess.run([str(build.build_cli()), *map(str, args)], capture_output=True, text=True, cwd=cwd, timeout=timeout)
    return r


def _fastq(path, ids, seqs):
    with open(path, "w") as f:
        for k, (i, s) in enumerate(zip(ids, seqs)):  # qualities that begin with "@", "+" and ">" among them
            f.write(f"@{i}\n{s}\n+\n{'@+>I'[k % 4] + 'I' * (len(s) - 1)}\n")


@pytest.fixture(scope="module")
def world_dir(tmp_path_factory):
    """The inputs, made once: protein, translated, nucleotide and bisulfite reads with their databases, and the query files' other forms."""
    tmp = tmp_path_factory.mktemp("query_blocks")
    qs, _, _ = _make_config1(tmp, nq=N, ndb=800)
    ids = [f"q{k} len=100" for k in range(N)]
    _fasta(tmp / "qx.fasta", ids, ["".join(CODONS[a][0] for a in q) for q in qs])  # the same reads as nucleotides: BLASTX
    _fastq(tmp / "q.fastq", ids, qs)
    text = (tmp / "q.fasta").read_bytes()
    (tmp / "q.fasta.bgz").write_bytes(bgzf(text[:len(text) // 2]) + bgzf(text[len(text) // 2:]) + bgzf(b""))
    (tmp / "q.fasta.gz").write_bytes(gzip.compress(text[:9000]) + gzip.compress(text[9000:]))
    rng = np.random.default_rng(5)
    genome = ["".join("ACGT"[i] for i in rng.integers(0, 4, 20000)) for _ in range(3)]
    reads, bs_reads = [], []
    for k in range(N):
        c, a = int(rng.integers(0, 3)), int(rng.integers(0, 19800))
        r = list(genome[c][a:a + 150])
        for p in rng.integers(0, 150, 4):
            r[p] = "ACGT"[int(rng.integers(0, 4))]
        r = "".join(r)
        r = r.translate(COMP)[::-1] if k % 2 else r
        reads.append(r)
        bs_reads.append(r.replace("G", "A") if k % 4 >= 2 else r.replace("C", "T"))
    _fasta(tmp / "g.fasta", [f"chr{i}" for i in range(3)], genome)
    _fasta(tmp / "r.fasta", [f"read{k} x" for k in range(N)], reads)
    _fasta(tmp / "rbs.fasta", [f"read{k} x" for k in range(N)], bs_reads)
    return tmp


def _same(cwd, cmd, q, db, ext, extra=(), blocks=(7,), lazy_extra=(), n=N, min_lines=20):
    """The eager file, then one lazy run per block size: the same bytes, and the third stderr line with the block count."""
    base = [cmd, "-q", q, *db, "--version-to-outputfile", "0", *extra]
    r = _run(cwd, *base, "-o", f"eager.{ext}")
    assert r.returncode == 0, r.stderr
    assert "lambda3 query blocks" not in r.stderr
    want = (cwd / f"eager.{ext}").read_bytes()
    if ext in ("m8", "m9", "sam"):
        assert len(want.splitlines()) >= min_lines
    for b in blocks:
        r = _run(cwd, *base, *lazy_extra, "--query-block", b, "-o", f"lazy.{ext}")
        assert r.returncode == 0, (b, r.stderr)
        assert (cwd / f"lazy.{ext}").read_bytes() == want, (cmd, ext, extra, b)
        line = next(l for l in r.stderr.splitlines() if l.startswith("lambda3 query blocks: "))
        assert line.startswith(f"lambda3 query blocks: {math.ceil(n / b)} block(s) of at most {b} read(s), {min(b, n)} read(s) in the largest"), line
        alive, handles = int(line.rsplit("at most ", 1)[1].split()[0]), 2 if "0,0" in extra else 1
        assert 1 <= alive <= handles + 2, line
        assert sum(l.startswith("lambda3 ") for l in r.stderr.splitlines()) == 3
    return want


def test_every_block_size_on_the_base_configuration(world_dir):
    _same(world_dir, "searchp", "q.fasta", ["-d", "db.fasta"], "m8", blocks=BLOCKS)


def test_lazy_query_switch_and_its_off_position(world_dir):
    base = ["searchp", "-q", "q.fasta", "-d", "db.fasta", "--version-to-outputfile", "0"]
    eager = _run(world_dir, *base, "-o", "e.m8")
    off = _run(world_dir, *base, "--lazy-query", "0", "-o", "off.m8")
    zero = _run(world_dir, *base, "--lazy-query", "1", "--query-block", "0", "-o", "zero.m8")
    on = _run(world_dir, *base, "--lazy-query", "1", "-o", "on.m8")
    assert eager.returncode == off.returncode == zero.returncode == on.returncode == 0, on.stderr
    heads = lambda r: [l for l in r.stderr.splitlines() if l.startswith("lambda3 ")]
    first = lambda r: next(l for l in r.stderr.splitlines() if l.startswith("lambda3 searchp"))
    # --lazy-query 0 and --query-block 0 are the eager path: the same two lines (the times aside), no third one
    for r in (off, zero):
        assert len(heads(r)) == 2 and first(r) == first(eager) and "lambda3 query blocks" not in r.stderr
    assert first(on) == first(eager)  # (the counts are summed over the blocks: one block here)
    assert "lambda3 query blocks: 1 block(s) of at most 1048576 read(s), 300 read(s) in the largest" in on.stderr
    want = (world_dir / "e.m8").read_bytes()
    assert all((world_dir / f).read_bytes() == want for f in ("off.m8", "zero.m8", "on.m8"))
    bad = _run(world_dir, *base, "--query-block", "-3", "-o", "x.m8")
    assert bad.returncode != 0 and "--query-block" in bad.stderr


@pytest.mark.parametrize("cmd,q,db", [("searchp", "qx.fasta", "db.fasta"), ("searchn", "r.fasta", "g.fasta"), ("searchbs", "rbs.fasta", "g.fasta")])
def test_programs(world_dir, cmd, q, db):
    extra = ["-a", "dna5"] if q == "qx.fasta" else []
    _same(world_dir, cmd, q, ["-d", db], "m8", extra=extra, blocks=(1, 7))
    _same(world_dir, cmd, q, ["-d", db], "sam", extra=extra)


@pytest.mark.parametrize("ext", ["m9", "sam", "bam", "m8.gz"])
@pytest.mark.parametrize("render", ["host", "gpu"])
def test_formats_and_render_sides(world_dir, ext, render):
    _same(world_dir, "searchp", "q.fasta", ["-d", "db.fasta"], ext, extra=["--render", render], blocks=(1, 7))


@pytest.mark.parametrize("extra", [["--records", "gpu"], ["--records", "host"], ["--search0", "0"], ["--search0", "1"], ["--devices", "0,0"],
                                   ["--seeding", "host"]], ids=lambda e: "".join(e).strip("-"))
def test_records_search0_devices(world_dir, extra):
    _same(world_dir, "searchp", "q.fasta", ["-d", "db.fasta"], "m8", extra=extra)


@pytest.mark.parametrize("q", ["q.fastq", "q.fasta.bgz", "q.fasta.gz"])
def test_query_file_forms(world_dir, q):
    want = _same(world_dir, "searchp", q, ["-d", "db.fasta"], "m8", blocks=(7, N + 1))
    assert want == _same(world_dir, "searchp", "q.fasta", ["-d", "db.fasta"], "m8", blocks=())


def test_taxonomy_columns_with_the_lca(tmp_path):
    ids, seqs = world(tmp_path, dup=True)
    with open(tmp_path / "q.fasta", "w") as f:
        for k in range(0, len(seqs), 3):
            f.write(f">q{k}\n{seqs[k][5:75]}\n")
    n = len(range(0, len(seqs), 3))
    r = _run(tmp_path, "mkindexp", "-d", "db.fasta", "-i", "db.lba", "-m", "m.accession2taxid", "-x", "dump")
    assert r.returncode == 0, r.stderr
    _same(tmp_path, "searchp", "q.fasta", ["-i", "db.lba"], "m8", extra=["--output-columns", "std staxids lcataxid"], blocks=(1, 7), n=n, min_lines=10)
    _same(tmp_path, "searchp", "q.fasta", ["-i", "db.lba"], "sam", extra=["--sam-bam-tags", "AS st lt ls"], blocks=(7,), n=n, min_lines=10)


def test_everything_at_once(world_dir):
    _same(world_dir, "searchn", "r.fasta", ["-d", "g.fasta"], "bam", extra=["--render", "gpu", "--records", "gpu", "--devices", "0,0", "--sam-bam-seq", "uniq"],
          blocks=(7, 64))


def test_an_error_in_a_later_block_keeps_the_blocks_before_it(world_dir):
    """A malformed FASTQ record in block 2: the run ends non-zero with the eager run's message; the file holds blocks 0 and 1."""
    text = (world_dir / "q.fastq").read_text().split("\n")
    good = "\n".join(text[:4 * 20]) + "\n"
    (world_dir / "bad.fastq").write_text(good + "@broken\nACDEF\n+\nII\n")
    (world_dir / "good.fastq").write_text(good)
    eager = _run(world_dir, "searchp", "-q", "bad.fastq", "-d", "db.fasta", "-o", "bad_eager.m8")
    lazy = _run(world_dir, "searchp", "-q", "bad.fastq", "-d", "db.fasta", "-o", "bad_lazy.m8", "--query-block", "10")
    assert eager.returncode != 0 and lazy.returncode != 0 and not (world_dir / "bad_eager.m8").exists()
    msg = "FASTQ record 'broken' has 2 quality characters for 5 letters"
    assert msg in eager.stderr and msg in lazy.stderr
    r = _run(world_dir, "searchp", "-q", "good.fastq", "-d", "db.fasta", "-o", "good.m8")
    assert r.returncode == 0 and (world_dir / "bad_lazy.m8").read_bytes() == (world_dir / "good.m8").read_bytes()


_WAIT4 = """
import os, subprocess, sys
p = subprocess.Popen(sys.argv[1:], stdout=subprocess.DEVNULL)
_, status, ru = os.wait4(p.pid, 0)
print(os.waitstatus_to_exitcode(status), ru.ru_maxrss)
"""


def _peak_rss(cwd, *args, timeout=300):
    """(return code, stderr, ru_maxrss in bytes) of one run, from os.wait4 in a small process of its own: a child's ru_maxrss begins at
    what its parent held when it forked, and this test process holds more than the runs that are measured."""
    r = subprocess.run([sys.executable, "-c", _WAIT4, str(build.build_cli()), *map(str, args)], cwd=cwd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    rc, kib = map(int, r.stdout.split())
    return rc, r.stderr, kib * 1024


def test_lazy_run_holds_less_memory_by_at_least_the_query_file(tmp_path):
    """One FASTA of random 150-nt reads of 64 MB against a small database.  The eager run holds the letters, two frames of ranks and
    their reduced copy -- over three times the file -- which the lazy run never holds: rss(eager) - rss(lazy) >= the file's size."""
    rng = np.random.default_rng(77)
    n = 64_000_000 // 160 + 1
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, 150))]
    with open(tmp_path / "big.fasta", "wb") as f:
        for lo in range(0, n, 50_000):
            f.write(b"".join(b">r%07d\n" % k + letters[k].tobytes() + b"\n" for k in range(lo, min(n, lo + 50_000))))
    size = (tmp_path / "big.fasta").stat().st_size
    assert size >= 64_000_000
    genome = ["".join("ACGT"[i] for i in rng.integers(0, 4, 5000)) for _ in range(2)]
    _fasta(tmp_path / "g.fasta", ["chrA", "chrB"], genome)
    base = ["searchn", "-q", "big.fasta", "-d", "g.fasta", "--version-to-outputfile", "0"]
    rc_e, err_e, rss_e = _peak_rss(tmp_path, *base, "-o", "eager.m8")
    rc_l, err_l, rss_l = _peak_rss(tmp_path, *base, "--query-block", "20000", "-o", "lazy.m8")
    assert rc_e == 0 and rc_l == 0, (err_e[-2000:], err_l[-2000:])
    print(f"query file {size} bytes; peak RSS eager {rss_e}, lazy {rss_l}, difference {rss_e - rss_l}")
    assert (tmp_path / "eager.m8").read_bytes() == (tmp_path / "lazy.m8").read_bytes()
    assert f"{math.ceil(n / 20000)} block(s)" in err_l
    assert rss_e - rss_l >= size, (rss_e, rss_l, size)
