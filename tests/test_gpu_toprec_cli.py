"""`lambda3 --records gpu` against `--records host`: _writeRecord's sort / unique / sort / cut on the device inside the Level-2 call
(lx_iterate_matches_dev_top) gives byte-identical .m8, .sam and .bam files and the same statistics on stderr, for searchp, searchn
and searchbs, cut to one record per query and to 25."""
import re
import subprocess

import numpy as np
import pytest

from tests.test_cli import STD, _cli, _fasta


def _mutate(rng, seq, letters, rate):
    s = list(seq)
    for p in np.flatnonzero(rng.random(len(s)) < rate):
        s[p] = letters[int(rng.integers(0, len(letters)))]
    return "".join(s)


def _inputs(tmp, program):
    """Queries with MANY subjects each: families of diverged copies, so that -n 1 and -n 25 both cut."""
    rng = np.random.default_rng({"searchp": 1, "searchn": 2, "searchbs": 3}[program])
    if program == "searchp":
        base = ["".join(STD[i] for i in rng.integers(0, 20, 220)) for _ in range(12)]
        subj = [_mutate(rng, b, STD, 0.12) for b in base for _ in range(30)]
        qry = [_mutate(rng, b, STD, 0.08)[20:200] for b in base for _ in range(3)]
    else:
        base = ["".join("ACGT"[i] for i in rng.integers(0, 4, 400)) for _ in range(10)]
        filler = lambda: "".join("ACGT"[i] for i in rng.integers(0, 4, 300))
        subj = [filler() + _mutate(rng, b, "ACGT", 0.04) + filler() for b in base for _ in range(30)]
        qry = [_mutate(rng, b, "ACGT", 0.03)[100:250] for b in base for _ in range(4)]
        comp = str.maketrans("ACGT", "TGCA")
        qry = [q.translate(comp)[::-1] if k % 2 else q for k, q in enumerate(qry)]
        if program == "searchbs":
            qry = [q.replace("C", "T") if k % 4 < 2 else q.replace("G", "A") for k, q in enumerate(qry)]
    _fasta(tmp / "d.fasta", [f"s{i}" for i in range(len(subj))], subj)
    _fasta(tmp / "q.fasta", [f"q{i}" for i in range(len(qry))], qry)


def _stats(stderr):
    m = re.search(r"seeds (\d+) -> promising (\d+) -> windows (\d+) -> traced (\d+) -> HSPs (\d+) -> written (\d+) \(queries with hit: (\d+)\)", stderr)
    assert m, stderr
    return m.groups()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 25])
@pytest.mark.parametrize("program", ["searchp", "searchn", "searchbs"])
def test_records_on_the_gpu_write_the_same_files(tmp_path, program, n):
    _inputs(tmp_path, program)
    written = None
    for ext in ("m8", "sam", "bam"):
        got = {}
        for where in ("host", "gpu"):
            out = tmp_path / f"{where}.{ext}"
            r = subprocess.run([str(_cli()), program, "-q", str(tmp_path / "q.fasta"), "-d", str(tmp_path / "d.fasta"), "-o", str(out), "-n", str(n),
                                "--records", where, "--version-to-outputfile", "0"], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert ("kernels on the GPU" in r.stderr) == (where == "gpu"), r.stderr
            got[where] = (out.read_bytes(), _stats(r.stderr))
        assert got["gpu"][1] == got["host"][1]
        assert got["gpu"][0] == got["host"][0], ext
        hsps, written = int(got["host"][1][4]), int(got["host"][1][5])
        assert 0 < written < hsps  # the cut removed records
    assert written


def test_cli_rejects_a_bad_records_value(tmp_path):
    _fasta(tmp_path / "q.fasta", ["q"], ["ACDEFGHIKLMNPQRSTVWY" * 3])
    _fasta(tmp_path / "d.fasta", ["s"], ["ACDEFGHIKLMNPQRSTVWY" * 5])
    r = subprocess.run([str(_cli()), "searchp", "-q", str(tmp_path / "q.fasta"), "-d", str(tmp_path / "d.fasta"), "-o", str(tmp_path / "o.m8"), "--records", "nonsense"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--records takes gpu, host or auto" in r.stderr, r.stderr
