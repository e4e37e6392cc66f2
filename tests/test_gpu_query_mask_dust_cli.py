"""`lambda3 searchn --query-masking dust`: a read that shares only a 50-letter AC repeat with a subject is found without masking and
not with it, a mutated homolog -- on which the Python restatement of the rule (tests/dust_cases.py) masks nothing -- keeps its records
byte for byte, the report line carries the restatement's counts, and the output file does not depend on where the seeding runs, where
the mask is made, or on the query file being read block by block.  One searchbs run.  Every process runs alone, under a time limit."""
import re
import subprocess

import numpy as np
import pytest

from lambda_amd import build
from tests import dust_cases as DC
from tests.test_cli import _fasta

pytestmark = pytest.mark.gpu


def _run(cwd, *args, timeout=120):
    return subprocess.run([str(build.build_cli()), *map(str, args)], capture_output=True, text=True, cwd=cwd, timeout=timeout)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("query_mask_dust_cli")
    rng = np.random.default_rng(12)
    rand = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))  # noqa: E731
    db = [rand(int(n)) for n in rng.integers(300, 600, 30)]
    db[0] = db[0][:100] + "AC" * 25 + db[0][150:]
    hom = list(db[1][40:140])
    for p in rng.integers(0, 100, 6):
        hom[p] = "ACGT"[int(rng.integers(0, 4))]
    queries = {"q_ac": rand(35) + "AC" * 25 + rand(35), "q_hom": "".join(hom), "q_n": "ACGTTGCA" * 3 + "N" + "A" * 5,
               "q_t": rand(30) + "T" * 9 + "N" + "T" * 12 + rand(30)}
    # the restatement: nothing of the homolog (and of the short read with an N) is masked, the repeat is, and the T runs without their N
    assert not DC.dust_mask(DC.ranks(queries["q_hom"])).any() and not DC.dust_mask(DC.ranks(queries["q_n"])).any()
    assert DC.dust_mask(DC.ranks(queries["q_ac"]))[35:85].all()
    t = DC.dust_mask(DC.ranks(queries["q_t"]))
    assert t[30:39].all() and not t[39] and t[40:52].all()
    _fasta(tmp / "db.fasta", [f"s{j}" for j in range(len(db))], db)
    _fasta(tmp / "q.fasta", list(queries), list(queries.values()))
    return tmp, queries


def _counts(queries, window=64, level=20):
    """(letters, masked letters, touched sequences) of the forward frames; a reverse complement's mask is the mirror"""
    masks = [DC.dust_mask(DC.ranks(q), window, level) for q in queries.values()]
    return sum(map(len, masks)), int(sum(m.sum() for m in masks)), sum(bool(m.any()) for m in masks)


def _report(err, frames_allowed, queries, window=64, level=20):
    line = [ln for ln in err.splitlines() if ln.startswith("lambda3 query masking: ")]
    assert len(line) == 1, err
    m = re.fullmatch(r"lambda3 query masking: dust (\d+)/(\d+), (\d+) of (\d+) letters masked, (\d+) sequence\(s\) touched, on the (GPU|host), [0-9.]+ ms", line[0])
    assert m, line[0]
    letters, masked, touched = _counts(queries, window, level)
    frames = int(m.group(4)) // letters
    assert frames in frames_allowed and (int(m.group(1)), int(m.group(2))) == (window, level)
    assert (int(m.group(4)), int(m.group(3)), int(m.group(5))) == (frames * letters, frames * masked, frames * touched)
    return m.group(6)


def _search(world, out, *extra, cmd="searchn"):
    r = _run(world[0], cmd, "-q", "q.fasta", "-d", "db.fasta", "-o", out, "--version-to-outputfile", "0", *extra)
    assert r.returncode == 0, r.stderr
    return (world[0] / out).read_text(), r.stderr


def test_masking_drops_the_repeat_and_keeps_the_homolog(world):
    plain, err = _search(world, "none.m8", "--query-masking", "none")
    assert "query masking" not in err
    assert plain == _search(world, "default.m8")[0]  # (none is the default)
    by_query = {q: [ln for ln in plain.splitlines() if ln.split("\t")[0] == q] for q in ("q_ac", "q_hom")}
    assert by_query["q_ac"] and by_query["q_hom"]
    assert any(ln.split("\t")[1] == "s0" for ln in by_query["q_ac"]) and any(ln.split("\t")[1] == "s1" for ln in by_query["q_hom"])
    masked, err = _search(world, "dust.m8", "--query-masking", "dust")
    assert masked.splitlines() == [ln for ln in plain.splitlines() if not ln.startswith("q_ac\t")]
    assert _report(err, (2,), world[1]) == "GPU"
    assert _counts(world[1])[2] == 2  # (q_ac and q_t)


@pytest.mark.parametrize("extra,place", [
    (["--seeding", "host"], "host"),
    (["--seeding", "gpu", "--masking", "host"], "host"),
    (["--seeding", "host", "--masking", "gpu"], "GPU"),
    (["--masking", "gpu"], "GPU"),
    (["--query-block", "1"], "GPU"),
    (["--query-block", "1", "--seeding", "host"], "host"),
    (["--search0", "0"], "GPU"),
])
def test_the_output_does_not_depend_on_the_place(world, extra, place):
    want, _ = _search(world, "dust_ref.m8", "--query-masking", "dust")
    got, err = _search(world, "dust_var.m8", "--query-masking", "dust", *extra)
    assert got == want and want
    assert _report(err, (2,), world[1]) == place
    # ... and without masking the same variation finds the repeat's read too
    rest = [x for k, x in enumerate(extra) if x != "--masking" and (k == 0 or extra[k - 1] != "--masking")]
    assert "q_ac\t" in _search(world, "none_var.m8", *rest)[0]


def test_other_parameters(world):
    # a score bound of 30: the AC repeat's intervals reach (l / 2) (l / 2 - 1) / (l - 1), under 16 at l = 62
    got, err = _search(world, "strict.m8", "--query-masking", "dust", "--dust-level", "300")
    assert "q_ac\t" in got and _counts(world[1], 64, 300)[1] == 0
    _report(err, (2,), world[1], 64, 300)
    # a window of 16 letters masks the repeat all the same
    got, err = _search(world, "w16.m8", "--query-masking", "dust", "--dust-window", "16")
    assert "q_ac\t" not in got and "q_hom\t" in got
    _report(err, (2,), world[1], 16, 20)


def test_searchbs_with_dust(world):
    _, err = _search(world, "bs.m8", "--query-masking", "dust", cmd="searchbs")
    _report(err, (2, 4), world[1])
