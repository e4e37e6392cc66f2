"""`lambda3 searchp --query-masking seg`: a query that shares only a 30-letter SP repeat with a subject is found without masking and
not with it, an ordinary homolog -- on which the Python restatement of the rule (tests/qmask_cases.py) masks nothing -- keeps its
records byte for byte, and the output file does not depend on where the seeding runs, where the mask is made, or on the query file
being read block by block.  Every process runs alone, under a time limit."""
import subprocess

import numpy as np
import pytest

from lambda_amd import build
from tests import qmask_cases as QC
from tests.test_cli import STD, _fasta

pytestmark = pytest.mark.gpu


def _run(cwd, *args, timeout=120):
    return subprocess.run([str(build.build_cli()), *map(str, args)], capture_output=True, text=True, cwd=cwd, timeout=timeout)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("query_mask_cli")
    rng = np.random.default_rng(12)
    rand = lambda n: "".join(STD[i] for i in rng.integers(0, 20, n))  # noqa: E731
    db = [rand(int(n)) for n in rng.integers(150, 300, 40)]
    db[0] = db[0][:60] + "SP" * 15 + db[0][90:]
    hom = list(db[1][20:120])
    for p in rng.integers(0, 100, 8):
        hom[p] = STD[int(rng.integers(0, 20))]
    queries = {"q_sp": rand(35) + "SP" * 15 + rand(35), "q_hom": "".join(hom)}
    # the restatement: nothing of the homolog is masked, the repeat is
    assert not QC.seg_mask(QC.ranks(queries["q_hom"])).any()
    assert QC.seg_mask(QC.ranks(queries["q_sp"]))[35:65].all()
    _fasta(tmp / "db.fasta", [f"s{j}" for j in range(len(db))], db)
    _fasta(tmp / "q.fasta", list(queries), list(queries.values()))
    return tmp


def _search(world, out, *extra):
    r = _run(world, "searchp", "-q", "q.fasta", "-d", "db.fasta", "-o", out, "--version-to-outputfile", "0", *extra)
    assert r.returncode == 0, r.stderr
    return (world / out).read_text(), r.stderr


def test_masking_drops_the_repeat_and_keeps_the_homolog(world):
    plain, err = _search(world, "none.m8", "--query-masking", "none")
    assert "query masking" not in err
    assert plain == _search(world, "default.m8")[0]  # (none is the default)
    by_query = {q: [ln for ln in plain.splitlines() if ln.split("\t")[0] == q] for q in ("q_sp", "q_hom")}
    assert by_query["q_sp"] and by_query["q_hom"]
    assert any(ln.split("\t")[1] == "s0" for ln in by_query["q_sp"]) and any(ln.split("\t")[1] == "s1" for ln in by_query["q_hom"])
    masked, err = _search(world, "seg.m8", "--query-masking", "seg")
    assert masked.splitlines() == by_query["q_hom"]
    line = [ln for ln in err.splitlines() if ln.startswith("lambda3 query masking: seg 12/2.2/2.5, ")]
    assert len(line) == 1 and " of 200 letters masked, 1 sequence(s) touched, on the GPU, " in line[0], err
    want = int(QC.seg_mask(QC.ranks((world / "q.fasta").read_text().split("\n>")[0].split("\n", 1)[1].replace("\n", ""))).sum())
    assert f", {want} of 200 letters masked" in line[0]


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
    want, _ = _search(world, "seg_ref.m8", "--query-masking", "seg")
    got, err = _search(world, "seg_var.m8", "--query-masking", "seg", *extra)
    assert got == want and want
    assert f"on the {place}, " in [ln for ln in err.splitlines() if ln.startswith("lambda3 query masking")][0]
    # ... and without masking the same variation finds the repeat's query too
    rest = [x for k, x in enumerate(extra) if x != "--masking" and (k == 0 or extra[k - 1] != "--masking")]
    assert "q_sp\t" in _search(world, "none_var.m8", *rest)[0]


def test_other_parameters(world):
    # a window and bounds under which the SP repeat is not low-complexity enough: k2 below one bit
    got, err = _search(world, "strict.m8", "--query-masking", "seg", "--seg-window", "8", "--seg-k1", "0.5", "--seg-k2", "0.9")
    assert "q_sp\t" in got and "seg 8/0.5/0.9, 0 of 200 letters masked, 0 sequence(s) touched" in err
