"""GPU tests of the front end's --lca gpu|host|auto and --lca-top-percent P: the output of --lca gpu byte-identical to that of --lca
host for .m8, .sam and the block pipeline at P = 100, 10 and 0; P = 100 the file of a run without either option; at P = 0 every
query's lcataxid against the model over the hits with the query's largest score; the refusals while the options are parsed."""
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests.test_taxonomy import model_join, model_lca, model_tree, taxdump, world

pytestmark = pytest.mark.gpu

COLUMNS = "std score staxids lcataxid"
KINDS = {"m8": ("o.m8", ["--output-columns", COLUMNS]),
         # (a .sam file names its command line in @PG, and the command lines differ by the very options under test: left out)
         "sam": ("o.sam", ["--sam-bam-tags", "AS st lt ls", "--version-to-outputfile", "0"]),
         "lazy": ("o.m8", ["--output-columns", COLUMNS, "--lazy-query", "1", "--query-block", "7"])}
STD = "ACDEFGHIKLMNPQRSTVWY"


def _run(cwd, *a):
    return subprocess.run([str(build.build_cli()), *map(str, a)], capture_output=True, text=True, cwd=cwd)


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    """tests/test_taxonomy.py's world(dup=True) and, for every distinct sequence, a copy with six substitutions whose taxon lies in
    the other domain: a query made from the sequence hits the originals with its best score and the copy with a weaker one, so that
    the LCA over all hits is the root and the LCA over the best hits is not"""
    tmp = tmp_path_factory.mktemp("lca_cli")
    ids, seqs = world(tmp, dup=True)
    base = model_join(ids, capi.LX_TAXMAP_NCBI, (tmp / "m.accession2taxid").read_bytes())
    off, flat = base["s_tax_off"], base["s_tax_ids"]
    map_lines = []
    for k in range(0, len(seqs), 2):
        taxa = set(flat[off[k]:off[k + 2]].tolist())
        s = list(seqs[k])
        for p in (13, 14, 15, 16, 65, 66):
            s[p] = STD[(STD.index(s[p]) + 7) % 20]
        acc = f"Q9{k:02d}A1"
        ids.append(f"sp|{acc}|COPY{k}_X mutated copy of {k}")
        seqs.append("".join(s))
        map_lines.append(f"{acc}\t{acc}.1\t{12 if taxa & {5, 6} else 5}\t{3000 + k}")
    with open(tmp / "db.fasta", "w") as f:
        for i, sq in zip(ids, seqs):
            f.write(f">{i}\n{sq}\n")
    with open(tmp / "m.accession2taxid", "a") as f:
        f.write("\n".join(map_lines) + "\n")
    with open(tmp / "q.fasta", "w") as f:
        for k in range(0, 40, 3):
            f.write(f">q{k}\n{seqs[k][5:75]}\n")
    r = _run(tmp, "mkindexp", "-d", "db.fasta", "-i", "db.lba", "-m", "m.accession2taxid", "-x", "dump")
    assert r.returncode == 0, r.stderr
    want = model_join(ids, capi.LX_TAXMAP_NCBI, (tmp / "m.accession2taxid").read_bytes())
    lists = [want["s_tax_ids"][want["s_tax_off"][s]:want["s_tax_off"][s + 1]].tolist() for s in range(len(ids))]
    nodes, names = taxdump()
    return tmp, ids, lists, model_tree(nodes, names, want["present"])


def search(tmp, kind, out, *extra):
    name, args = KINDS[kind]
    r = _run(tmp, "searchp", "-q", "q.fasta", "-i", "db.lba", "-o", out + name[1:], *args, *extra)
    assert r.returncode == 0, r.stderr
    return (tmp / (out + name[1:])).read_bytes(), r.stderr


@pytest.mark.parametrize("kind", list(KINDS))
def test_gpu_equals_host(db, kind):
    tmp = db[0]
    plain, err = search(tmp, kind, f"plain_{kind}")
    assert "lambda3 LCA:" not in err
    for top in (100, 10, 0):
        host, eh = search(tmp, kind, f"host_{kind}_{top}", "--lca", "host", "--lca-top-percent", top)
        gpu, eg = search(tmp, kind, f"gpu_{kind}_{top}", "--lca", "gpu", "--lca-top-percent", top)
        assert len(host) > 1000 and host == gpu, (kind, top)
        assert "folded on the host" in eh and "folded on the GPU" in eg
        if top == 100:
            assert host == plain


def test_top_percent_0_against_model(db):
    tmp, ids, lists, tree = db
    first = {i.split()[0]: s for s, i in enumerate(ids)}

    def by_query(data):
        out = {}
        for line in data.decode().splitlines():
            f = line.split("\t")
            assert f[13] == (";".join(map(str, lists[first[f[1]]])) or "*")
            out.setdefault(f[0], []).append((first[f[1]], int(f[12]), int(f[14])))
        return out

    best = by_query(search(tmp, "m8", "model_0", "--lca", "gpu", "--lca-top-percent", 0)[0])
    full = by_query(search(tmp, "m8", "model_100", "--lca", "gpu")[0])
    assert len(best) >= 10 and best.keys() == full.keys()
    differ = 0
    for q, hits in best.items():
        top = max(score for _, score, _ in hits)
        want0 = model_lca(tree["parents"], tree["heights"], [lists[s] for s, score, _ in hits if score == top])
        want100 = model_lca(tree["parents"], tree["heights"], [lists[s] for s, _, _ in hits])
        assert all(l == want0 for _, _, l in hits), (q, hits, want0)
        assert all(l == want100 for _, _, l in full[q]), (q, full[q], want100)
        differ += want0 != want100
    assert differ >= 3


def test_options_refused_while_parsing(db):
    tmp = db[0]
    r = _run(tmp, "searchp", "-q", "nowhere.fasta", "-i", "nowhere.lba", "-o", "x.m8", "--lca-top-percent", "101")
    assert r.returncode != 0 and "Value 101.000000 of option --lca-top-percent is not in range [0.000000,100.000000]." in r.stderr
    r = _run(tmp, "searchp", "-q", "nowhere.fasta", "-i", "nowhere.lba", "-o", "x.m8", "--lca", "x")
    assert r.returncode != 0 and "--lca takes gpu, host or auto" in r.stderr
