"""GPU tests of the taxonomy feature: the device join (lx_taxmap.hip) against the host join on the CPU tests' cases and on a map of
more than 2 M lines, mkindexp --table gpu against --table host, and searchp / searchn on an index with taxonomy -- staxids and the
LCA per query (columns and SAM / BAM tags) against the Python models, --devices 0,0, output without taxonomy columns identical to
that of the index without taxonomy, and the refusal of an LCA on an index without a tree."""
import gzip
import shutil
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests import bam_decode
from tests.test_taxonomy import (edge_join_cases, edge_join_error_cases, fit_chunk, join_error_cases, model_join, model_lca, model_tree,
                                 run_join, same_join, synthetic, taxdump, world)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


@pytest.mark.parametrize("fmt", [capi.LX_TAXMAP_NCBI, capi.LX_TAXMAP_UNIPROT])
@pytest.mark.parametrize("chunk", [1024, 4096, 0])
def test_device_join_equals_host(handle, fmt, chunk):
    ids, text = synthetic(fmt, seed=fmt * 10 + chunk % 7)
    host = run_join(ids, fmt, text, chunk=chunk, piece=4096)
    same_join(host, model_join(ids, fmt, text))
    for piece in (None, 37, 4096):
        same_join(run_join(ids, fmt, text, chunk=chunk, piece=piece, handle=handle), host)
    assert handle.last_phase_ms(6)[1] >= 1  # the join kernels ran
    same_join(run_join(ids, fmt, text[:-1], chunk=chunk, piece=333, handle=handle), run_join(ids, fmt, text[:-1], chunk=chunk))


def test_device_join_errors(handle):
    ids, cases = join_error_cases()
    for name, fmt, text in cases:
        for chunk, piece in ((0, None), (32, 3), (1024, 5)):
            with pytest.raises(capi.LambdaExtError) as eh:
                run_join(ids, fmt, text, chunk=chunk, piece=piece)
            with pytest.raises(capi.LambdaExtError) as ed:
                run_join(ids, fmt, text, chunk=chunk, piece=piece, handle=handle)
            assert str(ed.value) == str(eh.value), name
    text = b"accession\taccession.version\ttaxid\tgi\nQ00001\tx\tnope\t1\nXP_77\tX\t4294967295\t2\nP12345\tP\t007\t3\n"
    same_join(run_join(ids, capi.LX_TAXMAP_NCBI, text, chunk=32, piece=7, handle=handle), model_join(ids, capi.LX_TAXMAP_NCBI, text))


@pytest.mark.parametrize("case", range(12))
def test_device_join_edge_texts(handle, case):
    """tests/test_taxonomy.py's texts around join_parse_kernel's bounds: as one chunk (chunk_bytes = 0, so the text's tiles are the
    chunk's) and in chunks of 8192 bytes, against the host join, which the CPU tests hold against the model."""
    name, fmt, ids, text = edge_join_cases()[case]
    host = run_join(ids, fmt, text, chunk=0)
    same_join(host, model_join(ids, fmt, text))
    same_join(run_join(ids, fmt, text, chunk=0, handle=handle), host)  # (a tile that overflows is an error here: counters->overflow)
    assert handle.last_phase_ms(6)[1] >= 1
    chunk = fit_chunk(8192, text)
    same_join(run_join(ids, fmt, text, chunk=chunk, piece=4096, handle=handle), host)


def test_device_join_first_bad_taxon_in_line_order(handle):
    for name, fmt, ids, text in edge_join_error_cases():
        for chunk, piece in ((0, None), (8192, 4096)):
            with pytest.raises(capi.LambdaExtError) as eh:
                run_join(ids, fmt, text, chunk=chunk, piece=piece)
            with pytest.raises(capi.LambdaExtError) as ed:
                run_join(ids, fmt, text, chunk=chunk, piece=piece, handle=handle)
            assert "first-bad" in str(eh.value) and str(ed.value) == str(eh.value), (name, str(ed.value), str(eh.value))


def big_map(n_lines, n_subjects, seed):
    """an NCBI-style map of n_lines lines over accessions of three letters and five digits, and subjects whose ids carry the
    accession of a random line (a few of them twice, some none)"""
    rng = np.random.default_rng(seed)
    acc_idx = rng.integers(0, 26 ** 3 * 100_000, n_lines)
    lines = np.empty((n_lines, 38), np.uint8)
    for k, d in enumerate((26 ** 2 * 100_000, 26 * 100_000, 100_000)):
        lines[:, k] = ord("A") + (acc_idx // d) % 26
    for k in range(5):
        lines[:, 3 + k] = ord("0") + (acc_idx // 10 ** (4 - k)) % 10
    lines[:, 8] = lines[:, 19] = lines[:, 27] = ord("\t")
    lines[:, 9:17] = lines[:, 0:8]
    lines[:, 17], lines[:, 18] = ord("."), ord("1")
    tax = rng.integers(1, 3_000_000, n_lines)
    for k in range(7):
        lines[:, 20 + k] = ord("0") + (tax // 10 ** (6 - k)) % 10
    gi = np.arange(n_lines)
    for k in range(9):
        lines[:, 28 + k] = ord("0") + (gi // 10 ** (8 - k)) % 10
    lines[:, 37] = ord("\n")
    text = b"accession\taccession.version\ttaxid\tgi\n" + lines.tobytes()
    pick = rng.integers(0, n_lines, n_subjects)
    ids = [b"sp|" + lines[k, 0:8].tobytes() + b"|P_X" + (b" " + lines[(k + 1) % n_lines, 0:8].tobytes() if k % 17 == 0 else b"")
           if k % 13 else b"noacc" for k in pick.tolist()]
    return ids, text


def test_device_join_large(handle):
    ids, text = big_map(2_500_000, 200_000, 5)
    assert len(text) > 90_000_000
    host = run_join(ids, capi.LX_TAXMAP_NCBI, text, chunk=32 << 20, piece=7 << 20)
    dev = run_join(ids, capi.LX_TAXMAP_NCBI, text, chunk=32 << 20, piece=7 << 20, handle=handle)
    same_join(dev, host)
    ms, launches = handle.last_phase_ms(6)
    assert launches >= 3 and ms > 0
    assert host["matched"] > 150_000 and host["lines"] == 2_500_001
    # the default chunk (one chunk) gives the same lists
    same_join(run_join(ids, capi.LX_TAXMAP_NCBI, text, handle=handle), host)


# ---- the front end ------------------------------------------------------------------------------------------------------------
def _run(cwd, *a):
    r = subprocess.run([str(build.build_cli()), *map(str, a)], capture_output=True, text=True, cwd=cwd)
    return r


def _queries(tmp, ids, seqs, nucl):
    with open(tmp / "q.fasta", "w") as f:
        for k in range(0, len(seqs), 3):
            s = seqs[k][5:75]
            f.write(f">q{k}\n{s}\n")


def _expected(tmp, ids, fmt_map, with_tree=True):
    want = model_join(ids, capi.LX_TAXMAP_NCBI, (tmp / fmt_map).read_bytes())
    off, flat = want["s_tax_off"], want["s_tax_ids"]
    lists = [flat[off[s]:off[s + 1]].tolist() for s in range(len(ids))]
    nodes, names = taxdump()
    tree = model_tree(nodes, names, want["present"]) if with_tree else None
    return lists, tree


@pytest.mark.parametrize("cmd", ["searchp", "searchn"])
def test_search_taxonomy_columns(tmp_path, cmd):
    ids, seqs = world(tmp_path, dup=True)
    mk = "mkindexp" if cmd == "searchp" else "mkindexn"
    if cmd == "searchn":
        seqs = ["".join("ACGT"[ord(c) % 4] for c in sq) * 2 for sq in seqs]
        with open(tmp_path / "db.fasta", "w") as f:
            for i, sq in zip(ids, seqs):
                f.write(f">{i}\n{sq}\n")
    _queries(tmp_path, ids, seqs, cmd == "searchn")
    plain_dir, tax_dir = tmp_path / "plain", tmp_path / "tax"
    plain_dir.mkdir()
    tax_dir.mkdir()
    r = _run(tmp_path, mk, "-d", "db.fasta", "-i", plain_dir / "db.lba")
    assert r.returncode == 0, r.stderr
    r = _run(tmp_path, mk, "-d", "db.fasta", "-i", tax_dir / "db.lba", "-m", "m.accession2taxid", "-x", "dump", "--table", "gpu")
    assert r.returncode == 0, r.stderr
    r = _run(tmp_path, mk, "-d", "db.fasta", "-i", tmp_path / "host.lba", "-m", "m.accession2taxid", "-x", "dump", "--table", "host")
    assert r.returncode == 0, r.stderr
    assert (tax_dir / "db.lba").read_bytes() == (tmp_path / "host.lba").read_bytes()
    for d in (plain_dir, tax_dir):
        shutil.copy(tmp_path / "q.fasta", d / "q.fasta")
    lists, tree = _expected(tmp_path, ids, "m.accession2taxid")
    first = {i.split()[0]: s for s, i in enumerate(ids)}

    # tabular: std staxids lcataxid
    for dev in ("0", "0,0"):
        r = _run(tax_dir, cmd, "-q", "q.fasta", "-i", "db.lba", "-o", f"o{dev}.m8", "--output-columns", "std staxids lcataxid", "--devices", dev)
        assert r.returncode == 0, r.stderr
    out = (tax_dir / "o0.m8").read_text()
    assert out == (tax_dir / "o0,0.m8").read_text()
    recs = [l.split("\t") for l in out.splitlines() if l and not l.startswith("#")]
    assert len(recs) >= 10
    by_q = {}
    for f in recs:
        s = first[f[1]]
        assert f[12] == (";".join(map(str, lists[s])) or "*")
        by_q.setdefault(f[0], []).append((s, int(f[13])))
    multi = 0
    for q, hits in by_q.items():
        want = model_lca(tree["parents"], tree["heights"], [lists[s] for s, _ in hits])
        assert all(l == want for _, l in hits), (q, hits, want)
        multi += len({s for s, _ in hits}) > 1
    assert multi >= 3

    # SAM and BAM with st lt ls
    for ext in ("sam", "bam"):
        r = _run(tax_dir, cmd, "-q", "q.fasta", "-i", "db.lba", "-o", f"o.{ext}", "--sam-bam-tags", "AS st lt ls")
        assert r.returncode == 0, r.stderr
    sam = (tax_dir / "o.sam").read_text().splitlines()
    # (the BAM header differs: an @SQ line per subject, its own command line)
    records = lambda lines: [l for l in lines if not l.startswith("@")]
    assert records(bam_decode.to_sam(gzip.decompress((tax_dir / "o.bam").read_bytes()))) == records(sam)
    n = 0
    for line in sam:
        if line.startswith("@"):
            continue
        f = line.split("\t")
        tags = {t[:2]: t[5:] for t in f[11:]}
        s = first[f[2]]
        assert tags["st"] == (";".join(map(str, lists[s])) or "*")
        lt = int(tags["lt"])
        assert lt == by_q[f[0]][0][1]
        assert tags["ls"] == tree["names"][lt]
        n += 1
    assert n >= 10

    # without taxonomy columns the output does not depend on the index's taxonomy
    for d in (plain_dir, tax_dir):
        for o in ("n.m8", "n.sam"):
            r = _run(d, cmd, "-q", "q.fasta", "-i", "db.lba", "-o", o)
            assert r.returncode == 0, r.stderr
    for o in ("n.m8", "n.sam"):
        assert (plain_dir / o).read_bytes() == (tax_dir / o).read_bytes(), o
    # an index without taxonomy: "*" and 0, as before
    r = _run(plain_dir, cmd, "-q", "q.fasta", "-i", "db.lba", "-o", "p.m8", "--output-columns", "std staxids lcataxid")
    assert r.returncode == 0, r.stderr
    assert all(l.split("\t")[12:] == ["*", "0"] for l in (plain_dir / "p.m8").read_text().splitlines() if l)


def test_search_lca_needs_the_tree(tmp_path):
    ids, seqs = world(tmp_path, dup=True)
    _queries(tmp_path, ids, seqs, False)
    r = _run(tmp_path, "mkindexp", "-d", "db.fasta", "-i", "notree.lba", "-m", "m.accession2taxid")
    assert r.returncode == 0, r.stderr
    r = _run(tmp_path, "searchp", "-q", "q.fasta", "-i", "notree.lba", "-o", "o.m8", "--output-columns", "std lcataxid")
    assert r.returncode != 0 and "does not contain a taxonomic tree. Recreate it and provide --tax-dump-dir ." in r.stderr
    # staxids alone needs no tree
    r = _run(tmp_path, "searchp", "-q", "q.fasta", "-i", "notree.lba", "-o", "o.m8", "--output-columns", "std staxids")
    assert r.returncode == 0, r.stderr
    lists, _ = _expected(tmp_path, ids, "m.accession2taxid", with_tree=False)
    first = {i.split()[0]: s for s, i in enumerate(ids)}
    for l in (tmp_path / "o.m8").read_text().splitlines():
        f = l.split("\t")
        assert f[12] == (";".join(map(str, lists[first[f[1]]])) or "*")
