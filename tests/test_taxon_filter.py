"""Restricting a search to taxa of the index, the parts that need no device: lx_tax_subject_mask (the rule) against a Python model on
tests/test_taxonomy.py's small world and on random forests; lx_seed_result_filter on host-path seed results against the numpy
stable filter; the refusals of the ABI with their texts; the front end's refusals while it parses --taxon-list / --taxon-exclude /
--taxon-filter and, for a FASTA database, once the database is read."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests import level3_cases as L3
from tests.test_oracle import SCHEMES
from tests.test_taxonomy import model_join, model_tree, taxdump, world


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------
def model_chain(par, t):
    """t, its parent, ... up to the first element whose parent is <= 1; taxon 1 too where that parent is 1"""
    out, c = [t], t
    while par[c] > 1:
        c = int(par[c])
        out.append(c)
    if par[c] == 1:
        out.append(1)
    return out


def model_mask(par, hgt, off, ids, taxa, exclude):
    """(bits per subject, known per listed taxon) by the issue's definitions: chain, under, hit, known"""
    n_taxa, listed = len(par), {int(t) for t in taxa}
    under = [any(x in listed for x in model_chain(par, t)) for t in range(n_taxa)]
    n_s = len(off) - 1
    hit = [any(under[int(t)] for t in ids[int(off[s]):int(off[s + 1])]) for s in range(n_s)]
    bits = np.array([h != bool(exclude) for h in hit], dtype=bool)
    in_subjects, is_parent = {int(t) for t in ids}, {int(p) for p in par}
    known = np.array([int(L < n_taxa and (par[L] != 0 or L in is_parent or L in in_subjects)) for L in map(int, taxa)], dtype=np.uint8)
    return bits, known


def check_against_model(par, hgt, off, ids, taxa, exclude):
    words, kept, known = capi.subject_mask(par, hgt, off, ids, taxa, exclude)
    bits, want_known = model_mask(par, hgt, off, ids, taxa, exclude)
    n_s = len(off) - 1
    assert len(words) == (n_s + 63) // 64
    assert np.array_equal(capi.mask_bits(words, n_s), bits), (taxa, exclude)
    assert kept == int(bits.sum()) == sum(bin(int(w)).count("1") for w in words)  # (the second: no bit at or beyond n_s)
    assert np.array_equal(known, want_known), (taxa, known, want_known)
    return bits, known


@pytest.fixture(scope="module")
def small_world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("taxon_filter_world")
    ids, _ = world(tmp)
    join = model_join(ids, capi.LX_TAXMAP_NCBI, (tmp / "m.accession2taxid").read_bytes())
    tree = model_tree(*taxdump(), join["present"])
    lists = [join["s_tax_ids"][int(join["s_tax_off"][s]):int(join["s_tax_off"][s + 1])].tolist() for s in range(len(ids))]
    return np.array(tree["parents"], np.uint32), np.array(tree["heights"], np.uint32), join["s_tax_off"], join["s_tax_ids"], lists


def test_small_world(small_world):
    par, hgt, off, ids, lists = small_world
    bacteria, eukaryota = {5, 6}, {9, 10, 11, 12}
    assert any(not x for x in lists) and any(set(x) & bacteria for x in lists) and any(set(x) & eukaryota for x in lists)
    # {2}: Bacteria in the taxdump -- but this world's tree skips 2 as it skips 3 (both unassigned with one child: 4 hangs under the
    # root), so by the rule the list is not known and keeps nothing; {4} is the Bacteria side: only it, subjects without taxa are out
    assert par[2] == 0 and par[4] == 1
    bits, known = check_against_model(par, hgt, off, ids, [2], False)
    assert known.tolist() == [0] and not bits.any()
    bits, known = check_against_model(par, hgt, off, ids, [4], False)
    assert known.tolist() == [1] and bits.tolist() == [bool(set(x) & bacteria) for x in lists] and 0 < bits.sum() < len(lists)
    # exclude {7}: everything without a Eukaryota taxon, the subjects without taxa included
    bits, known = check_against_model(par, hgt, off, ids, [7], True)
    assert known.tolist() == [1] and bits.tolist() == [not (set(x) & eukaryota) for x in lists]
    assert all(bits[s] for s, x in enumerate(lists) if not x)
    # {1}: everything that has a connected taxon
    bits, known = check_against_model(par, hgt, off, ids, [1], False)
    assert known.tolist() == [1] and bits.tolist() == [bool(x) for x in lists]
    # {3}: skipped by the tree (unassigned, in-degree 1): not known, nothing kept
    assert par[3] == 0
    bits, known = check_against_model(par, hgt, off, ids, [3], False)
    assert known.tolist() == [0] and not bits.any()
    bits, known = check_against_model(par, hgt, off, ids, [5, 5, 12], False)
    assert known.tolist() == [1, 1, 1] and bits.tolist() == [bool(set(x) & {5, 12}) for x in lists] and bits.any()
    bits, known = check_against_model(par, hgt, off, ids, [999], False)  # >= n_taxa
    assert len(par) < 999 and known.tolist() == [0] and not bits.any()


def random_forest(rng, n_taxa, n_s, deep=False):
    """a tree lx_check_tax_tree admits: taxon 0 unassigned, 1 the root, the others under 0 (disconnected, or further roots), 1 or an
    earlier taxon, labels shuffled; deep: a chain of depth 60 somewhere in it"""
    order = np.concatenate([[0, 1], 2 + rng.permutation(max(n_taxa - 2, 0))]).astype(int)[:n_taxa]  # order[k] = the label of the k-th taxon made
    par = np.zeros(n_taxa, np.uint32)
    if n_taxa > 1:
        par[1] = rng.integers(0, 2)
    for k in range(2, n_taxa):
        r = rng.random()
        if deep and 2 < k <= 62:
            par[order[k]] = order[k - 1]
        elif r < 0.1:
            par[order[k]] = 0
        elif r < 0.3 or k == 2:
            par[order[k]] = 1
        else:
            par[order[k]] = order[int(rng.integers(2, k))]
    hgt = np.zeros(n_taxa, np.uint32)
    for k in range(2, n_taxa):
        t = order[k]
        hgt[t] = 0 if par[t] <= 1 else hgt[par[t]] + 1
    counts = rng.choice([0, 1, 5], n_s)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    ids = rng.integers(0, n_taxa, int(off[-1])).astype(np.uint32)
    return par, hgt, off, ids


def test_random_forests():
    rng = np.random.default_rng(20)
    deepest = 0
    for case in range(300):
        n_taxa = int(rng.integers(2, 301)) if case % 10 else (2, 300, 64)[case // 10 % 3]
        n_s = (1, 63, 64, 65, 200)[case % 5]
        par, hgt, off, ids = random_forest(rng, n_taxa, n_s, deep=n_taxa > 70 and case % 3 == 0)
        capi.check_tax_tree(par, hgt, off, ids)
        deepest = max(deepest, int(hgt.max()))
        taxa = rng.integers(1, n_taxa + 5, int(rng.integers(1, 6))).astype(np.uint32)
        if case % 4 == 0:
            taxa = np.concatenate([taxa, taxa[:1]])  # a duplicate
        check_against_model(par, hgt, off, ids, taxa, exclude=bool(case % 2))
    assert deepest >= 59


# ---- the filter of a host-path result ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_seeding():
    c = L3.make_case("protein", 120, seed=31, n_subjects=30)
    ix = capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"])
    p = capi.seed_params(SCHEMES["blosum62"].matrix_np(), seed_length=10, seed_offset=3, max_seed_dist=1, q_num_frames=1, unknown_rank=25, max_matches=256)

    def seed():
        return capi.seed_queries(None, ix, c["s_res"], c["q_res"], c["q_red"], c["q_off"], c["q_len"], p)

    yield seed, len(c["s_off"])
    ix.close()


def words_of(bits):
    padded = np.zeros((len(bits) + 63) // 64 * 64, np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


@pytest.mark.parametrize("frames", [1, 2])
def test_host_path_filter_equals_the_numpy_stable_filter(host_seeding, frames):
    seed, n_sseq = host_seeding
    n_s = (n_sseq + frames - 1) // frames
    rng = np.random.default_rng(frames)
    for bits in (rng.random(n_s) < 0.5, np.ones(n_s, bool), np.zeros(n_s, bool)):
        r = seed()
        before, st0 = r.matches(), r.stats
        assert len(before) >= 200 and r.dev() is None
        with capi.SubjectMask.from_words(None, words_of(bits), n_s) as m:
            assert m.info() == (n_s, int(bits.sum())) and np.array_equal(capi.mask_bits(m.words(), n_s), bits)
            got = capi.seed_result_filter(r, m, frames)
        want = before[bits[(before["subjId"] // frames).astype(np.int64)]]
        assert got == (len(before), len(want))
        st = r.stats
        assert st.n_matches == len(want) and r.matches().tobytes() == want.tobytes()
        assert (st.hits_after_seeding, st.hits_failed_pre_extend, st.reads_declined, st.launches_full) == \
               (st0.hits_after_seeding, st0.hits_failed_pre_extend, st0.reads_declined, st0.launches_full)
        r.close()


def test_host_path_filter_refuses_a_subject_beyond_the_mask(host_seeding):
    seed, n_sseq = host_seeding
    r = seed()
    before = r.matches()
    short = int(before["subjId"].max())  # a mask of `short` subjects: the largest subject id lies beyond it
    with capi.SubjectMask.from_words(None, words_of(np.zeros(short, bool)), short) as m:
        with pytest.raises(capi.LambdaExtError, match="names subject"):
            capi.seed_result_filter(r, m, 1)
    assert r.stats.n_matches == len(before) and r.matches().tobytes() == before.tobytes()
    r.close()


# ---- refusals of the ABI ------------------------------------------------------------------------------------------------------------
def test_abi_refusals(small_world, host_seeding):
    par, hgt, off, ids, _ = small_world
    lib = capi.load()
    tree, keep = capi._tax_tree(par, hgt, off, ids)
    words, kept = np.zeros(len(off) // 64 + 1, np.uint64), C.c_uint64(0)

    def refused(tree_p, f_p, mask_p, kept_p, text):
        assert lib.lx_tax_subject_mask(tree_p, f_p, mask_p, kept_p, None) == capi.LX_EINVAL
        assert text in capi.last_output_error(), capi.last_output_error()

    f, arr = capi.taxon_filter([2])
    refused(None, C.byref(f), words.ctypes.data, C.byref(kept), "NULL argument")
    refused(C.byref(tree), None, words.ctypes.data, C.byref(kept), "NULL argument")
    refused(C.byref(tree), C.byref(f), None, C.byref(kept), "NULL argument")
    refused(C.byref(tree), C.byref(f), words.ctypes.data, None, "NULL argument")
    f0 = capi.TaxonFilter(arr.ctypes.data, 0, 0, 0)
    refused(C.byref(tree), C.byref(f0), words.ctypes.data, C.byref(kept), "n == 0")
    fz, arrz = capi.taxon_filter([2, 0])
    refused(C.byref(tree), C.byref(fz), words.ctypes.data, C.byref(kept), "taxon 0")
    bad_h = hgt.copy()
    bad_h[5] += 1
    with pytest.raises(capi.LambdaExtError, match="lx_check_tax_tree: the height of taxon 5"):
        capi.subject_mask(par, bad_h, off, ids, [2])
    with pytest.raises(capi.LambdaExtError, match="bit at or beyond"):
        capi.SubjectMask.from_words(None, np.array([1 << 10], np.uint64), 10)
    seed, n_sseq = host_seeding
    r = seed()
    with capi.SubjectMask.from_words(None, words_of(np.ones(n_sseq, bool)), n_sseq) as m:
        for frames in (0, 7):
            with pytest.raises(capi.LambdaExtError, match=f"{frames} subject frames"):
                capi.seed_result_filter(r, m, frames)
        assert lib.lx_seed_result_filter(None, m.m, 1, None, None) == capi.LX_EINVAL and "NULL argument" in capi.last_output_error()
    assert lib.lx_seed_result_filter(r.r, None, 1, None, None) == capi.LX_EINVAL and "NULL argument" in capi.last_output_error()
    r.close()


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def _run(cwd, *a):
    return subprocess.run([str(build.build_cli()), *map(str, a)], capture_output=True, text=True, cwd=cwd)


@pytest.mark.parametrize("extra,text", [
    (["--taxon-list", "2", "--taxon-exclude", "7"], "only one of them"),
    (["--taxon-list", ""], "takes a comma-separated list of taxon ids"),
    (["--taxon-list", "a"], "takes a comma-separated list of taxon ids"),
    (["--taxon-exclude", "5,0"], "takes a comma-separated list of taxon ids"),
    (["--taxon-list", "0"], "takes a comma-separated list of taxon ids"),
    (["--taxon-list", "4294967296"], "takes a comma-separated list of taxon ids"),
    (["--taxon-filter", "gpu"], "give one of them"),
    (["--taxon-list", "2", "--taxon-filter", "x"], "--taxon-filter takes gpu, host or auto"),
])
def test_front_end_refuses_while_parsing(tmp_path, extra, text):
    r = _run(tmp_path, "searchp", "-q", "nowhere.fasta", "-i", "nowhere.lba", "-o", "x.m8", *extra)
    assert r.returncode != 0 and text in r.stderr, r.stderr
    assert "nowhere" not in r.stderr  # (no file was looked for)


def test_front_end_refuses_a_fasta_database(tmp_path):
    ids, seqs = world(tmp_path)
    (tmp_path / "q.fasta").write_text(f">q\n{seqs[0][:60]}\n")
    for option in ("--taxon-list", "--taxon-exclude"):
        r = _run(tmp_path, "searchp", "-q", "q.fasta", "-d", "db.fasta", "-o", "x.m8", option, "2")
        assert r.returncode != 0 and "the index has no taxonomy: build it with mkindex* -m and -x" in r.stderr, r.stderr
