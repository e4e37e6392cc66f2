"""GPU tests of the taxon filter: lx_subject_mask_create_dev against lx_tax_subject_mask word for word; lx_seed_result_filter on device
match lists against the numpy stable filter, record for record, at the scan tile's edges; the front end's --taxon-list /
--taxon-exclude / --taxon-filter against the unfiltered run and the Python model of the rule.

The device lists: a real device seed result (a few thousand matches of a small protein search) whose records are overwritten in
device memory with crafted ones -- record k names subject k, every other field is random --, cut to the wanted length by a first
filter with a prefix mask (itself compared with numpy); so every length and every mask pattern below is reached exactly."""
import ctypes as C
import re

import numpy as np
import pytest

from lambda_amd import capi
from tests import level3_cases as L3
from tests.test_gpu_lca_cli import _run, db  # noqa: F401  (db: the fixture, registered for this module too)
from tests.test_oracle import SCHEMES
from tests.test_taxon_filter import model_mask, random_forest, words_of
from tests.test_taxonomy import model_join, model_tree, taxdump, world

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048  # lx_level2.h: kL2ScanTile


def _hip_runtime():
    """the HIP runtime this process already has (the one the library is bound to), for copies the ABI has no call for"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


# ---- the mask -------------------------------------------------------------------------------------------------------------------------
def same_mask(handle, par, hgt, off, ids, lists_of_taxa):
    n_s = len(off) - 1
    with capi.TaxDev(handle, par, hgt, off, ids) as dev:
        for taxa in lists_of_taxa:
            for exclude in (False, True):
                want, kept, _ = capi.subject_mask(par, hgt, off, ids, taxa, exclude)
                with capi.SubjectMask.from_taxa(handle, dev, taxa, exclude) as m:
                    ms, launches = handle.last_phase_ms(14)
                    assert launches == 1 and ms > 0
                    assert m.info() == (n_s, kept)
                    got = m.words()
                    assert got.tobytes() == want.tobytes(), (taxa, exclude)
                    # the round trip: the words, given back, make the same mask on the device and on the host
                    with capi.SubjectMask.from_words(handle, got, n_s) as again, capi.SubjectMask.from_words(None, got, n_s) as host:
                        assert again.info() == host.info() == (n_s, kept) and again.words().tobytes() == host.words().tobytes() == want.tobytes()


def test_mask_on_the_small_world(handle, tmp_path):
    ids, _ = world(tmp_path)
    join = model_join(ids, capi.LX_TAXMAP_NCBI, (tmp_path / "m.accession2taxid").read_bytes())
    tree = model_tree(*taxdump(), join["present"])
    par, hgt = np.array(tree["parents"], np.uint32), np.array(tree["heights"], np.uint32)
    same_mask(handle, par, hgt, join["s_tax_off"], join["s_tax_ids"], [[2], [4], [7], [1], [3], [5, 5, 12], [999]])
    bits, _ = model_mask(par, hgt, join["s_tax_off"], join["s_tax_ids"], [4], False)
    with capi.TaxDev(handle, par, hgt, join["s_tax_off"], join["s_tax_ids"]) as dev, capi.SubjectMask.from_taxa(handle, dev, [4]) as m:
        assert np.array_equal(capi.mask_bits(m.words(), len(ids)), bits) and 0 < bits.sum() < len(ids)


@pytest.mark.parametrize("n_s", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("n_taxa", [2, 5000])
def test_mask_on_random_forests(handle, n_taxa, n_s):
    rng = np.random.default_rng(n_taxa + n_s)
    par, hgt, off, ids = random_forest(rng, n_taxa, n_s, deep=n_taxa > 70)
    # one subject with 40 taxa, in the middle
    s = n_s // 2
    many = rng.integers(0, n_taxa, 40).astype(np.uint32)
    ids = np.concatenate([ids[:int(off[s])], many, ids[int(off[s + 1]):]])
    off = np.concatenate([off[:s + 1], off[s + 1:] - (off[s + 1] - off[s]) + np.uint64(40)]).astype(np.uint64)
    capi.check_tax_tree(par, hgt, off, ids)
    one = [int(rng.integers(1, n_taxa + 1))]
    many_listed = rng.integers(1, n_taxa + 50, 3000).astype(np.uint32)  # duplicates, and taxa beyond the tree
    same_mask(handle, par, hgt, off, ids, [one, many_listed])


def test_mask_on_a_single_chain_of_depth_300(handle):
    """2 <- 3 <- ... <- 301 under the root: a climb from the deepest taxon takes max height + 1 steps, so the bound is what ends a
    climb that finds nothing, and the listed taxon near the top is found by the deepest taxon only through the whole chain"""
    n_taxa = 302
    par = np.arange(-1, n_taxa - 1).astype(np.int64)
    par[:3] = [0, 1, 1]
    par = par.astype(np.uint32)
    hgt = np.concatenate([[0, 0], np.arange(n_taxa - 2)]).astype(np.uint32)
    n_s = 130
    off = np.arange(n_s + 1, dtype=np.uint64)
    ids = (2 + (np.arange(n_s) * 7) % 300).astype(np.uint32)
    ids[-1] = 301
    capi.check_tax_tree(par, hgt, off, ids)
    assert hgt.max() == 299
    same_mask(handle, par, hgt, off, ids, [[2], [301], [150], [1], [302]])
    with capi.TaxDev(handle, par, hgt, off, ids) as dev, capi.SubjectMask.from_taxa(handle, dev, [2]) as m:
        assert m.info() == (n_s, n_s)


def test_mask_refusals(handle):
    par, hgt = np.array([0, 1, 1], np.uint32), np.zeros(3, np.uint32)
    off, ids = np.array([0, 1], np.uint64), np.array([2], np.uint32)
    other = capi.Handle(0)
    try:
        with capi.TaxDev(handle, par, hgt, off, ids) as dev:
            with pytest.raises(capi.LambdaExtError, match="the tree was made on another handle"):
                capi.SubjectMask.from_taxa(other, dev, [2])
            with pytest.raises(capi.LambdaExtError, match="taxon 0"):
                capi.SubjectMask.from_taxa(handle, dev, [2, 0])
            with pytest.raises(capi.LambdaExtError, match="n == 0"):
                capi.SubjectMask.from_taxa(handle, dev, [])
            with pytest.raises(capi.LambdaExtError, match="NULL argument"):
                capi.SubjectMask.from_taxa(handle, None, [2])
            assert handle.last_phase_ms(14)[1] == 0  # (a refused call reports no launch)
    finally:
        other.close()


# ---- the filter -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeding(handle):
    """seed(): a fresh device seed result of more than three scan tiles of matches"""
    c = L3.make_case("protein", 2200, seed=55, n_subjects=40)
    ix = capi.Index.build(handle, c["s_red"], c["s_off"], c["s_len"], 10)
    p = capi.seed_params(SCHEMES["blosum62"].matrix_np(), seed_length=10, seed_offset=3, max_seed_dist=0, q_num_frames=1, unknown_rank=25, max_matches=256)

    def seed():
        r = capi.seed_queries(handle, ix, c["s_res"], c["q_res"], c["q_red"], c["q_off"], c["q_len"], p)
        assert r.stats.n_matches >= 3 * SCAN_TILE + 5 and r.dev() is not None
        return r

    yield seed
    ix.close()


def download(r):
    n = int(r.stats.n_matches)
    down = np.zeros(max(n, 1), capi.MATCH_DTYPE)
    if n:
        assert _hip_runtime().hipMemcpy(C.c_void_p(down.ctypes.data), C.c_void_p(r.dev().data_ptr()), C.c_size_t(n * 48), 2) == 0  # 2 = device to host
    return down[:n]


def crafted_list(handle, seed, length, frames, rng):
    """a device result whose list is exactly `length` crafted records (record k on subject k, in frame k % frames), and the records"""
    r = seed()
    n = int(r.stats.n_matches)
    assert length <= n
    rec = np.zeros(n, capi.MATCH_DTYPE)
    for f in rec.dtype.names:
        rec[f] = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    rec["subjId"] = np.arange(n, dtype=np.uint64) * frames + np.arange(n, dtype=np.uint64) % frames
    assert _hip_runtime().hipMemcpy(C.c_void_p(r.dev().data_ptr()), C.c_void_p(rec.ctypes.data), C.c_size_t(n * 48), 1) == 0  # 1 = host to device
    with capi.SubjectMask.from_words(handle, words_of(np.arange(n) < length), n) as prefix:
        assert capi.seed_result_filter(r, prefix, frames) == (n, length)
    assert r.stats.n_matches == length and download(r).tobytes() == rec[:length].tobytes()
    return r, rec[:length]


def patterns(length):
    first, last = np.zeros(length, bool), np.zeros(length, bool)
    first[:1], last[-1:] = True, True
    return {"all": np.ones(length, bool), "none": np.zeros(length, bool), "alternating": np.arange(length) % 2 == 0, "first": first, "last": last}


@pytest.mark.parametrize("frames", [1, 2, 6])
def test_filter_equals_the_numpy_stable_filter(handle, seeding, frames):
    rng = np.random.default_rng(frames)
    for length in (0, 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 3 * SCAN_TILE + 5):
        for name, bits in patterns(length).items():
            r, rec = crafted_list(handle, seeding, length, frames, rng)
            st0 = r.stats
            host_copy = r.matches()  # (a host copy made before the filter: dropped by it and made anew)
            assert host_copy.tobytes() == rec.tobytes()
            n_s = length + 3  # (subjects beyond the list's, too)
            with capi.SubjectMask.from_words(handle, words_of(np.concatenate([bits, [True, False, True]])), n_s) as m:
                got = capi.seed_result_filter(r, m, frames)
                ms, launches = handle.last_phase_ms(14)
            want = rec[bits]
            assert got == (length, len(want)), (length, name)
            # (no list: no launch; all kept or none kept: the count alone, nothing to scatter; else the count and the scatter)
            assert launches == (0 if length == 0 else 1 if len(want) in (0, length) else 2) and (ms > 0) == (length > 0), (length, name, launches, ms)
            st = r.stats
            assert st.n_matches == len(want) and r.dev() is not None
            assert download(r).tobytes() == want.tobytes(), (length, name)
            assert r.matches().tobytes() == want.tobytes(), (length, name)
            assert (st.hits_after_seeding, st.hits_failed_pre_extend, st.reads_declined, st.launches_full) == \
                   (st0.hits_after_seeding, st0.hits_failed_pre_extend, st0.reads_declined, st0.launches_full)
            r.close()


def test_filter_refusals_leave_the_list_unchanged(handle, seeding):
    rng = np.random.default_rng(9)
    length = SCAN_TILE + 1
    r, rec = crafted_list(handle, seeding, length, 2, rng)
    other = capi.Handle(0)
    try:
        # the last record's subject lies beyond a mask of length - 1 subjects
        with capi.SubjectMask.from_words(handle, words_of(np.ones(length - 1, bool)), length - 1) as m:
            with pytest.raises(capi.LambdaExtError, match="beyond the mask"):
                capi.seed_result_filter(r, m, 2)
        with capi.SubjectMask.from_words(None, words_of(np.ones(length, bool)), length) as m:
            with pytest.raises(capi.LambdaExtError, match="on the host only"):
                capi.seed_result_filter(r, m, 2)
        with capi.SubjectMask.from_words(other, words_of(np.ones(length, bool)), length) as m:
            with pytest.raises(capi.LambdaExtError, match="another handle"):
                capi.seed_result_filter(r, m, 2)
        with capi.SubjectMask.from_words(handle, words_of(np.ones(length, bool)), length) as m:
            for frames in (0, 7):
                with pytest.raises(capi.LambdaExtError, match=f"{frames} subject frames"):
                    capi.seed_result_filter(r, m, frames)
        assert r.stats.n_matches == length and download(r).tobytes() == rec.tobytes() and r.matches().tobytes() == rec.tobytes()
    finally:
        r.close()
        other.close()


# ---- the front end ----------------------------------------------------------------------------------------------------------------------
BASE = ["--search0", "0", "-n", "256", "--output-columns", "std staxids"]
LINE = re.compile(r"lambda3 taxon filter: (\d+) of (\d+) subjects kept; (\d+) of (\d+) promising seeds dropped; on the (GPU|host) \(")


def search(tmp, out, *extra, ok=True):
    r = _run(tmp, "searchp", "-q", "q.fasta", "-i", "db.lba", "-o", out, *extra)
    assert (r.returncode == 0) == ok, r.stderr
    return ((tmp / out).read_bytes() if ok else b""), r.stderr


def kept_subjects(db, taxa, exclude):
    tmp, ids, lists, tree = db
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    flat = np.array([t for x in lists for t in x], np.uint32)
    bits, known = model_mask(tree["parents"], tree["heights"], off, flat, taxa, exclude)
    return {i.split()[0] for i, b in zip(ids, bits) if b}, known


@pytest.fixture(scope="module")
def unfiltered(db):
    data, err = search(db[0], "all.m8", *BASE)
    assert "lambda3 taxon filter" not in err
    lines = data.decode().splitlines()
    assert len(lines) >= 30
    return lines


def test_front_end_equals_the_unfiltered_run_filtered(db, unfiltered):
    tmp = db[0]
    smaller = 0
    # (taxon 2, Bacteria in the taxdump, is not in this index's tree: the tree skips it as it skips 3, and 4 hangs under the root --
    # so by the rule --taxon-list 2 is refused like --taxon-list 3, and 4 is the list that selects the Bacteria side)
    for option, taxa in (("--taxon-list", [4]), ("--taxon-list", [5, 12]), ("--taxon-exclude", [7]), ("--taxon-exclude", [3])):
        keep, known = kept_subjects(db, taxa, option == "--taxon-exclude")
        data, err = search(tmp, f"f_{option[8:]}_{taxa[0]}.m8", *BASE, option, ",".join(map(str, taxa)))
        want = [line for line in unfiltered if line.split("\t")[1] in keep]
        assert data.decode().splitlines() == want, (option, taxa)
        smaller += 0 < len(want) < len(unfiltered)
        m = LINE.search(err)
        assert m and int(m.group(1)) == len(keep) and int(m.group(2)) == len(db[1]) and int(m.group(3)) <= int(m.group(4)), err
        if len(keep) == len(db[1]):
            assert int(m.group(3)) == 0
        if taxa == [3]:
            assert known.tolist() == [0] and "WARNING: --taxon-exclude taxon 3: the index's tree does not hold it" in err and want == unfiltered
        else:
            assert "WARNING" not in err
    assert smaller >= 3
    for taxon in (2, 3):
        assert kept_subjects(db, [taxon], False)[1].tolist() == [0]
        _, err = search(tmp, "refused.m8", *BASE, "--taxon-list", taxon, ok=False)
        assert f"--taxon-list taxon {taxon}: the index's tree does not hold it" in err and "name a taxon above or below it" in err


@pytest.mark.parametrize("kind", ["m8", "sam", "lazy"])
def test_front_end_gpu_equals_host(db, kind):
    tmp = db[0]
    name, args = {"m8": ("o.m8", BASE), "sam": ("o.sam", ["--search0", "0", "--version-to-outputfile", "0"]),
                  "lazy": ("o.m8", [*BASE, "--lazy-query", "1", "--query-block", "7"])}[kind]

    def body(data):  # (@PG carries the command line)
        return [line for line in data.decode().splitlines() if not line.startswith("@PG")]

    for option, taxa in (("--taxon-list", "5,12"), ("--taxon-exclude", "7")):
        gpu, eg = search(tmp, f"gpu_{kind}_{name}", *args, option, taxa, "--taxon-filter", "gpu")
        host, eh = search(tmp, f"host_{kind}_{name}", *args, option, taxa, "--taxon-filter", "host")
        auto, ea = search(tmp, f"auto_{kind}_{name}", *args, option, taxa)
        assert len(gpu) > 300 and body(gpu) == body(host) == body(auto), (kind, option)
        assert LINE.search(eg).group(5) == "GPU" and LINE.search(eh).group(5) == "host" and LINE.search(ea).group(5) == "GPU"
        assert LINE.search(eg).groups()[:4] == LINE.search(eh).groups()[:4]
        if kind == "lazy":
            plain, _ = search(tmp, f"eager_{name}", *BASE, option, taxa)
            assert plain == gpu


def places(db, tag, *seeding):
    """-n 1 without a list and with --taxon-list 7: (the queries made from a sequence that has a Eukaryota copy, those of them that
    report no Eukaryota subject under the list, those whose one place went to another domain without the list)"""
    tmp, ids, lists, tree = db
    keep, _ = kept_subjects(db, [7], False)
    n_orig = 40
    one = ["--search0", "0", "-n", "1", "--output-columns", "std staxids", *seeding]
    plain = {f[0]: f[1] for f in (line.split("\t") for line in search(tmp, f"one_all_{tag}.m8", *one)[0].decode().splitlines())}
    lines = [line.split("\t") for line in search(tmp, f"one_7_{tag}.m8", *one, "--taxon-list", "7")[0].decode().splitlines()]
    got = {f[0]: f[1] for f in lines}
    assert len(got) == len(lines) and all(s in keep for s in got.values())  # one record per query, none outside the list
    with_copy, missing, freed = [], [], []
    for k in range(0, n_orig, 3):
        k0 = k - k % 2
        family = [ids[s].split()[0] for s in (k0, k0 + 1, n_orig + k0 // 2)]
        if any(name in keep for name in family):
            with_copy.append(k)
            if got.get(f"q{k}") not in keep:
                missing.append(k)
            elif plain.get(f"q{k}") not in keep:
                freed.append(k)
        else:
            assert f"q{k}" not in got
    print(f"-n 1 {' '.join(seeding)}: queries with a Eukaryota copy {with_copy}; without a Eukaryota record under --taxon-list 7 {missing}; "
          f"freed (another domain's subject without the list, a Eukaryota one with it) {freed}")
    return with_copy, missing, freed


def test_the_list_frees_the_places_of_a_query(db):
    """-n 1: without the list a query's one place goes to its best hit; with --taxon-list 7 every query made from a sequence that has
    a Eukaryota copy reports a Eukaryota subject, also where the best hit lies in Bacteria (the fixture's mutated copies lie in the
    other domain).

    Without more, five of the 14 such queries (q0, q12, q18, q24, q36: both originals Bacteria, the copy the only Eukaryota subject)
    would report nothing: at -n 1 the adaptive seeding (src/search_algo.hpp:679-727) elongates a seed until about one occurrence is
    left, which reads past a substitution and loses the copy before the match list exists.  With a list the front end therefore
    lets the seeding aim at -n + the number of dropped subjects (at most 64 per read): this test is what holds it to that."""
    with_copy, missing, freed = places(db, "adaptive")
    assert len(with_copy) >= 8 and not missing, missing
    assert len(freed) >= 3


def test_the_list_frees_the_places_of_a_query_where_the_seeding_finds_the_subject(db):
    """the same with --adaptive-seeding 0, where the seeding does not thin a seed's hits towards -n at all"""
    with_copy, missing, freed = places(db, "plain", "--adaptive-seeding", "0")
    assert len(with_copy) >= 8 and not missing, missing
    assert len(freed) >= 3
