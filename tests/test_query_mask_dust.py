"""The nucleotide masking rule, symmetric DUST, without a device: the two Python restatements of tests/dust_cases.py against each other
and against the stated cases, the host mask (lx_query_mask_create_dust with h == NULL) against them, the argument errors, info / copy,
the host seeder with a DUST mask against the brute-force seeder, and the host rule under AddressSanitizer and UBSan in a stand-alone
program."""
import ctypes as C
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lambda_amd import build, capi
from tests import dust_cases as DC
from tests import level3_cases as L3
from tests import qmask_cases as QC

ROOT = Path(__file__).resolve().parent.parent
MATRIX = np.ones((capi.LX_ALPH, capi.LX_ALPH), np.int8)
SETTINGS = [(8, 10), (16, 20), (30, 30), (64, 20), (64, 10), (8, 30)]


def _host_equals_restatement(seqs, window=64, level=20, definition=False):
    res, off, ln = DC.as_set(seqs)
    want = DC.dust_mask_set(res, off, ln, window, level)
    if definition:
        assert np.array_equal(want, DC.dust_mask_set(res, off, ln, window, level, definition=True))
    for threads in (1, 3):
        with capi.QueryMask.dust(None, res, off, ln, capi.DustParams(window, level), host_threads=threads) as m:
            got = m.copy()
            assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
            assert m.info() == DC.counts(want, off, ln)
    return want


@pytest.mark.parametrize("name", sorted(DC.named_cases()))
def test_named_cases(lx_lib, name):
    seqs, window, stated = DC.named_cases()[name]
    want = _host_equals_restatement(seqs, window, definition=True)
    first = want[:len(seqs[0])]
    if stated == "all":
        assert first.all()
    elif stated == "none":
        assert not first.any()
    elif stated is not None:
        assert list(np.flatnonzero(first)) == list(range(*stated))
    if name == "empty between":
        assert want[:20].all() and not want[20:50].any() and want[50:].all()
    if name == "two times six A":
        assert not want.any()  # (twelve A in one sequence would be masked: intervals end with their sequence)


def test_the_sweep_equals_the_definition():
    """on seeded sequences with planted repeats and Ns, at several windows and levels; and a reverse complement's mask is the mirror"""
    letters = masked = 0
    for seed in range(25):
        for s in DC.random_reads(seed, 70):
            for window, level in SETTINGS[:4]:
                d = DC.dust_mask_definition(s, window, level)
                assert np.array_equal(d, DC.dust_mask(s, window, level))
                assert np.array_equal(DC.dust_mask(DC.revcomp(s), window, level), d[::-1])
                letters, masked = letters + len(s), masked + int(d.sum())
    assert letters > 10000 and 1000 < masked < letters - 1000


def test_uniform_random_letters_are_almost_never_masked():
    x = DC.random_dna(np.random.default_rng(1), 20000)
    assert DC.dust_mask(x).sum() < 100  # (so every random set below plants repeats)


def test_random_sets(lx_lib):
    masked = free = untouched = 0
    for seed in range(120):
        seqs = DC.random_reads(seed)
        window, level = SETTINGS[seed % len(SETTINGS)]
        want = _host_equals_restatement(seqs, window, level)
        masked, free = masked + int(want.sum()), free + int((want == 0).sum())
        res, off, ln = DC.as_set(seqs)
        untouched += int((ln > 0).sum()) - DC.counts(want, off, ln)[2]
    assert masked > 2000 and free > 2000 and untouched


def test_long_sequences(lx_lib):
    """sequences of a thousand letters and more: a long repeat, repeats behind long random stretches, and stretches cut by an N"""
    rng = np.random.default_rng(8)
    assert _host_equals_restatement([DC.repeat("AC", 3000)]).all()
    for delta in (-1, 0, 1):
        for lead in (1024 - 30, 1024 - 5, 1024 + 2):
            seq = np.concatenate([DC.random_dna(rng, lead + delta), DC.repeat("ACG", 50), DC.random_dna(rng, 40)])
            want = _host_equals_restatement([seq])
            assert want[lead + delta + 2:lead + delta + 48].all() and not want.all()
        seq = np.concatenate([DC.random_dna(rng, 1000), DC.repeat("A", 26 + delta), [4], DC.repeat("A", 30)])
        want = _host_equals_restatement([seq], 16, 20)
        assert want[1001:1026 + delta].all() and not want[1026 + delta] and want[1027 + delta:].all()


def test_argument_errors_info_and_copy(lx_lib):
    seqs, _, _ = DC.named_cases()["empty between"]
    res, off, ln = DC.as_set(seqs)

    def einval(call, text):
        with pytest.raises(capi.LambdaExtError) as e:
            call()
        assert e.value.code == capi.LX_EINVAL and text in str(e.value), str(e.value)

    for bad in [(3, 20), (65, 20), (64, 0), (64, 1001), (-1, 20), (64, -5)]:
        einval(lambda: capi.QueryMask.dust(None, res, off, ln, capi.DustParams(*bad)), "lx_query_mask_create_dust")
    for ok in [(4, 1), (64, 1000)]:
        capi.QueryMask.dust(None, res, off, ln, capi.DustParams(*ok)).close()
    overlap = off.copy()
    overlap[2] -= 1
    einval(lambda: capi.QueryMask.dust(None, res, overlap, ln), "ascending order")
    out, p = C.c_void_p(), capi.DustParams()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lx_lib.lx_query_mask_create_dust(None, None, ptr(off), ptr(ln), len(off), C.byref(p), 0, C.byref(out)) == capi.LX_EINVAL
    assert "NULL" in capi.last_output_error()
    assert lx_lib.lx_query_mask_create_dust(None, ptr(res), None, ptr(ln), len(off), C.byref(p), 0, C.byref(out)) == capi.LX_EINVAL
    assert lx_lib.lx_query_mask_create_dust(None, ptr(res), ptr(off), ptr(ln), len(off), None, 0, C.byref(out)) == capi.LX_EINVAL
    assert lx_lib.lx_query_mask_create_dust(None, ptr(res), ptr(off), ptr(ln), len(off), C.byref(p), 0, None) == capi.LX_EINVAL
    d = capi.DustParams(1, 1)
    lx_lib.lx_dust_params_default(C.byref(d))
    assert (d.window, d.level) == (64, 20) == (p.window, p.level)
    # no sequences, and sequences without letters
    with capi.QueryMask.dust(None, np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64)) as m:
        assert m.info() == (0, 0, 0) and len(m.copy()) == 0
    with capi.QueryMask.dust(None, res, off, ln) as m:
        want = DC.dust_mask_set(res, off, ln)
        assert m.info() == (65, 35, 2) == DC.counts(want, off, ln) and np.array_equal(m.copy(), want)


def test_host_seeding_with_a_dust_mask_equals_brute_force(lx_lib):
    """a nucleotide case whose reads carry an AC repeat shared with subject 0: the host seeder with the DUST mask against the
    restatement of the blocked rule (qmask_cases.seed_starts_masked)"""
    c = nucleotide_case()
    q = (c["s_res"], c["q_res"], c["q_red"], c["q_off"], c["q_len"])
    mask = DC.dust_mask_set(for_the_rule(c["q_res"]), c["q_off"], c["q_len"])
    assert mask.any() and not mask.all()
    p = capi.seed_params(MATRIX, seed_length=14, seed_offset=7, max_seed_dist=0, half_exact=False, adaptive=False, pre_scoring=0, pre_scoring_thresh=0.0,
                         max_matches=1 << 40, q_num_frames=2, unknown_rank=c["unknown"])
    want = L3.sorted_matches(QC.brute_exact_matches_masked(c, mask, 14, 7))
    plain = L3.sorted_matches(L3.brute_exact_matches(c, 14, 7))
    with capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as ix, \
            capi.QueryMask.dust(None, for_the_rule(c["q_res"]), c["q_off"], c["q_len"]) as m:
        assert np.array_equal(m.copy(), mask)
        got = L3.sorted_matches(capi.seed_queries(None, ix, *q, p, mask=m).matches())
    assert np.array_equal(got, want.astype(capi.MATCH_DTYPE)) and 0 < len(want) < len(plain)


def for_the_rule(q_res):
    """level3_cases' nucleotide letters are ranked A, C, G, N, T, as lambda3 searchn's; the rule reads A, C, G, T, N"""
    return np.array([0, 1, 2, 4, 3], np.uint8)[q_res]


def nucleotide_case(n_reads=64, seed=31):
    """level3_cases.make_case('nucleotide') with a 40-letter AC stretch shared by subject 0 and every third read's first frame"""
    c = L3.make_case("nucleotide", n_reads, seed=seed)
    ac = np.resize(np.array([0, 1], np.uint8), 40)
    o = int(c["s_off"][0])
    c["s_res"][o + 10:o + 50] = ac
    c["s_red"][o + 10:o + 50] = L3.DNA4[ac]
    for r in range(0, n_reads, 3):
        if r in (5, 9):
            continue
        o = int(c["q_off"][r * c["frames"]])
        c["q_res"][o + 8:o + 48] = ac
        c["q_red"][o + 8:o + 48] = L3.DNA4[ac]
    return c


def _build_check(tmp_path):
    rocm_include = Path(build._hipcc()).resolve().parent.parent / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        rocm_include = Path("/opt/rocm/include")
    exe = tmp_path / "dust_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           f"-I{rocm_include}", f"-I{ROOT / 'lambda_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "dust_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_host_rule_clean_under_sanitizers(tmp_path):
    """dust_mask_sequence and the score functions it shares with the kernels on exact-size heap blocks: a clean exit under
    AddressSanitizer and UBSan, and the restatement's masks -- the named cases, random sets, and one long sequence"""
    sets = [(seqs, window, 20) for seqs, window, _ in DC.named_cases().values()]
    sets += [(DC.random_reads(seed), *SETTINGS[seed % len(SETTINGS)]) for seed in range(60)]
    rng = np.random.default_rng(9)
    sets += [([np.concatenate([DC.random_dna(rng, 1010), DC.repeat("ACT", 200), [4], DC.repeat("T", 130), DC.random_dna(rng, 3)])], 64, 20)]
    records = []
    for seqs, window, level in sets:
        for s in seqs:
            s = np.asarray(s, np.uint8)
            records.append(struct.pack("<III", window, level, len(s)) + s.tobytes() + DC.dust_mask(s, window, level).tobytes())
    corpus = tmp_path / "corpus.bin"
    corpus.write_bytes(b"LXDM" + struct.pack("<I", len(records)) + b"".join(records))
    r = subprocess.run([str(_build_check(tmp_path)), str(corpus)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f"{len(records)} records, 0 differ" in r.stdout
