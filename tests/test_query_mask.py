"""The query masking rule without a device: lx_seg_tables against the stated constants and Python's formula, the host mask
(lx_query_mask_create_seg with h == NULL) against the Python restatement of tests/qmask_cases.py, the argument errors, seeding with
hand-made masks against a brute-force seeder, and the host rule under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import struct
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from lambda_amd import build, capi
from tests import level3_cases as L3
from tests import qmask_cases as QC

ROOT = Path(__file__).resolve().parent.parent
MATRIX = np.ones((capi.LX_ALPH, capi.LX_ALPH), np.int8)
T_2_TO_12 = [131072, 311616, 524288, 760849, 1016449, 1287880, 1572864, 1869698, 2177059, 2493890, 2819329]


def _exact(**kw):
    base = dict(seed_length=10, seed_offset=5, max_seed_dist=0, half_exact=False, adaptive=False, pre_scoring=0, pre_scoring_thresh=0.0,
                max_matches=1 << 40, q_num_frames=1, unknown_rank=25)
    base.update(kw)
    return capi.seed_params(MATRIX, **base)


def _host_equals_restatement(seqs, **seg):
    res, off, ln = QC.as_set(seqs)
    want = QC.seg_mask_set(res, off, ln, **seg)
    p = capi.SegParams(seg.get("W", 12), seg.get("k1", 2.2), seg.get("k2", 2.5))
    for threads in (1, 3):
        with capi.QueryMask.seg(None, res, off, ln, p, host_threads=threads) as m:
            assert np.array_equal(m.copy(), want)
            assert m.info() == QC.counts(want, off, ln)
    return want


def test_tables(lx_lib):
    T, thr1, thr2 = capi.seg_tables()
    assert list(T[:2]) == [0, 0] and list(T[2:13]) == T_2_TO_12 and (thr1, thr2) == (1089179, 853250)
    for W, k1, k2 in [(4, 1.0, 2.0), (12, 2.2, 2.5), (64, 3.3, 6.0), (12, 2.2, 2.2)]:
        T, thr1, thr2 = capi.seg_tables(capi.SegParams(W, k1, k2))
        wT, w1, w2 = QC.seg_tables(W, k1, k2)
        assert list(map(int, T)) == wT and (thr1, thr2) == (w1, w2)


@pytest.mark.parametrize("name", sorted(QC.named_cases()))
def test_named_cases(lx_lib, name):
    want = _host_equals_restatement(QC.named_cases()[name])
    if name in ("ASASASASASAS", "length W", "length W + 1"):
        assert want.all()
    if name in ("eleven A", "length W - 1", "two times six A", "weak alone"):
        assert not want.any()


def test_weak_windows_join_their_trigger(lx_lib):
    """the cases are what their names say: windows that only reach thr2 in front of (behind) the stretch's trigger, in one run"""
    T, thr1, thr2 = QC.seg_tables()
    for name, weak_first in (("weak before trigger", True), ("weak behind trigger", False)):
        seq = QC.named_cases()[name][0]
        S = [sum(T[n] for n in Counter(map(int, seq[p:p + 12])).values()) for p in range(len(seq) - 11)]
        run = [p for p in range(len(S)) if S[p] >= thr2]
        assert run == list(range(run[0], run[-1] + 1))  # one run
        trig = [p for p in run if S[p] >= thr1]
        only2 = [p for p in run if S[p] < thr1]
        assert len(only2) >= 10 and trig
        assert (sum(p < trig[0] for p in only2) >= 10) if weak_first else (sum(p > trig[-1] for p in only2) >= 10)
        mask = QC.seg_mask(seq)
        assert mask[run[0]:run[-1] + 12].all() and mask.sum() == run[-1] + 12 - run[0]


def test_every_composition_of_twelve(lx_lib):
    wins = QC.composition_windows(12)
    T, thr1, thr2 = QC.seg_tables()
    S = [sum(T[n] for n in Counter(map(int, w)).values()) for w in wins]
    assert (len(wins), sum(s >= thr1 for s in S), sum(s >= thr2 for s in S)) == (77, 46, 58)
    want = _host_equals_restatement(wins)
    assert [bool(want[12 * k]) for k in range(77)] == [s >= thr1 for s in S]  # a single window is masked exactly when it triggers


def test_other_window_with_equal_thresholds(lx_lib):
    rng = np.random.default_rng(5)
    seqs = [np.concatenate([QC.random_protein(rng, 30), QC.repeat("QA", 25), QC.random_protein(rng, 9)]), QC.repeat("GGS", 100), QC.random_protein(rng, 6)]
    want = _host_equals_restatement(seqs, W=7, k1=1.6, k2=1.6)
    assert want.any() and not want.all()
    want = _host_equals_restatement(seqs + QC.random_frames(3), W=64, k1=3.0, k2=3.4)
    assert want.any()


def test_random_sets(lx_lib):
    masked = 0
    for seed in range(300):
        masked += int(_host_equals_restatement(QC.random_frames(seed)).sum())
    assert masked > 1000


def test_argument_errors(lx_lib):
    res, off, ln = QC.as_set(QC.named_cases()["empty between"])

    def einval(call, text):
        with pytest.raises(capi.LambdaExtError) as e:
            call()
        assert e.value.code == capi.LX_EINVAL and text in str(e.value), str(e.value)

    for bad in [(3, 1.0, 1.5), (65, 2.2, 2.5), (12, 0.0, 2.5), (12, 2.6, 2.5), (12, 2.2, 3.6), (12, float("nan"), 2.5)]:
        einval(lambda: capi.seg_tables(capi.SegParams(*bad)), "lx_seg_tables")
        einval(lambda: capi.QueryMask.seg(None, res, off, ln, capi.SegParams(*bad)), "lx_query_mask_create_seg")
    overlap = off.copy()
    overlap[2] -= 1
    einval(lambda: capi.QueryMask.seg(None, res, overlap, ln), "ascending order")
    einval(lambda: capi.QueryMask.from_bytes(None, np.zeros(len(res), np.uint8), overlap, ln), "ascending order")
    out, p = C.c_void_p(), capi.SegParams()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lx_lib.lx_query_mask_create_seg(None, None, ptr(off), ptr(ln), len(off), C.byref(p), 0, C.byref(out)) == capi.LX_EINVAL
    assert "NULL" in capi.last_output_error()
    assert lx_lib.lx_query_mask_create_seg(None, ptr(res), None, ptr(ln), len(off), C.byref(p), 0, C.byref(out)) == capi.LX_EINVAL
    assert lx_lib.lx_query_mask_create_seg(None, ptr(res), ptr(off), ptr(ln), len(off), None, 0, C.byref(out)) == capi.LX_EINVAL
    assert lx_lib.lx_query_mask_create_seg(None, ptr(res), ptr(off), ptr(ln), len(off), C.byref(p), 0, None) == capi.LX_EINVAL
    assert lx_lib.lx_query_mask_create(None, None, ptr(off), ptr(ln), len(off), C.byref(out)) == capi.LX_EINVAL
    assert lx_lib.lx_query_mask_info(None, None, None, None) == capi.LX_EINVAL and lx_lib.lx_query_mask_copy(None, None) == capi.LX_EINVAL
    assert lx_lib.lx_seg_tables(None, None, None, None) == capi.LX_EINVAL
    lx_lib.lx_query_mask_destroy(None)
    # a mask of another sequence table
    c = L3.make_case("protein", 8, seed=2)
    q = (c["s_res"], c["q_res"], c["q_red"], c["q_off"], c["q_len"])
    with capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as ix:
        shorter = c["q_len"].copy()
        shorter[3] -= 1
        for o, n in ((c["q_off"][:-1], c["q_len"][:-1]), (c["q_off"], shorter)):
            with capi.QueryMask.from_bytes(None, np.zeros(len(c["q_res"]), np.uint8), o, n) as m:
                einval(lambda: capi.seed_queries(None, ix, *q, _exact(), mask=m), "another sequence table")


def test_without_a_mask_nothing_changes(lx_lib):
    c = L3.make_case("translated", 40, seed=8)
    q = (c["s_res"], c["q_res"], c["q_red"], c["q_off"], c["q_len"])
    with capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as ix:
        scored = np.where(np.eye(capi.LX_ALPH, dtype=bool), 5, -2).astype(np.int8)  # (the default mode pre-scores its hits)
        for p in (_exact(q_num_frames=6), capi.seed_params(scored, q_num_frames=6, max_seed_dist=1)):
            a = capi.seed_queries(None, ix, *q, p).matches()
            b = capi.seed_queries(None, ix, *q, p, mask=None).matches()
            with capi.QueryMask.from_bytes(None, np.zeros(len(c["q_res"]), np.uint8), c["q_off"], c["q_len"]) as none:
                z = capi.seed_queries(None, ix, *q, p, mask=none).matches()
            assert len(a) > 50 and a.tobytes() == b.tobytes() == z.tobytes()


def _hand_masks(c, seed_length):
    """name -> 0 / 1 bytes over the case's queries"""
    n, rng = len(c["q_res"]), np.random.default_rng(4)
    ends = (c["q_off"] + c["q_len"]).astype(int)
    last, all_starts, skipped, sparse = (np.zeros(n, np.uint8) for _ in range(4))
    for o, e in zip(c["q_off"].astype(int), ends):
        if e - o >= seed_length:
            last[e - 1] = 1                         # blocks exactly the last start, L - seed_length
            all_starts[o + seed_length - 1:e:seed_length] = 1  # every window of seed_length letters holds one
            skipped[o:o + 3] = 1                    # the starts 0 .. 2 are passed over onto 3
    sparse[rng.random(n) < 0.03] = 1
    return {"none": np.zeros(n, np.uint8), "last start": last, "every start": all_starts, "skipped onto a free one": skipped, "sparse": sparse,
            "last and skipped": last | skipped}


@pytest.mark.parametrize("mode,seed_length,seed_offset", [("protein", 10, 5), ("protein", 7, 3), ("translated", 10, 5)])
def test_masked_exact_seeding_equals_brute_force(lx_lib, mode, seed_length, seed_offset):
    c = L3.make_case(mode, 70, seed=21)
    q = (c["s_res"], c["q_res"], c["q_red"], c["q_off"], c["q_len"])
    p = _exact(seed_length=seed_length, seed_offset=seed_offset, q_num_frames=c["frames"], unknown_rank=c["unknown"])
    unmasked = L3.sorted_matches(L3.brute_exact_matches(c, seed_length, seed_offset))
    with capi.Index.build(None, c["s_red"], c["s_off"], c["s_len"], c["alph"]) as ix:
        for name, bytes_ in _hand_masks(c, seed_length).items():
            want = L3.sorted_matches(QC.brute_exact_matches_masked(c, bytes_, seed_length, seed_offset))
            with capi.QueryMask.from_bytes(None, bytes_, c["q_off"], c["q_len"]) as m:
                assert np.array_equal(m.copy(), bytes_[:len(m.copy())]), name
                got = L3.sorted_matches(capi.seed_queries(None, ix, *q, p, mask=m).matches())
            assert np.array_equal(got, want.astype(capi.MATCH_DTYPE)), name
            if name == "none":
                assert np.array_equal(want, unmasked) and len(want) >= 100
            elif name == "every start":
                assert len(want) == 0
            else:
                assert 0 < len(want) < len(unmasked), name
            for r in got:  # no seed's first seed_length letters hold a masked letter
                o = int(c["q_off"][r["qryId"]]) + int(r["qryStart"])
                assert not bytes_[o:o + seed_length].any()


def _build_check(tmp_path):
    rocm_include = Path(build._hipcc()).resolve().parent.parent / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        rocm_include = Path("/opt/rocm/include")
    exe = tmp_path / "qmask_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           f"-I{rocm_include}", f"-I{ROOT / 'lambda_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "qmask_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_host_rule_clean_under_sanitizers(tmp_path):
    """seg_mask_sequence and the word functions it shares with the kernels on exact-size heap blocks: a clean exit under
    AddressSanitizer and UBSan, and the restatement's masks"""
    records = []
    sets = [(s, dict()) for s in QC.named_cases().values()] + [(QC.random_frames(seed), dict()) for seed in range(60)]
    sets += [(QC.random_frames(seed), dict(W=W, k1=k1, k2=k2)) for seed in range(60, 80) for W, k1, k2 in ((4, 1.0, 1.5), (7, 1.6, 1.6), (64, 3.0, 3.4))]
    rng = np.random.default_rng(9)
    sets += [([np.concatenate([QC.random_protein(rng, 70), QC.repeat("SPA", 200), QC.random_protein(rng, 3), QC.repeat("K", 130)])], dict())]
    for seqs, seg in sets:
        T, thr1, thr2 = QC.seg_tables(**seg)
        for s in seqs:
            records.append(struct.pack("<III", seg.get("W", 12), thr1, thr2) + np.array(T, "<u4").tobytes() + struct.pack("<I", len(s)) +
                           np.asarray(s, np.uint8).tobytes() + QC.seg_mask(s, **seg).tobytes())
    corpus = tmp_path / "corpus.bin"
    corpus.write_bytes(b"LXQM" + struct.pack("<I", len(records)) + b"".join(records))
    r = subprocess.run([str(_build_check(tmp_path)), str(corpus)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f"{len(records)} records, 0 differ" in r.stdout
