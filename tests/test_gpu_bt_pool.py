"""The checkpoint backtrace's pool of parked extensions (lx_ckpt.hip, LX_BT_POOL): a wavefront keeps up to 32 extensions in
LDS beside its 64 live ones and trades them with lanes that would sit a pass out.  Only the assignment of extensions to
lanes changes, so every record and op string must equal the oracle's whatever the survivor count, the queue's end, the
slot kind or the gaps."""
import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import oracle_lib
from tests.test_oracle import SCHEMES

pytestmark = pytest.mark.gpu


def _exactly(want_score, chosen):
    """per-extension cut-offs that let exactly the chosen extensions through"""
    mins = (want_score + 1).astype(np.int32)
    mins[chosen] = want_score[chosen]
    return mins


def _check(handle, oracle, q, s, ext, mins, rle=False, scheme="blosum62"):
    osc = oracle_lib.scoring_from(SCHEMES[scheme])
    want_score = oracle.score_batch(q, s, ext, osc, threads=8)
    surv = np.nonzero((want_score >= mins) & (want_score > 0) & (ext["s_len"] > 0))[0]
    want = oracle.align_batch(q, s, ext[surv], osc)
    score, hsp, off, ops = handle.extend_batch(q, s, ext, mins)
    assert (score == want_score).all()
    name = handle.last_trace_kernel_name()  # (few survivors: the adaptive mode runs ckpt_forward_kernel; both end in the backtrace)
    assert "single sweep" in name or "ckpt_forward_kernel" in name, name
    for i, (oh, oops) in zip(surv, want):
        g = hsp[i]
        assert (g["score"], g["q_begin"], g["q_end"], g["s_begin"], g["s_end"], g["n_ops"]) == \
               (oh.score, oh.q_begin, oh.q_end, oh.s_begin, oh.s_end, oh.n_ops), i
        st = int(off[i]) + int(g["ops_shift"])
        assert bytes(ops[st: st + oh.n_ops]) == oops, i
    if rle:
        score2, hsp2, off2, codes = handle.extend_batch_rle(q, s, ext, mins)
        assert (score2 == score).all()
        for f in ("score", "q_begin", "q_end", "s_begin", "s_end", "n_ops", "num_matches", "num_gap_opens"):
            assert (hsp2[f] == hsp[f]).all(), f
        for i, (oh, oops) in zip(surv, want):
            c = codes[int(off2[i]): int(off2[i]) + oh.n_ops]
            assert capi.Handle.expand_ops(c, oh.n_ops) == oops, i
    return len(surv)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 96, 97, 700])
def test_pool_survivor_counts(handle, oracle, k):
    """Survivors around one wavefront, one wavefront plus the pool (64 + 32) and several wavefronts' worth: the queue runs
    dry while extensions are parked, and the drain must hand every one of them back to a lane."""
    handle.set_scoring(SCHEMES["blosum62"], 0)
    q, s, ext = synth.make_batch_np(64, 150, 16, seed=7000 + k, sub_rate=0.2, indel_rate=0.04)
    osc = oracle_lib.scoring_from(SCHEMES["blosum62"])
    want_score = oracle.score_batch(q, s, ext, osc, threads=8)
    rng = np.random.default_rng(k)
    chosen = rng.choice(np.nonzero(want_score > 0)[0], k, replace=False)
    assert _check(handle, oracle, q, s, ext, _exactly(want_score, chosen)) == k


def test_pool_empty_windows_and_scoreless_extensions(handle, oracle):
    """Empty windows and extensions without a positive score come out of the queue between real ones (cut-off 0 lets them
    through), in a shuffled list: a lane that takes one ends up empty and must be fed again."""
    handle.set_scoring(SCHEMES["blosum62"], 0)
    q, s, ext = synth.make_batch_np(40, 150, 16, seed=31, sub_rate=0.25, indel_rate=0.05)
    ext = ext.copy()
    rng = np.random.default_rng(31)
    cut = rng.random(len(ext))
    ext["s_len"] = np.where(cut < 0.2, 0, ext["s_len"]).astype(np.uint32)
    ext = ext[rng.permutation(len(ext))]
    mins = np.where(rng.random(len(ext)) < 0.5, 0, 60).astype(np.int32)
    assert _check(handle, oracle, q, s, ext, mins) > 100


@pytest.mark.parametrize("indel_rate", [0.0, 0.08, 0.15])
def test_pool_gap_heavy_windows_and_codes(handle, oracle, indel_rate):
    """From gap-free windows (shortcut passes only) to gap-heavy ones that keep most lanes in tile phases; column bytes and
    run-length codes."""
    handle.set_scoring(SCHEMES["blosum62"], 0)
    q, s, ext = synth.make_batch_np(24, 150, 16, seed=77, sub_rate=0.15, indel_rate=indel_rate)
    assert _check(handle, oracle, q, s, ext, np.full(len(ext), 50, np.int32), rle=True) > 50


@pytest.mark.parametrize("lq", [200, 330, 440, 170])
def test_pool_panels_and_strip_widths(handle, oracle, lq):
    """(8,25) strips (a smaller pool beside the larger tile store), several panels of compact codes, and a narrow last panel."""
    handle.set_scoring(SCHEMES["blosum62"], 0)
    q, s, ext = synth.make_batch_np(8, lq, 24, seed=lq, sub_rate=0.2, indel_rate=0.04)
    assert _check(handle, oracle, q, s, ext, np.full(len(ext), 60, np.int32)) > 20


def test_pool_ambiguous_end_cells(handle, oracle):
    """A two-letter alphabet makes many cells tie for the best score: the tile phases scan the end strip block by block
    (scan mode) while other extensions are parked and traded."""
    handle.set_scoring(SCHEMES["nucl"], 0)
    try:
        rng = np.random.default_rng(5)
        nq, wpq, lq, ls = 48, 8, 120, 150
        q = rng.integers(0, 2, nq * lq).astype(np.uint8)
        s = rng.integers(0, 2, nq * wpq * ls).astype(np.uint8)
        s.reshape(nq * wpq, ls)[::3, 20:20 + 60] = np.tile(q.reshape(nq, lq)[:, 10:70], (wpq, 1)).reshape(nq * wpq, 60)[::3]
        ext = np.zeros(nq * wpq, dtype=capi.EXT_DTYPE)
        ext["q_off"] = np.repeat(np.arange(nq) * lq, wpq)
        ext["q_len"] = lq
        ext["s_off"] = np.arange(nq * wpq) * ls
        ext["s_len"] = ls
        q, s = np.concatenate([q, np.zeros(256, np.uint8)]), np.concatenate([s, np.zeros(256, np.uint8)])
        assert _check(handle, oracle, q, s, ext, np.full(len(ext), 20, np.int32), rle=True, scheme="nucl") > 100
    finally:
        handle.set_scoring(SCHEMES["blosum62"], 0)


def test_pool_overflow_slots(handle, oracle):
    """Tryptophan-rich queries push the best scores beyond what a compact code holds: their wavefronts get int16-pair slots
    in the overflow area, their neighbours compact ones, and parked extensions of both kinds are traded in one wavefront."""
    handle.set_scoring(SCHEMES["blosum62"], 0)
    rng = np.random.default_rng(99)
    wpq, nq, lq = 16, 10, 200
    q, s, ext = synth.make_batch_np(nq, lq, wpq, seed=4711, sub_rate=0.1, indel_rate=0.02)
    q, s = q.copy(), s.copy()
    for k in (1, 4, 5, 8):
        x0 = ext[k * wpq]
        qs = slice(int(x0["q_off"]), int(x0["q_off"]) + lq)
        q[qs] = np.where(rng.random(lq) < 0.97, 22, q[qs])
        for w, x in enumerate(ext[k * wpq: (k + 1) * wpq: 2]):
            ls = int(x["s_len"])
            b = (ls - lq) // 2
            win = s[int(x["s_off"]): int(x["s_off"]) + ls]
            win[b: b + lq] = np.where(rng.random(lq) < (1.0 if w == 0 else 0.9), q[qs], win[b: b + lq])
    assert _check(handle, oracle, q, s, ext, np.full(len(ext), 60, np.int32), rle=True) > 16
