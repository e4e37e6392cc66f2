"""What tests/test_gpu_limits.py and tests/test_gpu_schemes_edges.py share: the cases and their oracle results (computed once per
session), the device entry points under explicit options, and the comparison of scores, records and ops with the oracle."""
import numpy as np

from lambda_amd import capi
from tests import limit_cases, oracle_lib

_CASES = {}


def cached(name):
    """A case of limit_cases.all_cases(), built once per session: (sc, q, s, ext, target)."""
    if "all" not in _CASES:
        _CASES["all"] = limit_cases.all_cases()
    sc, (q, s, ext, target) = _CASES["all"][name]
    return sc, q, s, ext, target


def oracle_results(oracle, key, sc, q, s, ext, cutoff):
    k = ("want", key, cutoff)
    if k not in _CASES:
        osc = oracle_lib.scoring_from(sc)
        want = oracle.score_batch(q, s, ext, osc, threads=8)
        surv = np.nonzero((want >= cutoff) & (ext["s_len"] > 0) & (ext["q_len"] > 0))[0]
        al = oracle.align_batch(q, s, ext[surv], osc)
        st = []
        for i, (oh, oops) in zip(surv, al):
            x = ext[i]
            qq, ss = q[int(x["q_off"]): int(x["q_off"]) + int(x["q_len"])], s[int(x["s_off"]): int(x["s_off"]) + int(x["s_len"])]
            t = oracle.alignment_stats(qq, ss, oh, oops, osc, 0)
            st.append((oh.score, oh.q_begin, oh.q_end, oh.s_begin, oh.s_end, oh.n_ops, t.num_matches, t.num_mismatches, t.num_positives,
                       t.num_gap_opens, t.num_gap_extensions))
        _CASES[k] = (want, surv, [o for _, o in al], st)
    return _CASES[k]


FIELDS = ("score", "q_begin", "q_end", "s_begin", "s_end", "n_ops", "num_matches", "num_mismatches", "num_positives", "num_gap_opens",
          "num_gap_extensions")


def check_rows(ores, score, hsp, off, ops, tag):
    """Results by caller index (lx_extend_batch, lx_extend_batch_dev): every score, every survivor's record and op bytes."""
    want, surv, want_ops, want_rec = ores
    bad = np.nonzero(score != want)[0]
    assert len(bad) == 0, (tag, bad[:8], score[bad[:8]], want[bad[:8]])
    assert len(surv) > 5
    for i, oops, rec in zip(surv, want_ops, want_rec):
        g = hsp[i]
        assert tuple(int(g[f]) for f in FIELDS) == rec, (tag, i)
        st = int(off[i]) + int(g["ops_shift"])
        assert bytes(ops[st: st + rec[5]]) == oops, (tag, i)


def check_rle_rows(ores, score, hsp, off, codes, tag):
    want, surv, want_ops, want_rec = ores
    assert (score == want).all(), tag
    for i, oops, rec in zip(surv, want_ops, want_rec):
        g = hsp[i]
        assert tuple(int(g[f]) for f in FIELDS) == rec, (tag, i)
        assert capi.Handle.expand_ops(codes[int(off[i]):], rec[5]) == oops, (tag, i)


def check_list(ores, score, index, hsp, off, codes, tag):
    want, surv, want_ops, want_rec = ores
    assert (score == want).all(), tag
    assert len(index) == len(surv) and (np.sort(index) == surv).all(), tag
    pos = {int(i): k for k, i in enumerate(surv)}
    for k, i in enumerate(index):
        rec, oops = want_rec[pos[int(i)]], want_ops[pos[int(i)]]
        assert tuple(int(hsp[k][f]) for f in FIELDS) == rec, (tag, i)
        assert capi.Handle.expand_ops(codes[int(off[k]):], rec[5]) == oops, (tag, i)


def run_dev(handle, q, s, ext, run, cutoff, mode, mq=1):
    """lx_extend_batch_dev with the caller's promises (widest query, longest window, run length) under a pass-2 mode."""
    import torch

    n = len(ext)
    dev = torch.device("cuda:0")
    pad = np.zeros(256, np.uint8)
    d_q = torch.from_numpy(np.concatenate([q, pad])).to(dev)
    d_s = torch.from_numpy(np.concatenate([s, pad])).to(dev)
    d_ext = torch.from_numpy(ext.view(np.uint8).copy()).to(dev)
    sizes = ext["q_len"].astype(np.uint64) + ext["s_len"].astype(np.uint64)
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(sizes)[:-1]
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ops = torch.zeros(int(sizes.sum()) + 16, dtype=torch.uint8, device=dev)
    d_hsp = torch.full((n * 48,), 0xEE, dtype=torch.uint8, device=dev)
    d_score = torch.zeros(n, dtype=torch.int32, device=dev)
    d_count = torch.zeros(2, dtype=torch.int64, device=dev)
    handle.set_option(capi.LX_OPT_MAX_QLEN, int(ext["q_len"].max()))
    handle.set_option(capi.LX_OPT_MAX_SLEN, int(ext["s_len"].max()))
    handle.set_option(capi.LX_OPT_QUERY_RUN, run)
    handle.set_option(capi.LX_OPT_PASS2_MODE, mode)
    handle.set_option(capi.LX_OPT_MQ_SWEEP, mq)
    handle.set_option(capi.LX_OPT_ADAPT_PERMILLE, 0)  # (no adaptive step: the sweep under test runs whatever the last batch's survivors were)
    torch.cuda.synchronize()
    try:
        handle.extend_batch_dev(d_q, d_s, d_ext, n, cutoff, d_score, d_hsp, d_ops, d_off, d_count)
        handle.synchronize()
        name = handle.last_trace_kernel_name()
    finally:
        handle.set_option(capi.LX_OPT_MAX_QLEN, 0)
        handle.set_option(capi.LX_OPT_MAX_SLEN, 0)
        handle.set_option(capi.LX_OPT_QUERY_RUN, 0)
        handle.set_option(capi.LX_OPT_PASS2_MODE, 1)
        handle.set_option(capi.LX_OPT_MQ_SWEEP, 1)
        handle.set_option(capi.LX_OPT_ADAPT_PERMILLE, 30)
    hsp = np.frombuffer(d_hsp.cpu().numpy().tobytes(), dtype=capi.HSP_DTYPE)
    return d_score.cpu().numpy(), hsp, off, d_ops.cpu().numpy(), name


def dev_scores(handle, q, s, ext, run, packed):
    """lx_score_batch_dev with the caller's promises, the packed kernels on or off: (scores, kernel name)."""
    import torch

    dev = torch.device("cuda:0")
    pad = np.zeros(256, np.uint8)
    d_q = torch.from_numpy(np.concatenate([q, pad])).to(dev)
    d_s = torch.from_numpy(np.concatenate([s, pad])).to(dev)
    d_ext = torch.from_numpy(ext.view(np.uint8).copy()).to(dev)
    d_out = torch.full((len(ext),), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    handle.set_option(capi.LX_OPT_MAX_QLEN, int(ext["q_len"].max()))
    handle.set_option(capi.LX_OPT_MAX_SLEN, int(ext["s_len"].max()))
    handle.set_option(capi.LX_OPT_QUERY_RUN, run)
    handle.set_option(capi.LX_OPT_PACKED_HALF, packed)
    try:
        handle.score_batch_dev(d_q, d_s, d_ext, len(ext), d_out)
        handle.synchronize()
        name = handle.last_kernel_name()
    finally:
        handle.set_option(capi.LX_OPT_MAX_QLEN, 0)
        handle.set_option(capi.LX_OPT_MAX_SLEN, 0)
        handle.set_option(capi.LX_OPT_QUERY_RUN, 0)
        handle.set_option(capi.LX_OPT_PACKED_HALF, 1)
    return d_out.cpu().numpy(), name


def pack_runs(ext, run):
    """Slots for LX_OPT_QUERY_RUN = run: every query's windows in blocks of `run`, the last one filled with copies of its last window."""
    order = np.lexsort((ext["s_len"], ext["q_len"], ext["q_off"]))
    out, k = [], 0
    while k < len(order):
        kk = k
        while kk < len(order) and ext["q_off"][order[kk]] == ext["q_off"][order[k]] and ext["q_len"][order[kk]] == ext["q_len"][order[k]]:
            kk += 1
        for j in range(k, kk, run):
            idx = list(order[j: min(kk, j + run)])
            out += idx + [idx[-1]] * (run - len(idx))
        k = kk
    return ext[np.array(out)]
