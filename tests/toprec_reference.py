"""The yardstick of the tests of lx_toprec.hip: _writeRecord's sort / unique / sort / cut (src/search_algo.hpp:820-882) restated with
Python's stable `sorted` over tuple keys on the numpy record array -- independent of both the library's host form
(lx_postprocess_records) and its kernels -- and the crafted lists the tests share."""
import numpy as np

from lambda_amd import capi

STAT_FIELDS = ("qrys_with_hit", "hits_duplicate2", "hits_abundant", "hits_final", "pairs")


def write_record(m: np.ndarray, max_matches: int, with_index: bool = False):
    """(kept rows in output order, {statistic: value}[, their positions in `m`]) for rows `m`; every run of equal n_qid is one query."""
    st = dict.fromkeys(STAT_FIELDS, 0)
    n = len(m)
    if n == 0:
        return (m[:0].copy(), st, []) if with_index else (m[:0].copy(), st)
    sid, qs, qe, ss, se = (m[f].tolist() for f in ("n_sid", "q_start", "q_end", "s_start", "s_end"))
    qf, sf = m["q_frame"].astype(np.int16).tolist(), m["s_frame"].astype(np.int16).tolist()  # SIGNED: -3 sorts before +1
    bs = m["bit_score"].tolist()  # the stored doubles
    qid = m["n_qid"]
    cuts = np.flatnonzero(np.concatenate([[True], qid[1:] != qid[:-1], [True]])).tolist()
    key7 = lambda i: (sid[i], qs[i], qe[i], ss[i], se[i], qf[i], sf[i])
    keep = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        st["qrys_with_hit"] += 1  # :826
        order1 = sorted(range(lo, hi), key=lambda i: key7(i) + (-bs[i],))  # :832-853 (stable: ties keep the input order)
        uniq = [i for k, i in enumerate(order1) if k == 0 or key7(i) != key7(order1[k - 1])]  # :856-862
        st["hits_duplicate2"] += len(order1) - len(uniq)
        order2 = sorted(uniq, key=lambda i: -bs[i])  # :865
        if len(order2) > max_matches:  # :867-872
            st["hits_abundant"] += len(order2) - max_matches
            order2 = order2[:max_matches]
        st["hits_final"] += len(order2)
        st["pairs"] += len({sid[i] for i in order2})  # :876-882
        keep += order2
    rows = m[np.asarray(keep, dtype=np.int64)].copy()
    return (rows, st, keep) if with_index else (rows, st)


def stats_dict(st) -> dict:
    return {f: int(getattr(st, f)) for f in STAT_FIELDS}


def crafted_rows(rng, seg_sizes, dup_share=0.3, n_sid=40, wide=False, qids=None):
    """Rows for segments of the given sizes: keys from small ranges (ties in every field), `dup_share` of the rows with the seven-field
    key of another row of their segment, bit scores from a few values (ties), frames -3 .. +3; the fields the step does not read
    carry the row's input position, so that a moved row is recognised.  wide: keys that differ only beyond bit 32."""
    seg_sizes = np.asarray(seg_sizes, dtype=np.int64)
    n = int(seg_sizes.sum())
    m = np.zeros(n, dtype=capi.BLAST_MATCH_DTYPE)
    seg = np.repeat(np.arange(len(seg_sizes)), seg_sizes)
    m["n_qid"] = seg if qids is None else np.repeat(np.asarray(qids), seg_sizes)
    m["qry_id"] = np.arange(n)
    m["subj_id"] = np.arange(n)[::-1]
    hi = (rng.integers(0, 3, n).astype(np.uint64) << np.uint64(40)) if wide else np.zeros(n, np.uint64)
    m["n_sid"] = rng.integers(0, n_sid, n).astype(np.uint64) + hi
    m["q_start"] = rng.integers(0, 4, n)
    m["q_end"] = m["q_start"] + rng.integers(30, 33, n).astype(np.uint64)
    m["s_start"] = rng.integers(0, 3, n).astype(np.uint64) + ((rng.integers(0, 2, n).astype(np.uint64) << np.uint64(33)) if wide else np.uint64(0))
    m["s_end"] = m["s_start"] + rng.integers(30, 32, n).astype(np.uint64)
    m["q_frame"] = rng.integers(-3, 4, n)
    m["s_frame"] = rng.integers(-3, 4, n)
    m["bit_score"] = rng.integers(40, 56, n) / 2.0
    m["e_value"] = rng.random(n)
    m["score"] = np.arange(n) % 1000
    m["n_ops"] = rng.integers(1, 200, n)
    m["ops_off"] = np.arange(n) * 256
    starts = np.concatenate([[0], np.cumsum(seg_sizes)])
    for i in np.flatnonzero(rng.random(n) < dup_share):  # the key of another row of the same segment (bit score: its own, or equal as well)
        lo, hi_ = starts[seg[i]], starts[seg[i] + 1]
        j = int(rng.integers(lo, hi_))
        for f in ("n_sid", "q_start", "q_end", "s_start", "s_end", "q_frame", "s_frame"):
            m[f][i] = m[f][j]
        if rng.random() < 0.4:
            m["bit_score"][i] = m["bit_score"][j]
    return m


# segment sizes around what lx_toprec.hip is laid out for: a wavefront (64), a workgroup's rows (256), a staged tile (512: one more
# row and the large-segment path takes a second turn), several tiles
EDGE_SEGMENTS = [1, 2, 63, 64, 65, 255, 256, 257, 1025, 3000, 511, 512, 513, 767, 768, 769, 1, 1, 3]
