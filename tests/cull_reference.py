"""The yardstick of the tests of --max-hsps / --culling-limit (lx_cull_options): an independent model, stated differently from the
library's rule (lambda_amd/csrc/lx_cull.h counts, for every row, the better rows among ALL rows that are no duplicates).  The model
walks a query's deduplicated rows in output order and keeps lists of SURVIVORS: a row is dropped when max_hsps survivors share its
subject; then, over what that left, a row is dropped when culling_limit survivors envelop it.  That the two say the same is what the
tests check.  The query interval is what the .m8 writer prints as qstart / qend, restated here from its arithmetic."""
import numpy as np

from lambda_amd import capi
from tests import toprec_reference as ref

CULL_FIELDS = ("hits_max_hsps", "hits_culled")


def printed_interval(q_start, q_end, q_frame, q_len, translated):
    """(min, max) of the 1-based qstart / qend of the .m8 writer."""
    if translated:
        shift = abs(q_frame) - 1
        lo, hi = 3 * q_start + shift, 3 * q_end + shift
        qs, qe = (lo + 1, hi) if q_frame >= 0 else (q_len - lo, q_len - hi + 1)
    elif q_frame < 0:
        qs, qe = q_len - q_end + 1, q_len - q_start
    else:
        qs, qe = q_start + 1, q_end
    return min(qs, qe), max(qs, qe)


def write_record(m, max_matches, max_hsps=0, culling_limit=0, q_lens=None, translated=False):
    """(kept rows in output order, {statistic: value} with both new counters) for rows `m`; every run of equal n_qid is one query."""
    st = dict.fromkeys(ref.STAT_FIELDS + CULL_FIELDS, 0)
    n = len(m)
    if n == 0:
        return m[:0].copy(), st
    sid, qs, qe, ss, se = (m[f].tolist() for f in ("n_sid", "q_start", "q_end", "s_start", "s_end"))
    qf, sf = m["q_frame"].astype(np.int16).tolist(), m["s_frame"].astype(np.int16).tolist()
    bs = m["bit_score"].tolist()
    qid = m["n_qid"].tolist()
    cuts = np.flatnonzero(np.concatenate([[True], m["n_qid"][1:] != m["n_qid"][:-1], [True]])).tolist()
    key7 = lambda i: (sid[i], qs[i], qe[i], ss[i], se[i], qf[i], sf[i])
    keep = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        st["qrys_with_hit"] += 1
        order1 = sorted(range(lo, hi), key=lambda i: key7(i) + (-bs[i],))
        uniq = [i for k, i in enumerate(order1) if k == 0 or key7(i) != key7(order1[k - 1])]
        st["hits_duplicate2"] += len(order1) - len(uniq)
        rows = sorted(uniq, key=lambda i: -bs[i])  # output order
        if max_hsps:
            survivors, per_subject = [], {}
            for i in rows:
                if per_subject.get(sid[i], 0) >= max_hsps:
                    st["hits_max_hsps"] += 1
                else:
                    per_subject[sid[i]] = per_subject.get(sid[i], 0) + 1
                    survivors.append(i)
            rows = survivors
        if culling_limit:
            survivors, boxes = [], []  # boxes: the intervals of the survivors
            for i in rows:
                a, b = printed_interval(qs[i], qe[i], qf[i], int(q_lens[qid[i]]), translated)
                around = 0
                for x, y in boxes:
                    if x <= a and b <= y:
                        around += 1
                        if around >= culling_limit:
                            break
                if around >= culling_limit:
                    st["hits_culled"] += 1
                else:
                    survivors.append(i)
                    boxes.append((a, b))
            rows = survivors
        if len(rows) > max_matches:
            st["hits_abundant"] += len(rows) - max_matches
            rows = rows[:max_matches]
        st["hits_final"] += len(rows)
        st["pairs"] += len({sid[i] for i in rows})
        keep += rows
    return m[np.asarray(keep, dtype=np.int64)].copy(), st


def stats_dict(st, cst) -> dict:
    return {**ref.stats_dict(st), **{f: int(getattr(cst, f)) for f in CULL_FIELDS}}


MODES = {  # name: (frames, translated)
    "none": ((0,), False),
    "revcomp": ((1, -1), False),
    "translated": ((1, 2, 3, -1, -2, -3), True),
    "bisulfite": ((1, 2, -1, -2), False),
}


def nested_rows(rng, seg_sizes, mode, n_sid=4, q_len_range=(301, 3000)):
    """Rows for segments of the given sizes and the queries' lengths (one query per segment): few subjects, few bit scores (ties),
    frames of `mode`, and query ranges drawn so that nesting chains, equal intervals and partial overlaps all occur: a row's range is
    a fresh one, a range inside another row's of its segment (chains grow by repetition), or another row's own."""
    frames, translated = MODES[mode]
    seg_sizes = np.asarray(seg_sizes, dtype=np.int64)
    n, nq = int(seg_sizes.sum()), len(seg_sizes)
    q_lens = rng.integers(q_len_range[0], q_len_range[1], nq).astype(np.uint64)
    if translated:
        q_lens += (q_lens % 3 == 0).astype(np.uint64)  # lengths not divisible by 3
    m = np.zeros(n, dtype=capi.BLAST_MATCH_DTYPE)
    seg = np.repeat(np.arange(nq), seg_sizes)
    starts = np.concatenate([[0], np.cumsum(seg_sizes)])
    m["n_qid"] = seg
    m["qry_id"] = np.arange(n)
    m["subj_id"] = np.arange(n)[::-1]
    m["n_sid"] = rng.integers(0, n_sid, n)
    m["s_start"] = rng.integers(0, 50, n)
    m["s_end"] = m["s_start"] + rng.integers(30, 60, n).astype(np.uint64)
    m["q_frame"] = np.asarray(frames)[rng.integers(0, len(frames), n)]
    m["s_frame"] = 0
    m["bit_score"] = rng.integers(40, 46, n) / 2.0
    m["e_value"] = rng.random(n)
    m["n_ops"] = rng.integers(1, 200, n)
    m["ops_off"] = np.arange(n) * 256
    kind = rng.random(n)
    for i in range(n):
        ql, f = int(q_lens[seg[i]]), int(m["q_frame"][i])
        room = (ql - (abs(f) - 1)) // 3 if translated else ql  # the largest q_end of this frame
        j = int(rng.integers(starts[seg[i]], i)) if i > starts[seg[i]] else -1
        if j >= 0 and kind[i] < 0.2 and int(m["q_end"][j]) <= room:  # another row's own range (an equal interval when the frames agree)
            a, e = int(m["q_start"][j]), int(m["q_end"][j])
        elif j >= 0 and kind[i] < 0.6 and int(m["q_end"][j]) <= room and int(m["q_end"][j]) - int(m["q_start"][j]) >= 3:  # inside another row's
            a0, e0 = int(m["q_start"][j]), int(m["q_end"][j])
            a = int(rng.integers(a0, a0 + (e0 - a0) // 3 + 1))
            e = int(rng.integers(e0 - (e0 - a0) // 3, e0 + 1))
            m["q_frame"][i] = m["q_frame"][j]
        else:  # a fresh one
            a = int(rng.integers(0, room - 1))
            e = int(rng.integers(a + 1, room + 1))
        m["q_start"][i], m["q_end"][i] = a, e
    return m, q_lens, translated
