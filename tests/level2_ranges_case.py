"""Helper of tests/test_gpu_level2_ranges.py (run as a script, its environment -- LX_L2_RANGES, LX_HOST_TIMING -- set by the test): every
list below through lx_iterate_matches_dev and lx_iterate_matches_dev_top (at most 5 records per query), rows, columns and both
statistics structs written as one .npz; argv = out.npz.  Between the calls of a list the window list alone (lx_widen_and_preprocess_dev),
so that the test can see what the range plan had in front of it.  After each list a line "list NAME done" goes to stderr, between the
library's timing lines."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from lambda_amd import capi, synth

LISTS = ("reads", "proteins", "long_query")
DNA = np.array([0, 1, 2, 4], dtype=np.uint8)  # A, C, G, T as the library's nucleotide schemes rank them
LONG_QUERY = 1990                              # the query of "long_query" that holds more than 600 windows
SEED_LEN = 10


def make_list(name):
    """Queries cut from the subjects (substitutions on top), and per query `hits` seed hits: half of them along the query's own diagonal
    -- they merge into one window --, the others anywhere: a window each.  "long_query": one query more, 150 letters that stand 700
    times in the subjects, with a hit on each copy: 700 windows, 700 records for the cut of lx_iterate_matches_dev_top.
    Returns q_res, q_off, q_len, s_res, s_off, s_len, matches."""
    protein = name == "proteins"
    rng = np.random.default_rng({"reads": 5, "proteins": 6, "long_query": 5}[name])
    alphabet = synth.STD20 if protein else DNA
    nq, hits, sub_rate = (1500, 12, 0.25) if protein else (3000, 10, 0.03)
    q_len = rng.integers(50, 401, nq) if protein else rng.integers(140, 161, nq)
    s_len = rng.integers(500, 1501, 300) if protein else np.full(8, 60_000)
    s_off = np.concatenate([[0], np.cumsum(s_len)[:-1]])
    s_res = alphabet[rng.integers(0, len(alphabet), int(s_len.sum()))]
    copies = np.arange(700)
    copy_subj, copy_at = copies % 8, 300 + (copies // 8) * 600  # (600 letters apart on the eight subjects: windows that cannot merge)
    if name == "long_query":
        q_len[LONG_QUERY] = 150
        long_query = alphabet[rng.integers(0, len(alphabet), 150)]
        for sj, at in zip(copy_subj, copy_at):
            s_res[s_off[sj] + at: s_off[sj] + at + 150] = long_query
    q_off = np.concatenate([[0], np.cumsum(q_len)[:-1]])
    q_res = np.empty(int(q_len.sum()), dtype=np.uint8)
    home, pos = rng.integers(0, len(s_len), nq), np.empty(nq, dtype=np.int64)
    for i in range(nq):
        pos[i] = rng.integers(0, s_len[home[i]] - q_len[i] + 1)
        q_res[q_off[i]: q_off[i] + q_len[i]] = s_res[s_off[home[i]] + pos[i]: s_off[home[i]] + pos[i] + q_len[i]]
    if name == "long_query":
        q_res[q_off[LONG_QUERY]: q_off[LONG_QUERY] + 150] = long_query
    sub = rng.random(len(q_res)) < sub_rate
    q_res[sub] = alphabet[rng.integers(0, len(alphabet), int(sub.sum()))]
    own = hits // 2
    m = np.zeros(nq * hits, dtype=capi.MATCH_DTYPE)
    qid = np.repeat(np.arange(nq), hits)
    on_diagonal = np.tile(np.arange(hits) < own, nq)
    m["qryId"] = qid
    m["qryStart"] = (rng.random(nq * hits) * (q_len[qid] - SEED_LEN)).astype(np.int64)
    m["subjId"] = np.where(on_diagonal, home[qid], rng.integers(0, len(s_len), nq * hits))
    anywhere = (rng.random(nq * hits) * (s_len[m["subjId"].astype(np.int64)] - SEED_LEN)).astype(np.int64)
    m["subjStart"] = np.where(on_diagonal, pos[qid] + m["qryStart"].astype(np.int64), anywhere)
    if name == "long_query":
        extra = np.zeros(700, dtype=capi.MATCH_DTYPE)
        extra["qryId"], extra["qryStart"] = LONG_QUERY, 0
        extra["subjId"], extra["subjStart"] = copy_subj, copy_at
        m = np.concatenate([m, extra])
    m["qryEnd"] = m["qryStart"] + SEED_LEN
    m["subjEnd"] = m["subjStart"] + SEED_LEN
    m = m[rng.permutation(len(m))]  # (a seeding kernel's lanes emit them in no particular order)
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    return q_res, u64(q_off), u64(q_len), s_res, u64(s_off), u64(s_len), m


def scheme(name):
    if name == "proteins":
        return capi.builtin_scoring(62, gap_open=-11, gap_extend=-1), capi.karlin_params(62, 0, 0, -11, -1)
    return capi.builtin_scoring(0, match=2, mismatch=-3, gap_open=-5, gap_extend=-2), capi.karlin_params(0, 2, -3, -5, -2)


def flat(bms, ops, stats):
    return {"rows": bms.view(np.uint8).reshape(-1), "ops": np.frombuffer(b"".join(ops), dtype=np.uint8), "stats": np.frombuffer(bytes(stats), dtype=np.uint8)}


if __name__ == "__main__":
    import torch

    out = {}
    for name in LISTS:
        q, qoff, qlen, s, soff, slen, m = make_list(name)
        sc, ka = scheme(name)
        params = capi.SearchParams(1e-2, -1, 0, int(slen.sum()), 0, 1, 1, 0, capi.LX_FRAMES_NONE, capi.LX_FRAMES_NONE, ka)
        with capi.Handle(0) as h:
            h.set_scoring(sc, 0)
            h.set_subjects(s)
            h.set_subject_seqs(soff, slen)
            h.set_queries(q, qoff, qlen, qlen, 1)
            d_m = torch.from_numpy(m.view(np.uint8).copy()).to("cuda:0")
            for k, v in flat(*h.iterate_matches_dev(d_m, len(m), params)).items():
                out[f"{name}.{k}"] = v
            out[f"{name}.kernel"] = np.array(h.last_kernel_name())
            out[f"{name}.window_query"] = h.widen_and_preprocess_dev(d_m, len(m))["qryId"].copy()
            *res, rstats = h.iterate_matches_dev_top(d_m, len(m), params, 5)
            for k, v in flat(*res).items():
                out[f"{name}.top.{k}"] = v
            out[f"{name}.top.record_stats"] = np.frombuffer(bytes(rstats), dtype=np.uint8)
        print(f"list {name} done", file=sys.stderr, flush=True)
    np.savez(sys.argv[1], **out)
