"""The taxon filter on the host against the device: the subject mask (lx_tax_subject_mask against lx_subject_mask_create_dev over a
resident tree, the mask's download included) and the filter of a match list (lx_seed_result_filter on a host-path result against the
same call on a device result).

The tree is tools/lca_bench.py's seeded synthetic one (2.5 M taxa on 40 levels) with --subjects subjects (default 10^6 and 10^8); the
list of taxa is one clade of level 6 per --clades (default 20), which keeps a few percent of the subjects.  The match lists come from
one synthetic protein search seeded on either side -- --copies identical copies of each subject make a read's seeds hit several
subjects, and the reads are counted out from a pilot so that the list has about --matches matches (default 10^7) --; their records are
then overwritten (record k names subject k) so that a mask of the wanted density keeps exactly 1 %, 50 % or 99 % of them, scattered.
Every filter run needs a fresh list, so the overwrite is repeated outside the timed call.

Both sides are timed as the bare library call: one warm-up, then --runs runs each, alternating.  Printed: every run, the medians, the
kernels' device time (lx_last_phase_ms phase 14).

    python tools/taxon_filter_bench.py > profiles/taxon_filter_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi, synth  # noqa: E402
from tools.lca_bench import synthetic_tree  # noqa: E402

def hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def timed(f):
    t = time.perf_counter()
    out = f()
    return (time.perf_counter() - t) * 1e3, out


def bench_mask(h, a, n_subjects):
    par, hgt, off, ids = synthetic_tree(a.taxa, n_subjects, a.seed)
    capi.check_tax_tree(par, hgt, off, ids)
    level6 = np.flatnonzero(hgt == 6)
    taxa = level6[np.random.default_rng(a.seed).integers(0, len(level6), a.clades)].astype(np.uint32)
    host_ms, dev_ms, kernel_ms = [], [], []
    with capi.TaxDev(h, par, hgt, off, ids) as tax:
        for run in range(-1, a.runs):
            t_host, (want, kept, _) = timed(lambda: capi.subject_mask(par, hgt, off, ids, taxa))
            t_dev, m = timed(lambda: capi.SubjectMask.from_taxa(h, tax, taxa))
            k = h.last_phase_ms(14)[0]
            same = m.words().tobytes() == want.tobytes() and m.info() == (n_subjects, kept)
            m.close()
            if run >= 0:
                host_ms.append(t_host), dev_ms.append(t_dev), kernel_ms.append(k)
                print(f"mask subjects {n_subjects} run {run}: host {t_host:9.2f} ms, device {t_dev:9.2f} ms (kernels {k:7.3f} ms), kept {kept}, same words: {same}", flush=True)
            if not same:
                raise SystemExit("the device's mask differs from the host's")
    print(f"mask subjects {n_subjects}: host median {statistics.median(host_ms):.2f} ms, device median {statistics.median(dev_ms):.2f} ms "
          f"(kernels median {statistics.median(kernel_ms):.3f} ms), host / device {statistics.median(host_ms) / statistics.median(dev_ms):.2f}", flush=True)


def search_case(n_reads, n_distinct, copies, seed):
    """n_distinct random proteins of 96 letters, each `copies` times; reads: exact pieces of 64 letters"""
    rng = np.random.default_rng(seed)
    distinct = synth.STD20[rng.integers(0, 20, (n_distinct, 96))].astype(np.uint8)
    subjects = np.repeat(distinct, copies, axis=0)
    s_len = np.full(len(subjects), 96, np.uint64)
    s_off = (np.arange(len(subjects)) * 96).astype(np.uint64)
    which, at = rng.integers(0, n_distinct, n_reads), rng.integers(0, 32, n_reads)
    reads = distinct[which[:, None], at[:, None] + np.arange(64)[None, :]]
    q_len = np.full(n_reads, 64, np.uint64)
    q_off = (np.arange(n_reads) * 64).astype(np.uint64)
    return subjects.reshape(-1), s_off, s_len, reads.reshape(-1), q_off, q_len


def bench_filter(h, a):
    from tests.level3_cases import LI10 as li10
    from tests.test_oracle import SCHEMES

    p = capi.seed_params(SCHEMES["blosum62"].matrix_np(), seed_length=10, seed_offset=5, max_seed_dist=0, q_num_frames=1, unknown_rank=25, max_matches=1 << 20)
    n_distinct = 4096

    def seed_both(n_reads):
        s, s_off, s_len, q, q_off, q_len = search_case(n_reads, n_distinct, a.copies, a.seed)
        with capi.Index.build(h, li10[s], s_off, s_len, 10) as ix:
            d = capi.seed_queries(h, ix, s, q, li10[q], q_off, q_len, p)
            r = capi.seed_queries(None, ix, s, q, li10[q], q_off, q_len, p)
        return d, r

    d, r = seed_both(2000)
    per_read = max(1.0, d.stats.n_matches / 2000)
    d.close(), r.close()
    d, r = seed_both(int(a.matches / per_read) + 1)
    n = int(d.stats.n_matches)
    assert n == r.stats.n_matches
    print(f"filter: {n} matches ({per_read:.1f} per read; reads the device declined: {d.stats.reads_declined})", flush=True)
    rng = np.random.default_rng(a.seed)
    rec = np.zeros(n, capi.MATCH_DTYPE)
    for f in rec.dtype.names:
        rec[f] = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    rec["subjId"] = np.arange(n, dtype=np.uint64)
    hip, lib = hip_runtime(), capi.load()
    # (a filter shortens its list for good: every run works on a list seeded anew and overwritten; the lists are released between runs)
    d.close(), r.close()
    for percent in (1, 50, 99):
        bits = rng.random(n) < percent / 100
        words = np.packbits(np.concatenate([bits, np.zeros(-n % 64, bool)]), bitorder="little").view("<u8").astype(np.uint64)
        want = rec[bits]
        host_ms, dev_ms, kernel_ms = [], [], []
        for run in range(-1, a.runs):
            d, r = seed_both(int(a.matches / per_read) + 1)
            assert d.stats.n_matches == r.stats.n_matches == n
            assert hip.hipMemcpy(C.c_void_p(d.dev().data_ptr()), C.c_void_p(rec.ctypes.data), C.c_size_t(n * 48), 1) == 0
            C.memmove(lib.lx_seed_result_matches(r.r), rec.ctypes.data, n * 48)
            with capi.SubjectMask.from_words(h, words, n) as m:
                t_host, _ = timed(lambda: capi.seed_result_filter(r, m, 1))
                t_dev, got = timed(lambda: capi.seed_result_filter(d, m, 1))
                k = h.last_phase_ms(14)[0]
            same = got == (n, len(want)) and d.matches().tobytes() == want.tobytes() == r.matches().tobytes()
            d.close(), r.close()
            if run >= 0:
                host_ms.append(t_host), dev_ms.append(t_dev), kernel_ms.append(k)
                print(f"filter keep {percent} % run {run}: host {t_host:9.2f} ms, device {t_dev:9.2f} ms (kernels {k:7.3f} ms), same list: {same}", flush=True)
            if not same:
                raise SystemExit("the device's list differs from the host's")
        print(f"filter {n} matches keep {percent} %: host median {statistics.median(host_ms):.2f} ms, device median {statistics.median(dev_ms):.2f} ms "
              f"(kernels median {statistics.median(kernel_ms):.3f} ms), host / device {statistics.median(host_ms) / statistics.median(dev_ms):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, nargs="*", default=[1_000_000, 100_000_000])
    ap.add_argument("--matches", type=int, default=10_000_000)
    ap.add_argument("--taxa", type=int, default=2_500_000)
    ap.add_argument("--clades", type=int, default=20)
    ap.add_argument("--copies", type=int, default=4)  # (about 44 matches per read: below the 64 a device launch has room for)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    with capi.Handle(0) as h:
        for n_subjects in a.subjects:
            bench_mask(h, a, n_subjects)
        if a.matches:
            bench_filter(h, a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
