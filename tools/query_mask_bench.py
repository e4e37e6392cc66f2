"""Query masking on the host against the device: lx_query_mask_create_seg with h == NULL on --threads host threads (default 16)
against the same call on a handle, the upload of the letters and of the sequence table included, on seeded sets of --reads reads
(default 10^6 and 10^7) x 6 frames x 50 letters of which about every tenth frame is a repeat of one to three letters.

Both sides are timed as the bare library call: one warm-up, then --runs runs each, alternating.  Printed: every run, the medians, the
kernels' device time (lx_last_phase_ms phase 15), and whether the two masks and their counts agree.

    python tools/query_mask_bench.py > profiles/query_mask_bench.txt

Seeding without a mask against the parent commit (--parent-lib, the parent's liblambda_ext.so, loaded through LX_LIB_PATH): phase 9
of lx_seed_queries (the seeding kernel's device time) on the read set of BASELINE.json configs[2] -- lambda_amd/synth.py's
make_seed_list_np: --seed-reads reads of 150 bp (default 10^6) as two frames against a genome of --mbp Mbp (default 100), searchn's
seeding parameters --, one process per run (a library is loaded once per process), this tree and the parent alternating, --runs runs
each after a warm-up call in the same process.  Both series are printed, with their medians and spreads.

    python tools/query_mask_bench.py --parent-lib PARENT/liblambda_ext.so > profiles/query_mask_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi, synth  # noqa: E402

DNA4 = np.array([0, 1, 2, 0, 3], np.uint8)  # host/lx_seeding.hpp: kDna4 over the ranks A, C, G, N, T


def frames(n_reads: int, seed: int):
    """(q_res, q_off, q_len): n_reads x 6 frames of 50 letters"""
    rng = np.random.default_rng(seed)
    n = n_reads * 6
    res = rng.integers(0, 20, (n, 50), dtype=np.uint8)
    rep = np.flatnonzero(rng.random(n) < 0.1)
    period = rng.integers(1, 4, len(rep))
    unit = rng.integers(0, 20, (len(rep), 3), dtype=np.uint8)
    res[rep] = unit[np.arange(len(rep))[:, None], np.arange(50)[None, :] % period[:, None]]
    ln = np.full(n, 50, np.uint64)
    return res.reshape(-1), (np.arange(n, dtype=np.uint64) * 50), ln


def timed(f):
    t = time.perf_counter()
    out = f()
    return (time.perf_counter() - t) * 1e3, out


def seed_child(npz: str):
    """one process: the index on the device, a warm-up call, one timed call of lx_seed_queries with whatever library LX_LIB_PATH names"""
    d = np.load(npz)
    matrix = np.where(np.eye(capi.LX_ALPH, dtype=bool), 2, -3).astype(np.int8)
    p = capi.seed_params(matrix, seed_length=14, seed_offset=9, max_seed_dist=1, q_num_frames=2, unknown_rank=3, max_matches=25)
    with capi.Handle() as h, capi.Index.build(h, DNA4[d["s_res"]], d["s_off"], d["s_len"], 4) as ix:
        out = []
        for _ in range(2):
            r = capi.seed_queries(h, ix, d["s_res"], d["q_res"], DNA4[d["q_res"]], d["q_off"], d["q_len"], p)
            ms, launches = h.last_phase_ms(9)
            st = r.stats
            out.append({"phase9_ms": ms, "launches": launches, "matches": int(st.n_matches), "declined": int(st.reads_declined)})
            r.close()
    print(json.dumps(out[-1]))


def bench_seeding(a):
    q_res, q_off, q_len, _, s_res, s_off, s_len, _ = synth.make_seed_list_np(a.seed_reads, a.mbp, seed=0x1A3BDA03)
    with tempfile.TemporaryDirectory() as tmp:
        npz = str(Path(tmp) / "reads.npz")
        np.savez(npz, q_res=q_res, q_off=q_off, q_len=q_len, s_res=s_res, s_off=s_off, s_len=s_len)
        series = {"this tree": [], "parent commit": []}
        for run in range(a.runs):
            for name, lib in (("this tree", ""), ("parent commit", a.parent_lib)):
                env = dict(os.environ)
                env.pop("LX_LIB_PATH", None)
                if lib:
                    env["LX_LIB_PATH"] = str(Path(lib).resolve())
                r = subprocess.run([sys.executable, __file__, "--seed-child", npz], capture_output=True, text=True, env=env, timeout=900)
                assert r.returncode == 0, r.stderr[-2000:]
                series[name].append(json.loads(r.stdout.splitlines()[-1]))
    print(f"lx_seed_queries without a mask, {a.seed_reads} reads x 2 frames x 150 bp against {a.mbp} Mbp, phase 9 (the seeding kernel), alternating:")
    for name, runs in series.items():
        ms = [x["phase9_ms"] for x in runs]
        print(f"  {name:13s} ms: " + " ".join(f"{x:.2f}" for x in ms) + f"   median {statistics.median(ms):.2f}, spread {min(ms):.2f} .. {max(ms):.2f}"
              f"   ({runs[0]['matches']} matches, {runs[0]['declined']} reads declined, {runs[0]['launches']} launch(es))")
    assert len({(x["matches"], x["declined"]) for runs in series.values() for x in runs}) == 1, "the two libraries seed differently"
    mine, theirs = [x["phase9_ms"] for x in series["this tree"]], [x["phase9_ms"] for x in series["parent commit"]]
    print(f"  this tree's median / the parent's median: {statistics.median(mine) / statistics.median(theirs):.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="the parent commit's liblambda_ext.so: the yardstick of the seeding comparison")
    ap.add_argument("--seed-reads", type=int, default=10 ** 6)
    ap.add_argument("--mbp", type=float, default=100.0)
    ap.add_argument("--seed-child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--reads", type=int, nargs="*", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    if a.seed_child:
        return seed_child(a.seed_child)
    if a.parent_lib:
        bench_seeding(a)
    with capi.Handle() as h:
        for n_reads in a.reads:
            res, off, ln = frames(n_reads, a.seed)
            host_ms, dev_ms, kernel_ms, same = [], [], [], True
            for run in range(-1, a.runs):
                t_host, mh = timed(lambda: capi.QueryMask.seg(None, res, off, ln, host_threads=a.threads))
                t_dev, md = timed(lambda: capi.QueryMask.seg(h, res, off, ln))
                k = h.last_phase_ms(15)[0]
                if run < 0:
                    same = mh.info() == md.info() and mh.copy().tobytes() == md.copy().tobytes()
                    info = mh.info()
                mh.close(), md.close()
                if run >= 0:
                    host_ms.append(t_host), dev_ms.append(t_dev), kernel_ms.append(k)
            print(f"{n_reads} reads x 6 frames x 50 letters: {info[0]} letters, {info[1]} masked in {info[2]} sequences; host and device agree: {same}")
            print(f"  host, {a.threads} threads  ms: " + " ".join(f"{x:.1f}" for x in host_ms) + f"   median {statistics.median(host_ms):.1f}")
            print("  device, upload in ms: " + " ".join(f"{x:.1f}" for x in dev_ms) + f"   median {statistics.median(dev_ms):.1f}")
            print("  kernels (phase 15) ms: " + " ".join(f"{x:.2f}" for x in kernel_ms) + f"   median {statistics.median(kernel_ms):.2f}", flush=True)


if __name__ == "__main__":
    main()
