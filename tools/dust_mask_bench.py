"""The nucleotide query masking (symmetric DUST) on the host against the device: lx_query_mask_create_dust with h == NULL on --threads
host threads (default 16) against the same call on a handle, the upload of the letters and of the sequence table included, on seeded
sets of --reads reads (default 10^6 and 10^7) x 2 frames (a read and its reverse complement) x 150 letters.  One read in ten carries a
microsatellite of 20 to 60 letters, a repeat of a unit of 1 to 6 letters.

Both sides are timed as the bare library call: one warm-up, then --runs runs each, alternating.  Printed: every run, the medians, the
kernels' device time (lx_last_phase_ms phase 15), and whether the two masks and their counts agree.

    python tools/dust_mask_bench.py > profiles/dust_mask_bench.txt
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi  # noqa: E402

LETTERS = 150


def frames(n_reads: int, seed: int):
    """(q_res, q_off, q_len): n_reads x 2 frames of 150 letters, ranks A, C, G, T = 0 .. 3"""
    rng = np.random.default_rng(seed)
    res = np.empty((n_reads, 2, LETTERS), np.uint8)
    for lo in range(0, n_reads, 1 << 20):  # (in pieces: the index arrays below are eight bytes per letter)
        n = min(n_reads, lo + (1 << 20)) - lo
        fwd = rng.integers(0, 4, (n, LETTERS), dtype=np.uint8)
        rep = np.flatnonzero(rng.random(n) < 0.1)
        length, period = rng.integers(20, 61, len(rep)), rng.integers(1, 7, len(rep))
        start = (rng.random(len(rep)) * (LETTERS - length + 1)).astype(np.int64)
        unit = rng.integers(0, 4, (len(rep), 6), dtype=np.uint8)
        col = np.arange(LETTERS)[None, :]
        inside = (col >= start[:, None]) & (col < (start + length)[:, None])
        fwd[rep] = np.where(inside, unit[np.arange(len(rep))[:, None], (col - start[:, None]) % period[:, None]], fwd[rep])
        res[lo:lo + n, 0] = fwd
        res[lo:lo + n, 1] = 3 - fwd[:, ::-1]
    n = n_reads * 2
    return res.reshape(-1), (np.arange(n, dtype=np.uint64) * LETTERS), np.full(n, LETTERS, np.uint64)


def timed(f):
    t = time.perf_counter()
    out = f()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="*", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--level", type=int, default=20)
    a = ap.parse_args()
    p = capi.DustParams(a.window, a.level)
    with capi.Handle() as h:
        for n_reads in a.reads:
            try:
                res, off, ln = frames(n_reads, a.seed)
            except MemoryError:
                print(f"{n_reads} reads: not enough host memory for the set, left out", flush=True)
                continue
            host_ms, dev_ms, kernel_ms, same, info = [], [], [], True, None
            for run in range(-1, a.runs):
                t_host, mh = timed(lambda: capi.QueryMask.dust(None, res, off, ln, p, host_threads=a.threads))
                t_dev, md = timed(lambda: capi.QueryMask.dust(h, res, off, ln, p))
                k = h.last_phase_ms(15)[0]
                if run < 0:
                    same = mh.info() == md.info() and mh.copy().tobytes() == md.copy().tobytes()
                    info = mh.info()
                mh.close(), md.close()
                if run >= 0:
                    host_ms.append(t_host), dev_ms.append(t_dev), kernel_ms.append(k)
                print(f"{n_reads} reads, run {run}: host {t_host:.0f} ms, device {t_dev:.0f} ms", file=sys.stderr, flush=True)
            print(f"{n_reads} reads x 2 frames x {LETTERS} letters, dust {a.window}/{a.level}: {info[0]} letters, {info[1]} masked in {info[2]} sequences; "
                  f"host and device agree: {same}")
            print(f"  host, {a.threads} threads  ms: " + " ".join(f"{x:.1f}" for x in host_ms) + f"   median {statistics.median(host_ms):.1f}")
            print("  device, upload in ms: " + " ".join(f"{x:.1f}" for x in dev_ms) + f"   median {statistics.median(dev_ms):.1f}")
            print("  kernels (phase 15) ms: " + " ".join(f"{x:.2f}" for x in kernel_ms) + f"   median {statistics.median(kernel_ms):.2f}", flush=True)


if __name__ == "__main__":
    main()
