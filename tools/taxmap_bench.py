"""Throughput of the accession-to-taxon join (lx_taxmap_*): the device path (host to host, and the join kernels' device time) and the
host path on --threads threads, over the same seeded synthetic NCBI-style map.

The map has --lines lines of the form "ABC12345\tABC12345.1\t0009606\t000000001" (38 bytes; random accessions of three letters and five
digits, random taxa); the database has --subjects ids "sp|ACC|P_X" that carry the accession of a random line (every 13th id none,
every 17th one a second).  Host to host = feeding the map from host memory in 64 MiB pieces and lx_taxmap_finish (the per-subject
lists in host memory); the table is built before the clock starts and its time is reported apart.  Kernel = lx_last_phase_ms phase 6.

    python tools/taxmap_bench.py --lines 64000000 --subjects 4000000 --threads 16 > profiles/taxmap_bench.txt
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi  # noqa: E402

PIECE = 64 << 20


def synthetic(n_lines: int, n_subjects: int, seed: int):
    rng = np.random.default_rng(seed)
    acc_idx = rng.integers(0, 26 ** 3 * 100_000, n_lines)
    lines = np.empty((n_lines, 38), np.uint8)
    for k, d in enumerate((26 ** 2 * 100_000, 26 * 100_000, 100_000)):
        lines[:, k] = ord("A") + (acc_idx // d) % 26
    for k in range(5):
        lines[:, 3 + k] = ord("0") + (acc_idx // 10 ** (4 - k)) % 10
    del acc_idx
    lines[:, 8] = lines[:, 19] = lines[:, 27] = ord("\t")
    lines[:, 9:17] = lines[:, 0:8]
    lines[:, 17], lines[:, 18] = ord("."), ord("1")
    tax = rng.integers(1, 3_000_000, n_lines)
    for k in range(7):
        lines[:, 20 + k] = ord("0") + (tax // 10 ** (6 - k)) % 10
    del tax
    for k in range(9):
        lines[:, 28 + k] = ord("0") + (np.arange(n_lines) // 10 ** (8 - k)) % 10
    lines[:, 37] = ord("\n")
    pick = rng.integers(0, n_lines, n_subjects)
    ids = [b"sp|" + lines[k, 0:8].tobytes() + b"|P_X" + (b" " + lines[(k + 1) % n_lines, 0:8].tobytes() if k % 17 == 0 else b"")
           if k % 13 else b"noacc" for k in pick.tolist()]
    text = b"accession\taccession.version\ttaxid\tgi\n" + lines.tobytes()
    return ids, text


def run(handle, ids, text, threads):
    t0 = time.perf_counter()
    tm = capi.TaxMap(handle, capi.LX_TAXMAP_NCBI, ids, threads=threads)
    t1 = time.perf_counter()
    mv = memoryview(text)
    for a in range(0, len(text), PIECE):
        tm.feed(mv[a:a + PIECE])
    res = tm.finish()
    t2 = time.perf_counter()
    tm.close()
    return res, t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=64_000_000)
    ap.add_argument("--subjects", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    ids, text = synthetic(a.lines, a.subjects, a.seed)
    gb = len(text) / 1e9
    host, host_table_s, host_s = run(None, ids, text, a.threads)
    with capi.Handle(0) as h:
        run(h, ids, text[: 1 << 20], 0)  # (warm-up: device buffers, the kernels' first launch)
        dev, dev_table_s, dev_s = run(h, ids, text, 0)
        kernel_ms, launches = h.last_phase_ms(6)
    same = all(np.array_equal(dev[k], host[k]) for k in ("s_tax_off", "s_tax_ids", "present")) and all(
        dev[k] == host[k] for k in ("no_acc", "multi_acc", "no_tax", "multi_tax", "lines", "matched"))
    print(json.dumps({
        "lines": a.lines, "subjects": a.subjects, "map_bytes": len(text), "matched": host["matched"], "same_result": bool(same),
        "gpu_host_to_host_GBps": round(gb / dev_s, 3), "gpu_kernel_ms": round(kernel_ms, 1), "gpu_kernel_launch_groups": launches,
        "gpu_kernel_GBps": round(gb / (kernel_ms / 1e3), 2) if kernel_ms else None,
        "gpu_kernel_share": round(kernel_ms / 1e3 / dev_s, 3),
        f"host_{a.threads}t_GBps": round(gb / host_s, 3), "gpu_vs_host": round(host_s / dev_s, 2),
        "table_build_s": round(host_table_s, 2), "gpu_table_build_and_upload_s": round(dev_table_s, 2)}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
