"""Throughput of lx_gunzip on BGZF input: the device path (host to host and kernel only), the host path (h = NULL), and Python's
zlib decompressing the same members on --threads threads.

The inputs are synthetic FASTQ (150-letter reads, qualities) and protein FASTA (60-letter lines), made here and compressed as BGZF
(raw DEFLATE per 65 280-byte block at zlib level 6 behind the BC header).  Host-to-host = the whole lx_gunzip call, copies in and out
included; kernel = the decoder's device time (lx_last_phase_ms phase 5).

    python tools/gunzip_bench.py --mb 256 --threads 16 > profiles/gunzip_bench.txt
"""
from __future__ import annotations

import argparse
import json
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi  # noqa: E402

BLOCK = 65280


def fastq(n: int) -> bytes:
    rng = np.random.default_rng(1)
    reads = n // 300 + 1  # (records of about 330 bytes)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (reads, 150))]
    qual = (rng.integers(0, 12, (reads, 150)) + ord("5")).astype(np.uint8)
    lines = []
    for k in range(reads):
        lines.append(b"@read%d/1 lane 1\n%s\n+\n%s\n" % (k, seq[k].tobytes(), qual[k].tobytes()))
    return b"".join(lines)[:n]


def protein_fasta(n: int) -> bytes:
    rng = np.random.default_rng(2)
    rows = n // 61 + 1
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)[rng.integers(0, 20, (rows, 60))]
    text = np.concatenate([aa, np.full((rows, 1), ord("\n"), np.uint8)], axis=1)
    for r in range(0, rows, 6):  # a header every six lines
        text[r, :20] = np.frombuffer(b">sp|P%05d| protein " % (r % 100000), np.uint8)[:20]
    return text.tobytes()[:n]


def to_bgzf(data: bytes, threads: int):
    def one(i):
        blk = data[i:i + BLOCK]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        d = c.compress(blk) + c.flush()
        return struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, ord("B"), ord("C"), 2, len(d) + 25) + d + \
            struct.pack("<II", zlib.crc32(blk), len(blk))

    with ThreadPoolExecutor(threads) as ex:
        members = list(ex.map(one, range(0, len(data), BLOCK)))
    return members


def zlib_members(members, threads: int):
    def one(m):
        return len(zlib.decompress(m[18:-8], -15))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        size = sum(ex.map(one, members))
    return size, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    n = a.mb << 20
    with capi.Handle(0) as h:
        for kind, make in (("fastq", fastq), ("protein_fasta", protein_fasta)):
            data = make(n)
            members = to_bgzf(data, a.threads)
            stream = b"".join(members)
            capi.gunzip(h, stream[: sum(len(m) for m in members[:64])])  # (buffers and code objects)
            best, kern = 1e9, 1e9
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = capi.gunzip(h, stream)
                best = min(best, time.perf_counter() - t0)
                kern = min(kern, h.last_phase_ms(5)[0] / 1e3)
            assert out == data
            t0 = time.perf_counter()
            assert capi.gunzip(None, stream) == data
            host = time.perf_counter() - t0
            size, zsec = min((zlib_members(members, a.threads) for _ in range(a.reps)), key=lambda r: r[1])
            assert size == n
            line = {"text": kind, "bytes": n, "bgzf_bytes": len(stream), "members": len(members),
                    "gpu_host_to_host_MBps": round(n / best / 1e6, 1), "gpu_kernel_MBps": round(n / kern / 1e6, 1),
                    "host_path_1t_MBps": round(n / host / 1e6, 1), f"zlib_{a.threads}t_MBps": round(n / zsec / 1e6, 1)}
            line["gpu_vs_zlib"] = round(line["gpu_host_to_host_MBps"] / line[f"zlib_{a.threads}t_MBps"], 2)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
