"""Throughput of lx_gunzip_stream over one plain gzip member: the stream of this tree, which decodes the member on the device wave
by wave, against the same loop through the parent commit's library (--parent-lib, loaded through LX_LIB_PATH), whose stream
inflates every plain member on the calling thread.

The input is seeded synthetic FASTQ (150-letter reads, qualities) of --mb MiB, compressed at each of --levels into one member the
way pigz does it: blocks of 16 MiB compressed on --threads threads, each closed by a full flush, one CRC32 and ISIZE behind the
last.  Every run is a child process that opens the file, takes every piece (--piece bytes; the default is the front end's
QueryStream::kPiece); the first pass over the file checks the CRC32 of the text and is not counted.  Every run and the median are
printed, with the kernel phases (find, decode, chain + resolve), the counts and the bytes moved up and down of a pass.  No
threshold is set here: the file is where the number goes.

    python tools/gunzip_stream_bench.py --parent-lib /path/to/parent/liblambda_ext.so --out profiles/gunzip_stream_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BLOCK = 16 << 20
COUNTS = ("plain_parallel", "plain_host", "declined", "chunks", "chunks_dropped", "waves", "bytes_up", "bytes_down")


def fastq(n: int, seed: int = 1) -> bytes:
    """Records of one width, made column by column: '@read<9 digits>/1 lane 1', 150 letters, '+', 150 qualities."""
    rng = np.random.default_rng(seed)
    head = b"@read000000000/1 lane 1\n"
    width = len(head) + 150 + 3 + 150 + 1
    reads = n // width + 1
    rec = np.empty((reads, width), np.uint8)
    rec[:, :len(head)] = np.frombuffer(head, np.uint8)
    ids = np.arange(reads, dtype=np.int64)
    for d in range(9):
        rec[:, 5 + 8 - d] = 48 + (ids // 10 ** d) % 10
    at = len(head)
    rec[:, at:at + 150] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (reads, 150), dtype=np.uint8)]
    rec[:, at + 150:at + 153] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, at + 153:at + 303] = rng.integers(0, 12, (reads, 150), dtype=np.uint8) + ord("5")
    rec[:, at + 303] = ord("\n")
    return rec.tobytes()[:n]


def one_member(data: bytes, level: int, threads: int) -> bytes:
    def one(i):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        return c.compress(data[i:i + BLOCK]) + (c.flush() if i + BLOCK >= len(data) else c.flush(zlib.Z_FULL_FLUSH))

    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, range(0, max(len(data), 1), BLOCK)))
    return struct.pack("<BBBBIBB", 0x1F, 0x8B, 8, 0, 0, 0, 3) + b"".join(parts) + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def child(path: str, piece: int, reps: int):
    """reps + 1 passes over the file with whatever library LX_LIB_PATH names; one JSON line."""
    from lambda_amd import capi

    def one_pass(h, check):
        crc, size, phases = 0, 0, [0.0, 0.0, 0.0]
        t0 = time.perf_counter()
        for p in capi.gunzip_stream(h, path, piece):
            if check:
                crc = zlib.crc32(p, crc)
            size += len(p)
            for i, ph in enumerate((101, 102, 103)):
                phases[i] += h.last_phase_ms(ph)[0]
        secs = time.perf_counter() - t0
        last = h.last_gunzip_stats()  # (behind the call that reported the end: the whole file's)
        return secs, size, crc, {f: getattr(last, f) for f in COUNTS}, phases

    with capi.Handle(0) as h:
        first = one_pass(h, True)  # (buffers, code objects, the file in the page cache; the text's CRC32, which the timed passes leave out)
        runs = [one_pass(h, False) for _ in range(reps)]
    assert all(r[1] == first[1] for r in runs)
    print(json.dumps({"secs": [r[0] for r in runs], "bytes": first[1], "crc": first[2], "counts": runs[-1][3],
                      "find_decode_resolve_ms": [[round(x, 2) for x in r[4]] for r in runs]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 6, 9])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--piece", type=int, default=32 << 20)
    ap.add_argument("--parent-lib", default="", help="the parent commit's liblambda_ext.so: the yardstick")
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.piece, a.reps)
    sink = open(a.out, "a") if a.out else None

    def say(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    data = fastq(a.mb << 20)
    crc = zlib.crc32(data)
    for level in a.levels:
        raw = one_member(data, level, a.threads)
        with tempfile.NamedTemporaryFile(suffix=".fastq.gz") as f:
            f.write(raw)
            f.flush()
            line = {"text": "fastq", "bytes": len(data), "gz_bytes": len(raw), "level": level, "piece": a.piece}
            for name, lib in (("this_tree", ""), ("parent_commit", a.parent_lib)):
                if name == "parent_commit" and not lib:
                    continue
                env = dict(os.environ)
                env.pop("LX_LIB_PATH", None)
                if lib:
                    env["LX_LIB_PATH"] = str(Path(lib).resolve())
                r = subprocess.run([sys.executable, __file__, "--child", f.name, "--piece", str(a.piece), "--reps", str(a.reps)],
                                   capture_output=True, text=True, env=env, timeout=1500)
                assert r.returncode == 0, r.stderr[-2000:]
                got = json.loads(r.stdout.splitlines()[-1])
                assert (got["bytes"], got["crc"]) == (len(data), crc), name
                line[name + "_MBps_runs"] = [round(len(data) / s / 1e6, 1) for s in got["secs"]]
                line[name + "_MBps_median"] = round(statistics.median(line[name + "_MBps_runs"]), 1)
                line[name + "_counts"] = got["counts"]
                line[name + "_find_decode_resolve_ms_runs"] = got["find_decode_resolve_ms"]
            if a.parent_lib:
                line["this_tree_vs_parent_commit"] = round(line["this_tree_MBps_median"] / line["parent_commit_MBps_median"], 2)
            say(line)


if __name__ == "__main__":
    main()
