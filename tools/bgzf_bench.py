"""Throughput and ratio of the device BGZF encoder (lx_bgzf_compress) against zlib levels 1 and 6 on host threads.

The text is what the writers make (lx_render_records) of synthetic records -- SAM with every tag and the sequence, and .m8 --,
tiled to the asked size.  Host-to-host = the whole lx_bgzf_compress call (copies in and out included); kernel = the encoder's
device time (lx_last_phase_ms phase 4).  zlib compresses the same 65 280-byte blocks as raw DEFLATE on --threads threads.

    python tools/bgzf_bench.py --mb 256 --threads 16 > profiles/bgzf_bench.txt
"""
from __future__ import annotations

import argparse
import json
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi  # noqa: E402
from tests.test_bam_encoding import ALL_TAGS, _case, _options, _render  # noqa: E402

BLOCK = 65280


def texts(n: int):
    m, ops, names, qa, qoff = _case("blastn", seed=5, nq=2000, ns=200)
    opt, _ = _options("blastn", ALL_TAGS, capi.LX_SAM_SEQ_ALWAYS, 1, False, m, 200)
    sam = _render(capi.LX_OUT_SAM, "blastn", m, ops, names, qa, qoff, opt)
    m, ops, names, qa, qoff = _case("blastx", seed=6, nq=2000, ns=200)
    m8 = _render(capi.LX_OUT_BLAST_TAB, "blastx", m, ops, names, qa, qoff, None)
    return {"sam": (sam * (n // len(sam) + 1))[:n], "m8": (m8 * (n // len(m8) + 1))[:n]}


def zlib_blocks(data: bytes, level: int, threads: int):
    def one(i):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        return len(c.compress(data[i:i + BLOCK]) + c.flush())

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        size = sum(ex.map(one, range(0, len(data), BLOCK)))
    return size, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    n = a.mb << 20
    with capi.Handle(0) as h:
        for kind, data in texts(n).items():
            h.bgzf_compress(data[: 8 << 20])  # (buffers and code objects)
            best, kern = 1e9, 1e9
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = h.bgzf_compress(data)
                best = min(best, time.perf_counter() - t0)
                kern = min(kern, h.last_phase_ms(4)[0] / 1e3)
            line = {"text": kind, "bytes": n, "gpu_bytes": len(out), "gpu_ratio": round(n / len(out), 3),
                    "gpu_host_to_host_MBps": round(n / best / 1e6, 1), "gpu_kernel_MBps": round(n / kern / 1e6, 1)}
            for level in (1, 6):
                size, sec = zlib_blocks(data, level, a.threads)
                line[f"zlib{level}_ratio"] = round(n / size, 3)
                line[f"zlib{level}_{a.threads}t_MBps"] = round(n / sec / 1e6, 1)
            line["gpu_vs_zlib6"] = round(line["gpu_host_to_host_MBps"] / line[f"zlib6_{a.threads}t_MBps"], 2)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
