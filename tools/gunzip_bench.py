"""Throughput of lx_gunzip on BGZF input: the device path (host to host and kernel only), the host path (h = NULL), and Python's
zlib decompressing the same members on --threads threads.

The inputs are synthetic FASTQ (150-letter reads, qualities) and protein FASTA (60-letter lines), made here and compressed as BGZF
(raw DEFLATE per 65 280-byte block at zlib level 6 behind the BC header).  Host-to-host = the whole lx_gunzip call, copies in and out
included; kernel = the decoder's device time (lx_last_phase_ms phase 5).

    python tools/gunzip_bench.py --mb 256 --threads 16 > profiles/gunzip_bench.txt

--plain measures plain single-member gzip (zlib level 6) of the same two texts instead: lx_gunzip with a handle (the parallel device
path), the same call with LX_OPT_GUNZIP_PARALLEL_FROM = never (the calling thread's decoder: what a handle gave before the
parallel path existed), the same call through a checkout of the parent commit with its library built (--parent-tree, in a child process),
one-thread zlib.decompress, and device against host over a ladder of member sizes (the crossover).  Every run is printed, then the
medians; phase_ms splits the plain-member kernels into find / decode / resolve.

    python tools/gunzip_bench.py --plain --mb 256 --parent-tree /path/to/parent/checkout >> profiles/gunzip_bench.txt
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

# (--tree: the package of another checkout, for the child process that runs the parent commit's library)
sys.path.insert(0, sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv[:-1] else str(Path(__file__).resolve().parent.parent))

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


def gz_member(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def timed(f, reps):
    secs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        secs.append(time.perf_counter() - t0)
    return out, secs


def mbps(n, secs):
    return [round(n / s / 1e6, 1) for s in secs]


def plain_child(path: str, reps: int):
    """lx_gunzip with a handle through the package --tree names (no call of a newer interface)."""
    stream = Path(path).read_bytes()
    # (the figure must come from that checkout's own library: it is older than the parallel path, so it has no stats call)
    assert Path(capi.__file__).resolve().parent.parent == Path(sys.argv[sys.argv.index("--tree") + 1]).resolve()
    assert not hasattr(capi.load(), "lx_last_gunzip_stats"), "the parent checkout's library has the parallel path"
    with capi.Handle(0) as h:
        capi.gunzip(h, stream[:0] + gz_member(b"warm up " * 1000))
        out, secs = timed(lambda: capi.gunzip(h, stream), reps)
    print(json.dumps({"bytes": len(out), "crc": zlib.crc32(out), "secs": secs}))


def plain(a):
    import statistics
    import subprocess
    import tempfile

    n = a.mb << 20
    never = (1 << 64) - 1
    with capi.Handle(0) as h:
        for kind, make in (("fastq", fastq), ("protein_fasta", protein_fasta)):
            data = make(n)
            stream = gz_member(data)
            crc = zlib.crc32(data)
            h.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, 1 << 20)  # (the option's default is never)
            assert capi.gunzip(h, stream) == data  # (buffers and code objects; the whole result checked once)
            runs = {"gpu": [], "find_ms": [], "decode_ms": [], "resolve_ms": []}
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = capi.gunzip(h, stream)
                runs["gpu"].append(time.perf_counter() - t0)
                for key, ph in (("find_ms", 101), ("decode_ms", 102), ("resolve_ms", 103)):
                    runs[key].append(round(h.last_phase_ms(ph)[0], 2))
                assert zlib.crc32(out) == crc
            st = h.last_gunzip_stats()
            h.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, never)
            out, host = timed(lambda: capi.gunzip(h, stream), a.reps)
            assert zlib.crc32(out) == crc and h.last_gunzip_stats().plain_host == 1
            out, zs = timed(lambda: zlib.decompress(stream, 31), a.reps)
            line = {"text": kind, "plain_gzip": True, "bytes": n, "gz_bytes": len(stream), "chunks": st.chunks, "chunks_dropped": st.chunks_dropped,
                    "waves": st.waves, "declined": st.declined, "link_bytes_up": st.bytes_up, "link_bytes_down": st.bytes_down,
                    "gpu_host_to_host_MBps_runs": mbps(n, runs["gpu"]), "find_ms_runs": runs["find_ms"], "decode_ms_runs": runs["decode_ms"],
                    "resolve_ms_runs": runs["resolve_ms"], "handle_host_path_MBps_runs": mbps(n, host), "zlib_1t_MBps_runs": mbps(n, zs)}
            if a.parent_tree:
                with tempfile.NamedTemporaryFile(suffix=".gz") as f:
                    f.write(stream)
                    f.flush()
                    r = subprocess.run([sys.executable, __file__, "--plain-child", f.name, "--reps", str(a.reps), "--tree", a.parent_tree],
                                       capture_output=True, text=True, timeout=600)
                assert r.returncode == 0, r.stderr[-2000:]
                child = json.loads(r.stdout.splitlines()[-1])
                assert (child["bytes"], child["crc"]) == (n, crc)
                line["parent_commit_MBps_runs"] = mbps(n, child["secs"])
            for k in [k for k in line if k.endswith("_runs")]:
                line[k[:-5] + "_median"] = round(statistics.median(line[k]), 2)
            print(json.dumps(line), flush=True)
            if kind != "protein_fasta":
                continue
            # the crossover: device against host over member sizes (best of the runs)
            for mb in (0.5, 1, 2, 4, 16, 64):
                part = gz_member(data[: int(mb * (1 << 20))])
                h.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, 64)
                capi.gunzip(h, part)
                _, dev = timed(lambda: capi.gunzip(h, part), a.reps)
                par = h.last_gunzip_stats().plain_parallel
                h.set_option(capi.LX_OPT_GUNZIP_PARALLEL_FROM, never)
                _, hst = timed(lambda: capi.gunzip(h, part), a.reps)
                print(json.dumps({"crossover": True, "text": kind, "bytes": int(mb * (1 << 20)), "gz_bytes": len(part), "parallel": par,
                                  "device_ms": round(min(dev) * 1e3, 2), "host_ms": round(min(hst) * 1e3, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plain", action="store_true", help="plain single-member gzip instead of BGZF")
    ap.add_argument("--parent-tree", default="", help="--plain: a checkout of the parent commit (library built) to run the same call through")
    ap.add_argument("--tree", default="", help=argparse.SUPPRESS)
    ap.add_argument("--plain-child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.plain_child:
        return plain_child(a.plain_child, a.reps)
    if a.plain:
        return plain(a)
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
