"""BAM output on the device (lx_write_bam_dev) against the host writer's path (lx_render_records(LX_OUT_BAM) + lx_bgzf_compress).

Record lists of 10^5 and 10^6 rows for BLASTN and BLASTX -- the rows, ops and queries of one synthetic case repeated, every repetition
with queries, letters and ops of its own -- with the default tags and with all fourteen (taxonomy included).  Both paths end with the
same .bam file on disk (compared once per list); the times are of the C calls alone, the arguments are marshalled before the clock
starts.  Per list: every run and the median of either path, the host path split into render and compress, the device time of the
render kernels (lx_last_phase_ms phase 11) and of the encoder (phase 4), and the bytes that cross the link: up = what the call
uploads (host path: the rendered stream; device path: rows, ops, query letters, lengths, offsets and id words), down = the members.

    python tools/bam_render_bench.py > profiles/bam_render_bench.txt

--qual gives every query base qualities (lx_output_options::q_qual; both paths then write them, and they count among the bytes up).
--programs / --tags pick among the lists.  --dev-only times the device path alone and needs nothing a library from before --qual
lacks, so that two builds can be compared on the same lists (LX_LIB_PATH=... python tools/bam_render_bench.py --dev-only --label parent).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi  # noqa: E402
from tests.test_bam_encoding import ALL_TAGS, _case, _options  # noqa: E402


def records(program: str, total: int):
    m, ops, names, qa, qoff = _case(program, seed=17, nq=2000, ns=200)
    nq, reps = len(names["q_ids"]), total // len(m) + 1
    big = np.tile(m, reps)
    rep = np.repeat(np.arange(reps, dtype=np.uint64), len(m))
    big["n_qid"] += rep * nq
    big["qry_id"] = big["n_qid"]
    big["ops_off"] += rep * len(ops)
    names = dict(q_ids=[f"read{t}_{x}" for t in range(reps) for x in names["q_ids"]], q_lens=np.tile(names["q_lens"], reps), s_ids=names["s_ids"],
                 s_lens=names["s_lens"])
    off = np.tile(qoff, reps) + np.repeat(np.arange(reps, dtype=np.uint64) * len(qa), nq)
    return big[:total].copy(), ops * reps, names, qa * reps, off


def qualities(n: int) -> bytes:
    """n Phred+33 characters, neighbours different."""
    i = np.arange(n, dtype=np.int64)
    return (33 + (7 * i + i // 94) % 94).astype(np.uint8).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--qual", action="store_true", help="write base qualities (q_qual)")
    ap.add_argument("--programs", nargs="*", default=["blastn", "blastx"])
    ap.add_argument("--tags", nargs="*", default=["default", "all"])
    ap.add_argument("--dev-only", action="store_true", help="time lx_write_bam_dev alone")
    ap.add_argument("--label", default="", help="copied into every line")
    a = ap.parse_args()
    lib = capi.load()
    tmp = Path(tempfile.mkdtemp(prefix="bam_render_bench_"))
    with capi.Handle(0) as h:
        for program in a.programs:
            for rows in a.rows:
                m, ops, names, qa, qoff = records(program, rows)
                qq = qualities(len(qa)) if a.qual else None
                for tags in a.tags:
                    if tags == "all":
                        opt, keep = _options(program, ALL_TAGS, capi.LX_SAM_SEQ_UNIQ, 1, True, m, 200)
                    else:
                        opt, keep = capi.output_options(), None
                    if qq is not None:
                        args, held = capi._writer_args(m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], qa, qoff, opt, qq)
                    else:
                        args, held = capi._writer_args(m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], qa, qoff, opt)
                    prog = program.encode()
                    p_host, p_dev = tmp / "host.bam", tmp / "dev.bam"
                    ms = lambda xs, k: [round(x[k] * 1e3, 1) for x in xs]  # noqa: E731

                    def host_path():
                        t0 = time.perf_counter()
                        raw = C.c_void_p()
                        assert lib.lx_render_records(capi.LX_OUT_BAM, 1, prog, *args, -1, C.byref(raw)) == capi.LX_OK
                        t1 = time.perf_counter()
                        size = lib.lx_bytes_size(raw)
                        out = np.empty(capi.bgzf_bound(size), dtype=np.uint8)
                        got = C.c_uint64(0)
                        rc = lib.lx_bgzf_compress(h.h, lib.lx_bytes_data(raw), size, out.ctypes.data, len(out), C.byref(got), capi.LX_BGZF_EOF)
                        lib.lx_bytes_free(raw)
                        assert rc == capi.LX_OK
                        t2 = time.perf_counter()
                        with open(p_host, "wb") as f:
                            f.write(memoryview(out[: got.value]))
                        t3 = time.perf_counter()
                        return dict(total=t3 - t0, render=t1 - t0, compress=t2 - t1, write=t3 - t2, stream=size, members=int(got.value),
                                    bgzf_kernels_ms=h.last_phase_ms(4)[0])

                    def dev_path():
                        t0 = time.perf_counter()
                        rc = lib.lx_write_bam_dev(h.h, str(p_dev).encode(), prog, *args[:3], len(ops), *args[3:])
                        t1 = time.perf_counter()
                        assert rc == capi.LX_OK, lib.lx_last_error(h.h)
                        return dict(total=t1 - t0, render_kernels_ms=h.last_phase_ms(11)[0], bgzf_kernels_ms=h.last_phase_ms(4)[0])

                    if a.dev_only:
                        dev_path()  # (buffers, code objects, pages)
                        ds = [dev_path() for _ in range(a.reps)]
                        print(json.dumps({"label": a.label, "program": program, "rows": rows, "tags": tags, "qual": a.qual, "bam_bytes": p_dev.stat().st_size,
                                          "dev_path_ms": ms(ds, "total"), "dev_path_median_ms": round(statistics.median(ms(ds, "total")), 1),
                                          "dev_render_kernels_ms": [round(x["render_kernels_ms"], 2) for x in ds],
                                          "dev_bgzf_kernels_ms": [round(x["bgzf_kernels_ms"], 2) for x in ds]}), flush=True)
                        del held, keep
                        continue
                    host_path(), dev_path()  # (buffers, code objects, pages)
                    same = p_host.read_bytes() == p_dev.read_bytes()
                    hs = [host_path() for _ in range(a.reps)]
                    ds = [dev_path() for _ in range(a.reps)]
                    up_dev = (m.nbytes + len(ops) + len(qa) * (2 if a.qual else 1) + 24 * len(names["q_ids"]) + sum(len(x.split()[0]) for x in names["q_ids"]))
                    line = {"program": program, "rows": rows, "tags": tags, "qual": a.qual, "files_identical": same, "stream_bytes": hs[0]["stream"],
                            "bam_bytes": hs[0]["members"],
                            "host_path_ms": ms(hs, "total"), "host_path_median_ms": round(statistics.median(ms(hs, "total")), 1),
                            "host_render_ms": ms(hs, "render"), "host_compress_ms": ms(hs, "compress"), "host_write_ms": ms(hs, "write"),
                            "host_bgzf_kernels_ms": round(statistics.median(x["bgzf_kernels_ms"] for x in hs), 2),
                            "dev_path_ms": ms(ds, "total"), "dev_path_median_ms": round(statistics.median(ms(ds, "total")), 1),
                            "dev_render_kernels_ms": round(statistics.median(x["render_kernels_ms"] for x in ds), 2),
                            "dev_bgzf_kernels_ms": round(statistics.median(x["bgzf_kernels_ms"] for x in ds), 2),
                            "host_path_bytes_up": hs[0]["stream"], "dev_path_bytes_up": int(up_dev), "bytes_down": hs[0]["members"]}
                    line["dev_vs_host"] = round(line["host_path_median_ms"] / line["dev_path_median_ms"], 2)
                    print(json.dumps(line), flush=True)
                    del held, keep
    for p in tmp.iterdir():
        p.unlink()
    tmp.rmdir()


if __name__ == "__main__":
    main()
