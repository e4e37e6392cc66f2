"""Text output on the device (lx_write_text_dev) against the host writer's paths.

Record lists of 10^5 and 10^6 rows for BLASTN and BLASTX (tools/bam_render_bench.py's lists) written as .m8 with the standard columns,
.m9 with all 24 columns, .sam with the default tags and .sam with all fourteen (taxonomy included), each plain and .gz.  The host path
of a plain file is lx_write_records_ex + lx_write_footer, of a .gz file lx_write_records_bgzf (lx_render_records on the host threads,
the stream uploaded and compressed on the device); the device path is lx_write_text_dev with bgzf = 0 / 1.  Both end with the same file
on disk (compared once per case); the times are of the C calls alone, the arguments are marshalled before the clock starts.  Per case:
every run and the median of either path after one warm-up run of both, the device time of the render kernels (lx_last_phase_ms phase
12) and of the encoder (phase 4), and the bytes that cross the link: up = what the call uploads (host path: nothing for a plain file,
the rendered stream for .gz; device path: rows, ops, query letters, lengths, offsets and id words), down = the file's bytes.

    python tools/text_render_bench.py > profiles/text_render_bench.txt

--qual gives every query base qualities (lx_output_options::q_qual; both paths then write them as SAM's QUAL, and they count among
the bytes up).  --programs / --cases / --gz pick among the cases.  --dev-only times the device path alone and needs nothing a library
from before --qual lacks, so that two builds can be compared on the same lists (LX_LIB_PATH=... python tools/text_render_bench.py
--dev-only --label parent).
"""
from __future__ import annotations

import argparse
import gzip
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from lambda_amd import capi  # noqa: E402
from tests.test_bam_encoding import ALL_TAGS, _options  # noqa: E402
from tools.bam_render_bench import qualities, records  # noqa: E402

ALL_COLUMNS = ("qseqid sseqid pident length mismatch gapopen qstart qend sstart send evalue bitscore qlen slen score nident positive gaps ppos "
               "frames qframe sframe staxids lcataxid")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--qual", action="store_true", help="write base qualities (q_qual)")
    ap.add_argument("--programs", nargs="*", default=["blastn", "blastx"])
    ap.add_argument("--cases", nargs="*", default=["m8 std", "m9 all columns", "sam default tags", "sam all tags"])
    ap.add_argument("--gz", type=int, nargs="*", default=[0, 1])
    ap.add_argument("--dev-only", action="store_true", help="time lx_write_text_dev alone")
    ap.add_argument("--label", default="", help="copied into every line")
    a = ap.parse_args()
    lib = capi.load()
    tmp = Path(tempfile.mkdtemp(prefix="text_render_bench_"))
    with capi.Handle(0) as h:
        for program in a.programs:
            for rows in a.rows:
                m, ops, names, qa, qoff = records(program, rows)
                qq = qualities(len(qa)) if a.qual else None
                groups = len(set(m["n_qid"].tolist()))
                up_dev = m.nbytes + len(ops) + len(qa) * (2 if a.qual else 1) + 24 * len(names["q_ids"]) + sum(len(x.split()[0]) for x in names["q_ids"]) + 4 * len(m)
                for case, fmt in (("m8 std", capi.LX_OUT_BLAST_TAB), ("m9 all columns", capi.LX_OUT_BLAST_TAB_COMMENTS),
                                  ("sam default tags", capi.LX_OUT_SAM), ("sam all tags", capi.LX_OUT_SAM)):
                    if case not in a.cases:
                        continue
                    if case == "sam default tags" or case == "m8 std":
                        opt, keep = capi.output_options(), None
                    else:
                        opt, keep = _options(program, ALL_TAGS, capi.LX_SAM_SEQ_UNIQ, 1, True, m, 200)
                        opt.columns = ALL_COLUMNS.encode()
                    if qq is not None:
                        args, held = capi._writer_args(m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], qa, qoff, opt, qq)
                    else:
                        args, held = capi._writer_args(m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], qa, qoff, opt)
                    prog = program.encode()
                    for gz in a.gz:
                        p_host, p_dev = tmp / "host.out", tmp / "dev.out"
                        ms = lambda xs, k: [round(x[k] * 1e3, 1) for x in xs]  # noqa: E731

                        def host_path():
                            t0 = time.perf_counter()
                            if gz:
                                rc = lib.lx_write_records_bgzf(h.h, str(p_host).encode(), fmt, prog, *args, groups)
                            else:
                                rc = lib.lx_write_records_ex(str(p_host).encode(), fmt, 1, prog, *args)
                                rc = rc or lib.lx_write_footer(str(p_host).encode(), fmt, groups)
                            t1 = time.perf_counter()
                            assert rc == capi.LX_OK, capi.last_output_error()
                            return dict(total=t1 - t0, bgzf_kernels_ms=h.last_phase_ms(4)[0] if gz else 0.0)

                        def dev_path():
                            t0 = time.perf_counter()
                            rc = lib.lx_write_text_dev(h.h, str(p_dev).encode(), fmt, gz, prog, *args[:3], len(ops), *args[3:], groups)
                            t1 = time.perf_counter()
                            assert rc == capi.LX_OK, lib.lx_last_error(h.h)
                            return dict(total=t1 - t0, render_kernels_ms=h.last_phase_ms(12)[0], bgzf_kernels_ms=h.last_phase_ms(4)[0] if gz else 0.0)

                        if a.dev_only:
                            dev_path()  # (buffers, code objects, pages)
                            ds = [dev_path() for _ in range(a.reps)]
                            print(json.dumps({"label": a.label, "program": program, "rows": rows, "case": case, "gz": bool(gz), "qual": a.qual,
                                              "file_bytes": p_dev.stat().st_size,
                                              "dev_path_ms": ms(ds, "total"), "dev_path_median_ms": round(statistics.median(ms(ds, "total")), 1),
                                              "dev_render_kernels_ms": [round(x["render_kernels_ms"], 2) for x in ds],
                                              "dev_bgzf_kernels_ms": [round(x["bgzf_kernels_ms"], 2) for x in ds]}), flush=True)
                            continue
                        host_path(), dev_path()  # (buffers, code objects, pages)
                        file_bytes = p_host.stat().st_size
                        same = p_host.read_bytes() == p_dev.read_bytes()
                        stream = file_bytes
                        if gz:
                            stream = len(gzip.decompress(p_host.read_bytes()))
                        hs = [host_path() for _ in range(a.reps)]
                        ds = [dev_path() for _ in range(a.reps)]
                        line = {"program": program, "rows": rows, "case": case, "gz": bool(gz), "qual": a.qual, "files_identical": same, "text_bytes": stream,
                                "file_bytes": file_bytes,
                                "host_path_ms": ms(hs, "total"), "host_path_median_ms": round(statistics.median(ms(hs, "total")), 1),
                                "dev_path_ms": ms(ds, "total"), "dev_path_median_ms": round(statistics.median(ms(ds, "total")), 1),
                                "dev_render_kernels_ms": round(statistics.median(x["render_kernels_ms"] for x in ds), 2),
                                "host_bgzf_kernels_ms": round(statistics.median(x["bgzf_kernels_ms"] for x in hs), 2),
                                "dev_bgzf_kernels_ms": round(statistics.median(x["bgzf_kernels_ms"] for x in ds), 2),
                                "host_path_bytes_up": stream if gz else 0, "dev_path_bytes_up": int(up_dev), "bytes_down": file_bytes}
                        line["dev_vs_host"] = round(line["host_path_median_ms"] / line["dev_path_median_ms"], 2)
                        print(json.dumps(line), flush=True)
                    del held, keep
    for p in tmp.iterdir():
        p.unlink()
    tmp.rmdir()


if __name__ == "__main__":
    main()
