"""`lambda3 searchn` eager against `--query-block N`: wall time, the front end's stage times and peak RSS, three runs each, every
run and the median, into profiles/query_blocks_bench.txt.

    python tools/query_blocks_bench.py [--reads 2000000,8000000] [--blocks 65536,262144,1048576,4194304] [--runs 3] [--mbp 50]
                                       [--parent-cli PATH/lambda3] [--out profiles/query_blocks_bench.txt]

The reads are those of tools/cli_scale_nucl.py (150 bp cut from a random genome of 20 contigs, both strands, 2 % substitutions, a
quarter of the reads random), made here in one vectorised step and without its single-base deletions, so that 8 M reads take
seconds to make.  --parent-cli names the front end of the parent commit, built elsewhere: ITS eager run on the same box is the
yardstick for time (not this tree's eager path), and its run-to-run spread, (max - min) / median, is the tolerance: the default N
is the smallest N whose median is within that spread of the best N's.  Without --parent-cli the tree's own eager run stands in and
the report says so.  The memory claim is read off the same table: lazy RSS at the larger read count against the smaller (expected
flat), beside the eager pair (expected to grow with the reads)."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from lambda_amd import build

ROOT = Path(__file__).resolve().parent.parent


def make_inputs(tmp, n_reads, mbp):
    rng = np.random.default_rng(0x1A3BDA03)
    nt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    genome = nt[rng.integers(0, 4, int(mbp * 1e6))]
    per = len(genome) // 20
    with open(tmp / "g.fasta", "wb") as f:
        for j in range(20):
            f.write(b">chr%d\n" % j + genome[j * per:(j + 1) * per].tobytes() + b"\n")
    path = tmp / f"r{n_reads}.fasta"
    with open(path, "wb") as f:
        for lo in range(0, n_reads, 500_000):
            n = min(500_000, n_reads - lo)
            contig, at = rng.integers(0, 20, n), rng.integers(0, per - 160, n)
            r = genome[(contig * per + at)[:, None] + np.arange(150)[None, :]]
            sub = rng.random(r.shape) < 0.02
            r[sub] = nt[rng.integers(0, 4, int(sub.sum()))]
            k = np.arange(lo, lo + n)
            minus = k % 2 == 1
            r[minus] = comp[r[minus][:, ::-1]]
            rnd = k % 4 == 3
            r[rnd] = nt[rng.integers(0, 4, (int(rnd.sum()), 150))]
            f.write(b"".join(b">read%d\n" % i + row.tobytes() + b"\n" for i, row in zip(k, r)))
    return path


def run(cli, args):
    """(wall s, peak RSS MiB, {stage: ms}, output bytes' hash) of one run; raises when it fails."""
    t0 = time.perf_counter()
    p = subprocess.Popen([str(cli), *map(str, args)], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    err = p.stderr.read()
    _, status, ru = os.wait4(p.pid, 0)
    wall = time.perf_counter() - t0
    if os.waitstatus_to_exitcode(status) != 0:
        raise RuntimeError(err[-2000:])
    line = next(l for l in err.splitlines() if l.startswith("lambda3 times [ms]"))
    stages = {k: float(re.search(rf"{k} (?:\([^)]*\) )?([0-9.]+)", line).group(1)) for k in ("read", "search", "records \\+ output", "total")}
    blocks = next((l for l in err.splitlines() if l.startswith("lambda3 query blocks")), "")
    return wall, ru.ru_maxrss / 1024, stages, blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", default="2000000,8000000")
    ap.add_argument("--blocks", default="65536,262144,1048576,4194304")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--mbp", type=float, default=50)
    ap.add_argument("--parent-cli", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "query_blocks_bench.txt"))
    a = ap.parse_args()
    cli = build.build_cli()
    reads, blocks = [int(x) for x in a.reads.split(",")], [int(x) for x in a.blocks.split(",")]
    tmp = Path(tempfile.mkdtemp(prefix="lx_query_blocks_bench_"))
    out = [f"query_blocks_bench: searchn, {a.mbp:.0f} Mbp genome, {a.runs} run(s) each; wall [s], peak RSS [MiB], stage times [ms]",
           "yardstick for time: " + (f"the parent commit's eager run ({a.parent_cli})" if a.parent_cli else
                                     "THIS tree's eager run (no --parent-cli given: not the yardstick the default N is to be chosen by)")]
    for n in reads:
        q = make_inputs(tmp, n, a.mbp)
        base = ["searchn", "-q", q, "-d", tmp / "g.fasta", "--version-to-outputfile", "0"]
        rows = {}
        configs = ([("parent eager", a.parent_cli, [])] if a.parent_cli else []) + [("eager", cli, [])] + [(f"lazy N={b}", cli, ["--query-block", b]) for b in blocks]
        for name, exe, extra in configs:
            got = [run(exe, base + ["-o", tmp / "out.m8"] + extra) for _ in range(a.runs)]
            rows[name] = got
            for k, (wall, rss, st, bl) in enumerate(got):
                out.append(f"{n:>9} reads  {name:<16} run {k}: wall {wall:7.2f}  rss {rss:8.0f}  " + "  ".join(f"{s.replace(chr(92), '')} {v:.0f}" for s, v in st.items()) +
                           (f"  | {bl.split(': ', 1)[1]}" if bl else ""))
            walls = [g[0] for g in got]
            out.append(f"{n:>9} reads  {name:<16} median: wall {statistics.median(walls):7.2f}  rss {statistics.median(g[1] for g in got):8.0f}  "
                       f"spread (max - min) / median {(max(walls) - min(walls)) / statistics.median(walls):.3f}")
        yard = rows.get("parent eager", rows["eager"])
        yw = [g[0] for g in yard]
        spread = (max(yw) - min(yw)) / statistics.median(yw)
        med = {b: statistics.median(g[0] for g in rows[f"lazy N={b}"]) for b in blocks}
        best = min(med.values())
        choice = min(b for b in blocks if med[b] <= best * (1 + spread))
        out.append(f"{n:>9} reads  yardstick median {statistics.median(yw):.2f} s, spread {spread:.3f}; best lazy median {best:.2f} s; smallest N within the spread of it: {choice}; "
                   f"lazy at that N against the yardstick: {med[choice] / statistics.median(yw):.3f} x")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
