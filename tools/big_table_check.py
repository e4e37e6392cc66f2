"""The sliced word-table build (LX_OPT_INDEX_SLICE_WORDS) at sizes no test reaches, on seeded random dna4 sets.  A tool, not a test:
no threshold, the figures go to profiles/big_table_check.txt (or --out).
    python tools/big_table_check.py overhead [log2_words = 28]    one sort against slices of a quarter and half the set, three runs each:
                                                                  what slicing costs where it is not needed
    python tools/big_table_check.py real [words = 2^31 + 2^20]    beyond one sort, with the front end's 2^30 words per slice: the table
                                                                  against the h == NULL build's (SHA-256 of lx_index_save), seeding on it
The real run holds two tables of 16 bytes a word in host memory, and one lx_index_save of as much at a time."""
import argparse, ctypes as C, hashlib, sys, threading, time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from lambda_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["overhead", "real"])
ap.add_argument("size", nargs="?", type=int)
ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "big_table_check.txt"))
ap.add_argument("--threads", type=int, default=16)
args = ap.parse_args()
out = open(args.out, "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def dna4(total, seed):
    """`total` letters of 0..3 in sequences of 2^26 letters (the last one shorter)"""
    rng = np.random.default_rng(seed)
    red = np.empty(total, np.uint8)
    for a in range(0, total, 1 << 28):
        red[a:a + (1 << 28)] = rng.integers(0, 4, min(1 << 28, total - a), dtype=np.uint8)
    lens = np.full(-(-total // (1 << 26)), 1 << 26, np.uint64)
    lens[-1] = total - (len(lens) - 1) * (1 << 26)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    return red, off, lens


def build(handle, hip, slice_words, red, off, lens):
    """lx_index_build on the handle: (index, wall s, phase-8 ms, launches, peak device bytes above what stood before)"""
    free, tot = C.c_size_t(), C.c_size_t()
    hip.hipMemGetInfo(C.byref(free), C.byref(tot))
    before, least, stop = free.value, [free.value], threading.Event()

    def watch():
        f, t = C.c_size_t(), C.c_size_t()
        while not stop.wait(0.01):
            if hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0:
                least[0] = min(least[0], f.value)

    th = threading.Thread(target=watch)
    th.start()
    handle.set_option(capi.LX_OPT_INDEX_SLICE_WORDS, slice_words)
    t0 = time.perf_counter()
    try:
        ix = capi.Index.build(handle, red, off, lens, 4, args.threads)
    finally:
        wall = time.perf_counter() - t0
        handle.set_option(capi.LX_OPT_INDEX_SLICE_WORDS, 0)
        stop.set()
        th.join()
    ms, launches = handle.last_phase_ms(8)
    return ix, wall, ms, launches, before - least[0]


def sha_of_save(ix):
    """SHA-256 of lx_index_save's bytes, hashed where they stand"""
    lib, b = capi.load(), C.c_void_p()
    if lib.lx_index_save(ix.ix, C.byref(b)) != capi.LX_OK:
        raise RuntimeError("lx_index_save: " + capi.last_output_error())
    try:
        n, h = lib.lx_bytes_size(b), hashlib.sha256()
        base = lib.lx_bytes_data(b)
        base = base if isinstance(base, int) else C.cast(base, C.c_void_p).value
        for a in range(0, n, 1 << 30):
            h.update((C.c_ubyte * min(1 << 30, n - a)).from_address(base + a))
        return h.hexdigest(), n
    finally:
        lib.lx_bytes_free(b)


def overhead(log2_words):
    total = 1 << log2_words
    red, off, lens = dna4(total, 0x51CE)
    say(f"== overhead: a seeded random dna4 set of 2^{log2_words} = {total} words in {len(lens)} sequences, lx_index_build on the handle, three runs each")
    with capi.Handle(0) as h:
        hip = hip_runtime()
        build(h, hip, 0, red[:1 << 20], off[:1], np.array([1 << 20], np.uint64))[0].close()  # (the first launch's one-off costs)
        want = None
        for name, n in (("one sort", 0), (f"slices of 2^{log2_words - 2}", total >> 2), (f"slices of 2^{log2_words - 1}", total >> 1)):
            runs = []
            for r in range(3):
                ix, wall, ms, launches, peak = build(h, hip, n, red, off, lens)
                digest = hashlib.sha256(ix.entries(0, 1 << 20).tobytes() + ix.entries(total - (1 << 20), 1 << 20).tobytes()).hexdigest()[:16]
                ix.close()
                want = want or digest
                runs.append((wall, ms, peak))
                say(f"{name} run {r + 1}: wall {wall * 1e3:.0f} ms, phase 8 {ms:.1f} ms in {launches} launch(es), peak device memory {peak / 2 ** 30:.2f} GiB"
                    f" ({peak / total:.1f} B per word), first and last 2^20 entries {'equal' if digest == want else 'DIFFER'}")
            med = lambda k: sorted(x[k] for x in runs)[1]
            say(f"{name} median: wall {med(0) * 1e3:.0f} ms, phase 8 {med(1):.1f} ms, peak {med(2) / 2 ** 30:.2f} GiB")


def real(total):
    red, off, lens = dna4(total, 0xB16)
    say(f"== real size: a seeded random dna4 set of {total} words (2^31 + {total - 2 ** 31}) in {len(lens)} sequences, slices of 2^30 words")
    with capi.Handle(0) as h:
        hip = hip_runtime()
        dev, wall, ms, launches, peak = build(h, hip, 1 << 30, red, off, lens)
        say(f"lx_index_build on the handle: wall {wall:.1f} s, phase 8 {ms:.0f} ms in {launches} slice(s), peak device memory {peak / 2 ** 30:.1f} GiB ({peak / total:.1f} B per word)")
        t0 = time.perf_counter()
        sha_dev, n = sha_of_save(dev)
        say(f"lx_index_save: {n} bytes, sha256 {sha_dev} ({time.perf_counter() - t0:.0f} s to save and hash)")
        t0 = time.perf_counter()
        host = capi.Index.build(None, red, off, lens, 4, args.threads)
        say(f"lx_index_build with h == NULL on {args.threads} threads: {time.perf_counter() - t0:.1f} s")
        sha_host, _ = sha_of_save(host)
        say(f"lx_index_save: sha256 {sha_host} -- {'IDENTICAL' if sha_host == sha_dev else 'DIFFERENT'}")
        # 10^5 reads of 100 letters: pieces of the subjects with 4 % substitutions; the reduced letters double as alignment ranks
        rng = np.random.default_rng(7)
        starts = rng.integers(0, total - 200, 100000)
        starts -= np.maximum(0, (starts % (1 << 26)) + 100 - (1 << 26))  # (inside one sequence)
        q = np.concatenate([red[a:a + 100] for a in starts])
        sub = rng.random(len(q)) < 0.04
        q[sub] = rng.integers(0, 4, int(sub.sum()), dtype=np.uint8)
        q_len = np.full(100000, 100, np.uint64)
        q_off = (np.arange(100000, dtype=np.uint64) * np.uint64(100))
        matrix = np.full((capi.LX_ALPH, capi.LX_ALPH), -3, np.int8)
        np.fill_diagonal(matrix, 2)
        p = capi.seed_params(matrix, seed_length=14, seed_offset=7, max_seed_dist=1, unknown_rank=31, host_threads=args.threads)
        order = [f for f in capi.MATCH_DTYPE.names]
        t0 = time.perf_counter()
        d = capi.seed_queries(h, dev, red, q, q, q_off, q_len, p)
        t_dev, (k_ms, k_n) = time.perf_counter() - t0, h.last_phase_ms(9)
        t0 = time.perf_counter()
        g = capi.seed_queries(None, host, red, q, q, q_off, q_len, p)
        t_host = time.perf_counter() - t0
        same = np.array_equal(np.sort(d.matches(), order=order), np.sort(g.matches(), order=order))
        say(f"lx_seed_queries of 100000 reads: on the resident table {t_dev:.2f} s wall (kernel {k_ms:.0f} ms in {k_n} launch(es), {d.stats.reads_declined} read(s) declined, "
            f"{d.stats.launches_full} launch(es) full), host path {t_host:.2f} s; {d.stats.n_matches} / {g.stats.n_matches} matches, sorted lists {'EQUAL' if same else 'DIFFER'}")
        d.close(), g.close(), dev.close(), host.close()


if args.mode == "overhead":
    overhead(args.size or 28)
else:
    real(args.size or (1 << 31) + (1 << 20))
