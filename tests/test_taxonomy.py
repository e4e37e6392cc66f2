"""CPU tests of the taxonomy of mkindex* indexes (src/mkindex_algo.hpp:68-107, :277-598, src/mkindex_misc.hpp:69-144): the accession
matcher against Python's re on the reference's pattern, the host join (lx_taxmap_*) and the tree (lx_taxonomy_build) against Python
models of the reference, and the front end's -m / -x with the index's trailing section read from its documented layout."""
import gzip
import re
import struct
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi

ACC_RE = re.compile(
    rb"[OPQ][0-9][A-Z0-9]{3}[0-9]|[A-NR-Z][0-9]([A-Z][A-Z0-9]{2}[0-9]){1,2}|"
    rb"[A-Z][0-9]{5}|[A-Z]{2}[0-9]{6}|"
    rb"[A-Z]{3}[0-9]{5}|"
    rb"[A-Z]{4}[0-9]{8,10}|"
    rb"[A-Z]{5}[0-9]{7}|"
    rb"(NC|AC|NG|NT|NW|NZ|NM|NR|XM|XR|NP|AP|XP|YP|ZP)_[0-9]+|"
    rb"UPI[A-F0-9]{10}")
NCBI_HEADER = b"accession\taccession.version\ttaxid\tgi"
BAD_TAX = "Error: Expected taxonomical ID, but got something I couldn't read: "


# ---- models -------------------------------------------------------------------------------------------------------------------
class ModelError(Exception):
    pass


def model_join(ids, fmt, text: bytes):
    acc2s, no_acc, multi_acc = {}, 0, 0
    for s, i in enumerate(ids):
        ms = [m.group() for m in ACC_RE.finditer(i.encode() if isinstance(i, str) else i)]
        for a in ms:
            acc2s[a] = s
        no_acc += len(ms) == 0
        multi_acc += len(ms) > 1
    lines = text.split(b"\n") if text else []
    if text.endswith(b"\n"):
        lines = lines[:-1]
    first = 1
    if fmt == capi.LX_TAXMAP_NCBI:
        if (lines[0] if lines else b"") != NCBI_HEADER:
            raise ModelError("lx_taxmap: line 1: Unexpected first line in NCBI taxid file.")
        first = 2
    lists = [[] for _ in ids]
    matched = 0
    for ln, line in enumerate(lines[first - 1:], first):
        f = line.split(b"\t")
        if fmt == capi.LX_TAXMAP_UNIPROT and (len(f) < 2 or f[1] != b"NCBI_TaxID"):
            continue
        s = acc2s.get(f[0])
        if s is None:
            continue
        tax = f[2] if len(f) > 2 else b""
        m = re.match(rb"[0-9]+", tax)
        if not m or int(m.group()) > 0xFFFFFFFF:
            raise ModelError(f"lx_taxmap: line {ln}: {BAD_TAX}{tax.decode()}")
        lists[s].append(int(m.group()))
        matched += 1
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.uint64)
    flat = np.array([t for x in lists for t in x], dtype=np.uint32)
    present = np.array(sorted(set(flat.tolist()) | {1}), dtype=np.uint32)
    return {"s_tax_off": off, "s_tax_ids": flat, "present": present, "no_acc": no_acc, "multi_acc": multi_acc,
            "no_tax": sum(len(x) == 0 for x in lists), "multi_tax": sum(len(x) > 1 for x in lists), "lines": len(lines),
            "matched": matched}


def run_join(ids, fmt, text, chunk=0, piece=None, handle=None):
    with capi.TaxMap(handle, fmt, ids, chunk_bytes=chunk) as tm:
        piece = piece or max(1, len(text))
        for a in range(0, len(text), piece):
            tm.feed(text[a:a + piece])
        return tm.finish()


def same_join(got, want):
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(got[k], v), k
        else:
            assert got[k] == v, (k, got[k], v)


def model_tree(nodes: bytes, names: bytes, present):
    edges = []
    for line in nodes.decode().split("\n"):
        if not line:
            continue
        f = line.split("\t")
        edges.append((int(f[0]), int(f[2])))
    size = max([2] + [max(a, b) + 1 for a, b in edges] + [int(p) + 1 for p in present])
    par = [0] * size
    for a, b in edges:
        par[a] = b
    pres = [False] * size
    for p in present:
        pres[int(p)] = True
    pres[1] = True
    kept = list(pres)
    for i in range(size):
        if pres[i]:
            cur = i
            while True:
                cur = par[cur]
                kept[cur] = True
                if cur <= 1:
                    break
    par = [p if kept[i] else 0 for i, p in enumerate(par)]
    indeg = [0] * size
    for p in par:
        indeg[p] += 1
    for i in range(size):
        cur = par[i]
        while cur > 1 and indeg[cur] == 1 and not pres[cur]:
            cur = par[cur]
        par[i] = cur
    for i in range(size):
        if indeg[i] == 1 and not pres[i]:
            par[i] = 0
            kept[i] = False
    hgt = []
    for i in range(size):
        h, cur = 0, par[i]
        while cur > 1:
            cur = par[cur]
            h += 1
        hgt.append(h)
    nm = [""] * size
    for line in names.decode().split("\n"):
        f = line.split("\t")
        if len(f) < 7 or f[6] != "scientific name":
            continue
        t = int(f[0])
        if t >= size:
            raise ModelError(f"Error: taxonomical ID is {t}, but no such taxon in tree.")
        if kept[t]:
            nm[t] = f[2]
    nm[0] = "invalid"
    unnamed = [i for i in range(size) if kept[i] and not nm[i]]
    for i in unnamed:
        nm[i] = "n/a"
    return {"parents": np.array(par, np.uint32), "heights": np.array(hgt, np.uint32), "names": nm, "unnamed": len(unnamed),
            "n_nodes": sum(p > 0 for p in par), "max_height": max(hgt)}


def model_lca(parents, heights, taxa_of_hits):
    """computeLCA folded over a query's hits (src/search_algo.hpp:884-907)."""
    def lca(a, b):
        while heights[a] > heights[b]:
            a = parents[a]
        while heights[b] > heights[a]:
            b = parents[b]
        while a != b:
            a, b = parents[a], parents[b]
        return a
    cur = 0
    for taxa in taxa_of_hits:
        if taxa and parents[taxa[0]] != 0:
            cur = taxa[0]
            break
    if cur:
        for taxa in taxa_of_hits:
            for t in taxa:
                if parents[t] != 0:
                    cur = lca(t, cur)
    return cur


# ---- a small world: a taxdump and a database of accession-bearing ids ---------------------------------------------------------
def taxdump():
    # 1 root; 2 Bacteria <- 1; 3 <- 2 (in-degree 1 chain); 4 <- 3; 5 <- 4; 6 <- 4; 7 Eukaryota <- 1; 8 <- 7; 9 <- 8; 10 <- 8;
    # 11 <- 7 (no name); 12 <- 10; 20 unused <- 1
    edges = [(1, 1), (2, 1), (3, 2), (4, 3), (5, 4), (6, 4), (7, 1), (8, 7), (9, 8), (10, 8), (11, 7), (12, 10), (20, 1)]
    nodes = "".join(f"{a}\t|\t{b}\t|\tno rank\t|\t\t|\n" for a, b in edges).encode()
    names = "".join(f"{a}\t|\t{n}\t|\t\t|\t{c}\t|\n" for a, n, c in [
        (1, "root", "scientific name"), (1, "all", "synonym"), (2, "Bacteria", "scientific name"), (3, "Mid", "scientific name"),
        (4, "Proteobacteria", "scientific name"), (5, "E. coli", "scientific name"), (6, "Salmonella", "scientific name"),
        (7, "Eukaryota", "scientific name"), (8, "Mammalia", "scientific name"), (9, "Homo sapiens", "scientific name"),
        (10, "Mus", "scientific name"), (12, "Mus musculus", "scientific name"), (20, "Unused", "scientific name")]).encode()
    return nodes, names


def test_find_accessions_hand_cases():
    cases = [b"sp|P12345|X_HUMAN", b"A0A023GPI8", b"gi|1|ref|XP_0012345.1|", b"UPI0000000001", b"UPIABCDEF0123", b"ABCD12345678",
             b"ABCD123456789", b"ABCD1234567890", b"ABCD12345678901", b"ABCD1234567", b"P12345P12345", b"A0A023GPI8A0A023",
             b"NC_1NC_2", b"XX_123", b"ABCDE1234567", b"AB123456", b"ABC12345", b"Q9Y2R2-2", b"", b"lowercase p12345", b"O1A2B3C4D5"]
    for c in cases:
        assert capi.find_accessions(c) == [(m.start(), m.end() - m.start()) for m in ACC_RE.finditer(c)], c


def test_find_accessions_random():
    rng = np.random.default_rng(7)
    frags = [b"P12345", b"A0A023GPI8", b"XP_0012345", b"UPI00000000AB", b"UPIABCDEF0123", b"ABCD123456789", b"ABCDE1234567",
             b"AB123456", b"ABC12345", b"NC_", b"sp|", b"|", b".1", b"_HUMAN", b"Q9", b"WP_", b"tr|", b" "]
    alpha = np.frombuffer(b"ABCDEFNOPQRUXZ0123456789_|. ab", np.uint8)
    ids = []
    for _ in range(100_000):
        parts = []
        for _ in range(int(rng.integers(0, 6))):
            if rng.random() < 0.5:
                parts.append(frags[int(rng.integers(0, len(frags)))])
            else:
                parts.append(alpha[rng.integers(0, len(alpha), int(rng.integers(0, 7)))].tobytes())
        ids.append(b"".join(parts))
    text = b"\n".join(ids)  # (no accession spans a newline; one call covers them all)
    assert capi.find_accessions(text) == [(m.start(), m.end() - m.start()) for m in ACC_RE.finditer(text)]


def synthetic(fmt, n_ids=300, n_lines=3000, seed=1):
    """ids with 0-3 accessions (some shared across subjects) and a map over those and other accessions"""
    rng = np.random.default_rng(seed)
    pool = [f"P{d:05d}" for d in range(60)] + [f"XP_{d}" for d in range(60)] + [f"ABC{d:05d}" for d in range(60)] + \
           [f"A0A{d:03d}GPI8" for d in range(60)] + [f"UPIABCDEF{d:04d}" for d in range(60)]
    ids = []
    for s in range(n_ids):
        k = int(rng.integers(0, 4))
        accs = [pool[int(rng.integers(0, len(pool)))] for _ in range(k)]
        ids.append(" ".join(["sp|" + a + "|X" for a in accs] or [f"noacc{s}"]) + " desc")
    lines = [NCBI_HEADER] if fmt == capi.LX_TAXMAP_NCBI else []
    for i in range(n_lines):
        a = pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.7 else f"QQQ{i:05d}"
        t = str(int(rng.integers(2, 60)))
        if rng.random() < 0.05:
            t += "abc"  # from_chars stops at the letters
        if fmt == capi.LX_TAXMAP_NCBI:
            lines.append(f"{a}\t{a}.1\t{t}\t{i}".encode())
        else:
            cat = "NCBI_TaxID" if rng.random() < 0.6 else "GeneID"
            lines.append(f"{a}\t{cat}\t{t}".encode())
    return ids, b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("fmt", [capi.LX_TAXMAP_NCBI, capi.LX_TAXMAP_UNIPROT])
@pytest.mark.parametrize("chunk", [1024, 4096, 0])
def test_host_join_matches_model(fmt, chunk):
    ids, text = synthetic(fmt, seed=fmt * 10 + chunk % 7)
    want = model_join(ids, fmt, text)
    assert want["matched"] > 100 and want["multi_tax"] > 0
    for piece in (None, 1, 37, 4096):
        if piece == 1 and chunk == 0:
            continue
        same_join(run_join(ids, fmt, text, chunk=chunk, piece=piece), want)
    # no final newline: the last line still counts
    same_join(run_join(ids, fmt, text[:-1], chunk=chunk, piece=333), model_join(ids, fmt, text[:-1]))


def join_error_cases():
    ids = ["sp|P12345|A", "ref|XP_77.1| B", "sp|P12345|C later"]
    h = NCBI_HEADER + b"\n"
    return ids, [
        ("bad header", capi.LX_TAXMAP_NCBI, b"accession\ttaxid\n" + b"P12345\tP12345.1\t9\t1\n"),
        ("empty NCBI file", capi.LX_TAXMAP_NCBI, b""),
        ("bad taxid on a matched line", capi.LX_TAXMAP_NCBI, h + b"Q00001\tx\tnope\t1\nP12345\tP.1\t9\t1\nXP_77\tX\t+5\t2\nP12345\tP\tabc\t3\n"),
        ("overflow", capi.LX_TAXMAP_NCBI, h + b"XP_77\tX\t4294967296\t2\n"),
        ("missing field", capi.LX_TAXMAP_NCBI, h + b"P12345\n"),
        ("uniprot bad", capi.LX_TAXMAP_UNIPROT, b"P12345\tGeneID\tzz\nXP_77\tNCBI_TaxID\t\nP12345\tNCBI_TaxID\t5\n"),
    ]


def test_host_join_errors():
    ids, cases = join_error_cases()
    for name, fmt, text in cases:
        with pytest.raises(ModelError) as me:
            model_join(ids, fmt, text)
        for chunk, piece in ((0, None), (32, 3), (1024, 5)):
            with pytest.raises(capi.LambdaExtError) as e:
                run_join(ids, fmt, text, chunk=chunk, piece=piece)
            assert e.value.code == capi.LX_EINVAL and str(me.value) in str(e.value), (name, str(e.value), str(me.value))
    # bad taxa on lines whose accession is not in the table are never read; 4294967295 is the largest taxon
    text = NCBI_HEADER + b"\nQ00001\tx\tnope\t1\nXP_77\tX\t4294967295\t2\nP12345\tP\t007\t3\n"
    got = run_join(ids, capi.LX_TAXMAP_NCBI, text, chunk=32, piece=7)
    same_join(got, model_join(ids, capi.LX_TAXMAP_NCBI, text))
    assert got["s_tax_ids"].tolist() == [4294967295, 7] and got["s_tax_off"].tolist() == [0, 0, 1, 2]


# ---- texts built around the device join's structural bounds (join_parse_kernel, lx_taxmap.hip) ---------------------------------------
# The kernel sees a chunk of whole lines -- for the NCBI form, what follows the header line -- in tiles of JOIN_TILE bytes, 16 bytes per
# lane; with chunk_bytes = 0 the whole text is one chunk, so an offset below is an offset in that chunk.
JOIN_TILE = 4096            # kJoinTile
JOIN_TILE_CAP = 512         # kJoinTileCap = kJoinTile / 8
EDGE_IDS = ["ref|NC_1| the shortest accession", "sp|P12345|B_X", "ref|XP_77.1| C", "sp|P12345|D later"]


class _Chunk:
    """the lines of one chunk, with the offset the next line starts at"""

    def __init__(self, fmt, seed):
        self.fmt, self.rng, self.parts, self.pos = fmt, np.random.default_rng(seed), [], 0

    def add(self, line: bytes):
        self.parts.append(line)
        self.pos += len(line)

    def match(self, acc: str, tax, tail: str = "77"):
        """a line whose accession is in the table"""
        self.add((f"{acc}\t{acc}.1\t{tax}\t{tail}\n" if self.fmt == capi.LX_TAXMAP_NCBI else f"{acc}\tNCBI_TaxID\t{tax}\n").encode())

    def ordinary(self):
        """a line as the other texts have them: 20 to 38 bytes, most of them matching"""
        k = int(self.rng.integers(0, 1000))
        acc = ("P12345", "XP_77", "NC_1")[k % 3] if k % 10 < 7 else f"QQQ{k:05d}"
        if self.fmt == capi.LX_TAXMAP_UNIPROT and k % 4 == 0:
            self.add(f"{acc}\tGeneID\t{k}\n".encode())
        else:
            self.match(acc, 100 + k, tail=str(k))

    def pad_to(self, target: int):
        """ordinary lines, then one line that matches nothing and ends just before `target`"""
        assert target >= self.pos
        while target - self.pos > 120:
            self.ordinary()
        gap = target - self.pos
        if gap:
            self.add(b"Z" * (gap - 1) + b"\n")
        assert self.pos == target

    def text(self, final_newline=True) -> bytes:
        body = b"".join(self.parts)
        if not final_newline:
            assert body.endswith(b"\n")
            body = body[:-1]
        return (NCBI_HEADER + b"\n" if self.fmt == capi.LX_TAXMAP_NCBI else b"") + body


def edge_join_cases():
    """(name, fmt, ids, text) texts whose join succeeds"""
    out = []
    N, U = capi.LX_TAXMAP_NCBI, capi.LX_TAXMAP_UNIPROT
    # densest tile: "NC_1\t\t1\n" is the shortest line that yields a pair (8 bytes: kJoinTileCap's bound).  From offset 0 every tile
    # holds 512 of them, two per lane (`a` and `b`, cnt == 2 without the overflow flag; excl + 1 == 511 in the last lane)
    c = _Chunk(N, 1)
    for i in range(3000):
        c.add(f"NC_1\t\t{1 + i % 9}\n".encode())
    assert c.pos == 3000 * 8 and c.pos > 5 * JOIN_TILE
    out.append(("densest tile: 512 pairs, two per lane", N, EDGE_IDS, c.text()))
    # the same shifted by 1 .. 7 bytes (an empty line before each run of 700): the lane's two line starts sit at s and s + 8 of its 16
    # bytes; the tile an empty line falls in has room for 511 or 512 lines, and three lines name an accession that is not in
    # the table (their lanes have cnt == 1), so tiles hold 511 or 512 pairs
    c = _Chunk(N, 2)
    for shift in range(1, 8):
        c.add(b"\n")
        assert c.pos % 8 == shift
        for i in range(700):
            c.add(f"NC_{2 if (shift, i) in ((2, 300), (4, 350), (7, 600)) else 1}\t\t{1 + (i + shift) % 9}\n".encode())
    out.append(("densest tile shifted by 1 .. 7 bytes: 511 or 512 pairs", N, EDGE_IDS, c.text()))
    # a matching line that starts d bytes before a tile's edge, d = 0 .. 24.  d = 0 is a line start on a tile's first byte (`prev` is
    # text[t0 - 1]); the others split field 0, "NCBI_TaxID" or the taxon's digits across the tiles (get()'s `q < n ? text[q]` path)
    for fmt in (N, U):
        c = _Chunk(fmt, 3 + fmt)
        for d in range(25):
            c.pad_to(JOIN_TILE * (d + 1) - d)
            c.match("XP_77" if fmt == N else "P12345", 10000 + d)
            c.match("NC_1", 20000 + d)
        c.ordinary()
        out.append((f"a line start 0 .. 24 bytes before a tile's edge, format {fmt}", fmt, EDGE_IDS, c.text()))
    # long lines: field 0 of 9999 bytes (beyond max_len: lookup() refuses it by its length) and a matching line whose fourth field is
    # 9000 bytes, so that at least one whole tile has no line start (lines == 0, cnt == 0 in all of its lanes, tile_cnt == 0 in the scan)
    for fmt in (N, U):
        c = _Chunk(fmt, 5 + fmt)
        c.pad_to(1000)
        c.match("P12345", 31)
        c.add(b"A" * 9999 + b"\n")
        c.match("XP_77", 32)
        c.ordinary()
        c.match("NC_1", 33)
        c.add((b"NC_1\tNC_1.1\t34\t" if fmt == N else b"NC_1\tNCBI_TaxID\t34\t") + b"9" * 9000 + b"\n")
        c.match("P12345", 35)
        c.ordinary()
        out.append((f"lines of 10 000 and 9 000 bytes, format {fmt}", fmt, EDGE_IDS, c.text()))
    # empty lines: 100 '\n' in a row are 100 lines, 16 line starts in a lane and no pair
    for fmt in (N, U):
        c = _Chunk(fmt, 7 + fmt)
        c.pad_to(JOIN_TILE - 40)
        c.match("XP_77", 41)
        for _ in range(100):
            c.add(b"\n")
        c.match("P12345", 42)
        c.ordinary()
        out.append((f"a run of 100 empty lines, format {fmt}", fmt, EDGE_IDS, c.text()))
    # no final newline at a tile's end: the chunk is 4096 k or 4096 k + 1 bytes before lx_taxmap_finish appends the '\n', and the last
    # line matches (tn == 1 in the last tile: the staging loop for a partial tile)
    for fmt in (N, U):
        for extra in (0, 1):
            c = _Chunk(fmt, 9 + fmt)
            last = (b"XP_77\tXP_77.1\t51\t1\n" if fmt == N else b"XP_77\tNCBI_TaxID\t51\n")
            c.pad_to(2 * JOIN_TILE + extra - (len(last) - 1))
            c.add(last)
            t = c.text(final_newline=False)
            assert c.pos - 1 == 2 * JOIN_TILE + extra and not t.endswith(b"\n")
            out.append((f"no final newline, {2 * JOIN_TILE + extra} bytes, format {fmt}", fmt, EDGE_IDS, t))
    return out


def edge_join_error_cases():
    """(name, fmt, ids, text): two matched lines whose taxa do not parse, in tiles 1 and 3 of the one chunk; the error names the one in
    tile 1, whichever workgroup runs first (atomicMin on bad_off) and whichever host thread's part it falls in"""
    out = []
    for fmt in (capi.LX_TAXMAP_NCBI, capi.LX_TAXMAP_UNIPROT):
        c = _Chunk(fmt, 11 + fmt)
        c.pad_to(JOIN_TILE + 100)
        c.match("XP_77", "first-bad")
        c.pad_to(3 * JOIN_TILE + 100)
        c.match("P12345", "second-bad")
        c.ordinary()
        out.append((f"bad taxa in tiles 1 and 3, format {fmt}", fmt, EDGE_IDS, c.text()))
    return out


def fit_chunk(chunk: int, text: bytes) -> int:
    """chunk_bytes for a text: a line longer than the chunk is refused by design, so the chunk is doubled until the longest line fits"""
    longest = max(len(l) for l in text.split(b"\n")) + 1
    while 0 < chunk < longest:
        chunk *= 2
    return chunk


@pytest.mark.parametrize("case", range(12))
def test_host_join_edge_texts_match_model(case):
    name, fmt, ids, text = edge_join_cases()[case]
    want = model_join(ids, fmt, text)
    assert want["matched"] >= 2, name
    if name.startswith("densest tile:"):
        assert want["matched"] == 3000 and want["s_tax_ids"].tolist() == [1 + i % 9 for i in range(3000)]
    for chunk in (0, 4096, 1024):
        for piece in (None, 37, 4096):
            same_join(run_join(ids, fmt, text, chunk=fit_chunk(chunk, text), piece=piece), want)


def test_edge_join_cases_are_what_they_claim():
    cases = edge_join_cases()
    assert len(cases) == 12
    for name, fmt, ids, text in cases:
        body = text[len(NCBI_HEADER) + 1:] if fmt == capi.LX_TAXMAP_NCBI else text
        nl = np.nonzero(np.frombuffer(body, np.uint8) == 10)[0]
        starts = [0] + [int(i) + 1 for i in nl if i + 1 < len(body)]
        acc = (b"NC_1\t", b"P12345\t", b"XP_77\t")
        per_tile = np.bincount([p // JOIN_TILE for p in starts if body.startswith(acc, p) and b"GeneID" not in body[p:p + 16]])
        if name.startswith("densest tile:"):
            assert (per_tile[:5] == JOIN_TILE_CAP).all()
        elif name.startswith("densest tile shifted"):
            assert set(per_tile[:-1].tolist()) == {JOIN_TILE_CAP - 1, JOIN_TILE_CAP} and {p % 8 for p in starts} == set(range(8))
        elif name.startswith("a line start"):
            assert all(JOIN_TILE * (d + 1) - d in starts for d in range(25))
        elif name.startswith("lines of"):
            tiles_with_start = {p // JOIN_TILE for p in starts}
            assert len(set(range(len(body) // JOIN_TILE)) - tiles_with_start) >= 2
        elif name.startswith("a run of 100"):
            assert b"\n" * 101 in body
        else:
            assert len(body) in (2 * JOIN_TILE, 2 * JOIN_TILE + 1) and not body.endswith(b"\n")


def test_host_join_first_bad_taxon_in_line_order():
    for name, fmt, ids, text in edge_join_error_cases():
        with pytest.raises(ModelError) as me:
            model_join(ids, fmt, text)
        assert "first-bad" in str(me.value)
        for chunk, piece in ((0, None), (4096, 37), (1024, 4096)):
            with pytest.raises(capi.LambdaExtError) as e:
                run_join(ids, fmt, text, chunk=chunk, piece=piece)
            assert e.value.code == capi.LX_EINVAL and str(me.value) in str(e.value), (name, str(e.value), str(me.value))


def test_tree_matches_model():
    nodes, names = taxdump()
    for present in ([5, 6], [9, 12, 5], [3, 9], [11], [5, 30], [12, 10, 8]):
        got, want = capi.taxonomy_build(nodes, names, present), model_tree(nodes, names, present)
        for k in ("parents", "heights"):
            assert np.array_equal(got[k], want[k]), (present, k, got[k], want[k])
        assert [n for n in got["names"]] == want["names"], present
        assert (got["unnamed"], got["n_nodes"], got["max_height"]) == (want["unnamed"], want["n_nodes"], want["max_height"])
    got = capi.taxonomy_build(nodes, names, [11, 30])
    assert got["names"][11] == "n/a" and got["parents"][30] == 0 and len(got["parents"]) == 31
    assert 'Taxon with ID 11 has no name associated, defaulting to "n/a".' in got["warnings"]
    with pytest.raises(capi.LambdaExtError) as e:
        capi.taxonomy_build(nodes, names + b"99\t|\tGhost\t|\t\t|\tscientific name\t|\n", [5])
    assert "Error: taxonomical ID is 99, but no such taxon in tree." in str(e.value)
    with pytest.raises(capi.LambdaExtError) as e:
        capi.taxonomy_build(b"x\t|\t1\t|\n", names, [5])
    assert BAD_TAX + "x" in str(e.value)


# ---- the front end ------------------------------------------------------------------------------------------------------------
STD = "ACDEFGHIKLMNPQRSTVWY"


def world(tmp, n=40, seed=3, dup=False):
    """a protein database whose ids carry accessions, an NCBI map, a UniProt map and a taxdump (dup: subjects 2k and 2k + 1 share
    their sequence, so that a query hits both)"""
    rng = np.random.default_rng(seed)
    taxa = [5, 6, 9, 12, 10, 11]
    ids, ncbi, uni = [], [NCBI_HEADER.decode()], []
    for s in range(n):
        acc = f"P{s:05d}"
        ids.append(f"sp|{acc}|PROT{s}_X protein {s}" if s % 7 else f"ref|XP_{s}.1| no. {s} also A{s:05d}")
        if s % 5:
            t = taxa[s % len(taxa)]
            ncbi.append(f"{acc}\t{acc}.1\t{t}\t{1000 + s}")
            uni.append(f"{acc}\tNCBI_TaxID\t{t}")
            uni.append(f"{acc}\tGeneID\t{s}")
        if s % 7 == 0:
            ncbi.append(f"XP_{s}\tXP_{s}.1\t{taxa[(s + 1) % len(taxa)]}\t{2000 + s}")
    seqs = ["".join(STD[i] for i in rng.integers(0, 20, int(rng.integers(80, 200)))) for _ in range(n)]
    if dup:
        seqs = [seqs[s - s % 2] for s in range(n)]
    with open(tmp / "db.fasta", "w") as f:
        for i, sq in zip(ids, seqs):
            f.write(f">{i}\n{sq}\n")
    (tmp / "m.accession2taxid").write_text("\n".join(ncbi) + "\n")
    (tmp / "m.accession2taxid.gz").write_bytes(gzip.compress(((tmp / "m.accession2taxid").read_bytes())))
    (tmp / "idmapping.dat").write_text("\n".join(uni))
    (tmp / "dump").mkdir(exist_ok=True)
    nodes, names = taxdump()
    (tmp / "dump" / "nodes.dmp").write_bytes(nodes)
    (tmp / "dump" / "names.dmp").write_bytes(names)
    return ids, seqs


def read_section(data: bytes, at: int):
    assert data[at:at + 8] == b"LXTAXON1"
    p = at + 8
    n_s, = struct.unpack_from("<Q", data, p)
    p += 8
    off = np.frombuffer(data, np.uint64, n_s + 1, p)
    p += 8 * (n_s + 1)
    ids = np.frombuffer(data, np.uint32, int(off[-1]), p)
    p += 4 * int(off[-1])
    has_tree, = struct.unpack_from("<Q", data, p)
    p += 8
    out = {"s_tax_off": off, "s_tax_ids": ids, "has_tree": has_tree}
    if has_tree:
        n, = struct.unpack_from("<Q", data, p)
        p += 8
        out["parents"] = np.frombuffer(data, np.uint32, n, p)
        out["heights"] = np.frombuffer(data, np.uint32, n, p + 4 * n)
        lens = np.frombuffer(data, np.uint32, n, p + 8 * n)
        p += 12 * n
        names = []
        for L in lens:
            names.append(data[p:p + int(L)].decode())
            p += int(L)
        out["names"] = names
    assert p == len(data)
    return out


def _run(*a, cwd=None):
    return subprocess.run([str(build.build_cli()), *map(str, a)], capture_output=True, text=True, cwd=cwd)


@pytest.mark.parametrize("cmd", ["mkindexp", "mkindexn", "mkindexbs"])
def test_cli_mkindex_taxonomy(tmp_path, cmd):
    ids, seqs = world(tmp_path)
    if cmd != "mkindexp":  # nucleotide databases: the same ids over nucleotide letters
        with open(tmp_path / "db.fasta", "w") as f:
            for i, sq in zip(ids, seqs):
                f.write(f">{i}\n{''.join('ACGT'[ord(c) % 4] for c in sq)}\n")
    db = tmp_path / "db.fasta"
    r = _run(cmd, "-d", db, "-i", tmp_path / "plain.lba")
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "plain.lba").read_bytes()
    nodes, names = taxdump()
    cases = [("ncbi.lba", ["-m", tmp_path / "m.accession2taxid", "-x", tmp_path / "dump"], capi.LX_TAXMAP_NCBI, "m.accession2taxid", True),
             ("gz.lba", ["-m", tmp_path / "m.accession2taxid.gz", "-x", tmp_path / "dump", "-t", "3"], capi.LX_TAXMAP_NCBI, "m.accession2taxid", True),
             ("uni.lba", ["-m", tmp_path / "idmapping.dat"], capi.LX_TAXMAP_UNIPROT, "idmapping.dat", False)]
    for name, extra, fmt, mapfile, tree in cases:
        r = _run(cmd, "-d", db, "-i", tmp_path / name, *extra)
        assert r.returncode == 0, r.stderr
        assert "Subjects without tax IDs:" in r.stderr and "Subjects with more than one tax ID:" in r.stderr
        assert ("Maximum Tree Height:" in r.stderr) == tree
        data = (tmp_path / name).read_bytes()
        assert data[:len(plain)] == plain  # the old layout is untouched: the section follows it
        sec = read_section(data, len(plain))
        want = model_join(ids, fmt, (tmp_path / mapfile).read_bytes())
        assert np.array_equal(sec["s_tax_off"], want["s_tax_off"]) and np.array_equal(sec["s_tax_ids"], want["s_tax_ids"])
        assert f"Subjects without tax IDs:             {want['no_tax']}/{len(ids)}" in r.stderr
        assert sec["has_tree"] == int(tree)
        if tree:
            mt = model_tree(nodes, names, want["present"])
            assert np.array_equal(sec["parents"], mt["parents"]) and np.array_equal(sec["heights"], mt["heights"])
            assert sec["names"] == mt["names"]


def test_cli_taxonomy_refusals(tmp_path):
    world(tmp_path)
    db = tmp_path / "db.fasta"
    r = _run("mkindexp", "-d", db, "-i", tmp_path / "a.lba", "-x", tmp_path / "dump")
    assert r.returncode != 0 and "There is no point in including a taxonomic tree in the index, if you don't also include taxonomic IDs for your sequences." in r.stderr
    r = _run("mkindexp", "-d", db, "-i", tmp_path / "b.lba", "-m", tmp_path / "map.tsv")
    assert r.returncode != 0 and "taxonomy" in r.stderr
    r = _run("mkindexp", "-d", db, "-i", tmp_path / "c.lba", "-m", tmp_path / "m.accession2taxid.bz2")
    assert r.returncode != 0 and "bzip2" in r.stderr
    bad = tmp_path / "bad.accession2taxid"
    bad.write_text("accession\ttaxid\nP00001\tP00001.1\t5\t1\n")
    r = _run("mkindexp", "-d", db, "-i", tmp_path / "d.lba", "-m", bad)
    assert r.returncode != 0 and "Unexpected first line in NCBI taxid file." in r.stderr
    assert not (tmp_path / "d.lba").exists()
