"""lx_gunzip_stream's walk with a plain member decoded wave by wave (lambda_amd/csrc/lx_gunzip_stream.h), without a GPU:
tests/native/gunzip_stream_check.cpp runs the library's Stream over waves made by the __host__ __device__ functions of
lx_pgunzip.h in loops, under AddressSanitizer and UBSan, every buffer of a wave a heap block of its exact size.  zlib says what
every file decodes to; lx_gunzip without a handle says what a damaged one is called; the same walk with no device says in which
call the damage is reached."""
import subprocess
import zlib
from pathlib import Path

import pytest

from lambda_amd import build, capi
from tests import gunzip_stream_parallel_cases as sc
from tests import pgunzip_cases as pc

ROOT = Path(__file__).resolve().parent.parent
NO_BOUNDARY = 1  # LX_GUNZIP_DECLINE_NO_BOUNDARY
FIELDS = ("piece", "plain_parallel", "plain_host", "declined", "last_decline", "chunks", "dropped", "waves", "bgzf_members", "bytes_down")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    rocm_include = Path(build._hipcc()).resolve().parent.parent / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        rocm_include = Path("/opt/rocm/include")
    out = tmp_path_factory.mktemp("gunzip_stream_check") / "gunzip_stream_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           f"-I{rocm_include}", f"-I{ROOT / 'include'}", f"-I{ROOT / 'lambda_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "gunzip_stream_check.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, tmp_path, records):
    """records: (chunk, wave, piece, device, file) -> per record {rc, calls: [dict per call], total: sums, checked, mismatches, error, pieces}."""
    corpus, out = tmp_path / "corpus.bin", tmp_path / "bytes.bin"
    corpus.write_bytes(sc.pack_corpus([(c, w, p, dev, sc.FROM, d) for c, w, p, dev, d in records]))
    r = subprocess.run([str(exe), str(corpus), str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    got, at, res = out.read_bytes(), 0, []
    for line in r.stdout.splitlines():
        tag, rest = line[0], line[2:]
        if tag == "R":
            i, rc, ncalls = (int(x) for x in rest.split())
            assert i == len(res)
            res.append({"rc": rc, "ncalls": ncalls, "calls": [], "error": None, "pieces": []})
        elif tag == "C":
            c = dict(zip(FIELDS, (int(x) for x in rest.split())))
            res[-1]["calls"].append(c)
            if c["piece"] >= 0:
                res[-1]["pieces"].append(got[at:at + c["piece"]])
                at += c["piece"]
        elif tag == "X":
            res[-1]["checked"], res[-1]["mismatches"] = (int(x) for x in rest.split())
        elif tag == "E":
            res[-1]["error"] = rest
    assert at == len(got) and len(res) == len(records)
    for o in res:
        assert len(o["calls"]) == o["ncalls"]
        o["total"] = {f: sum(c[f] for c in o["calls"]) for f in FIELDS[1:]}
        assert o["mismatches"] == 0, o  # chain_wave(), chain() and the restated rule agree on every wave's tables
    return res


def _sound(o, text, piece):
    """A stream that ended well: zlib's bytes, every piece inside the contract, the end reported once."""
    assert o["rc"] == 0 and o["error"] is None
    assert b"".join(o["pieces"]) == text
    assert all(1 <= len(p) <= piece + 65536 for p in o["pieces"])
    assert [c["piece"] for c in o["calls"]].count(-1) == 1 and o["calls"][-1]["piece"] == -1


def test_pieces_of_a_member_decoded_in_waves(exe, tmp_path):
    text, m_text = pc.text(600_000), pc.marker_stream()[1]
    recs, names = [], []
    for level in (1, 6, 9):  # waves of two chunks of 32 KiB hold ~200 KB of text: three pieces, the boundaries inside a wave's text
        recs.append((32768, 2, 65536, 1, pc.gz(600_000, level)))
        names.append(f"l{level}")
    g = pc.gz(600_000, 6)
    for c in pc.edge_chunks(g):
        recs.append((c, 512, 65536, 1, g))
        names.append(f"edge_{c}")
    recs.append((32768, 2, 4096, 1, g))  # a piece smaller than one chunk's text (~110 KB)
    names.append("small_piece")
    recs.append((32768, 2, 4096, 1, pc.marker_stream()[0]))  # copies from 32 768 bytes back: from text handed out many pieces ago
    names.append("markers")
    recs.append((32768, 512, 1 << 30, 1, g))  # one wave, one piece
    names.append("one_piece")
    res = dict(zip(names, _run(exe, tmp_path, recs)))
    for name, o in res.items():
        piece = dict(zip(names, recs))[name][2]
        _sound(o, m_text if name == "markers" else text, piece)
        t = o["total"]
        assert (t["plain_parallel"], t["plain_host"], t["declined"], t["dropped"]) == (1, 0, 0, 0), (name, t)
        assert t["bytes_down"] == len(b"".join(o["pieces"])) and o["checked"] == t["waves"] >= 1, (name, t)
    for level in (1, 6, 9):
        o = res[f"l{level}"]
        assert o["total"]["waves"] >= 2 and o["calls"][0]["waves"] == 1 and o["calls"][0]["bytes_down"] > 2 * 65536, o["calls"][0]
        assert len(o["pieces"][0]) == 65536 and o["calls"][1]["waves"] == 0  # cut from the first wave's text; the second piece without a wave
    assert res["small_piece"]["total"]["waves"] >= 4 and all(len(p) == 4096 for p in res["small_piece"]["pieces"][:20])
    assert res["markers"]["total"]["waves"] == 2 and res["markers"]["total"]["chunks"] == 3
    assert len(res["one_piece"]["pieces"]) == 1
    # a piece that ends exactly where the first wave's text ends: the piece is that text, and the next call runs the next wave
    first = res["l6"]["calls"][0]["bytes_down"]
    (o,) = _run(exe, tmp_path, [(32768, 2, first, 1, pc.gz(600_000, 6))])
    _sound(o, text, first)
    assert len(o["pieces"][0]) == first and o["calls"][0]["waves"] == 1 and o["calls"][1]["waves"] >= 1, o["calls"][:2]


@pytest.mark.parametrize("case", ["late_fixed", "late_stored"])
def test_a_decline_in_a_later_wave_resumes_on_the_host(exe, tmp_path, case):
    raw, text = getattr(sc, case)()
    assert zlib.decompress(raw, 31) == text
    # (a wave has a piece's worth of input, and only a wave of more than four chunks can decline this way: pieces from 5 chunks'
    # input on.  Pieces and waves of many sizes: what is left of the waves' text when the host goes on, and so where its bytes land
    # in the stream's buffer and when the buffer has to move its text, differs with each)
    grid = [(wave, piece) for wave in (6, 8, 16) for piece in (262144, 270_000, 300_000, 400_000, 524288, 600_000, 800_000, 1 << 20)]
    res = _run(exe, tmp_path, [(32768, wave, piece, 1, raw) for wave, piece in grid])
    for o, (wave, piece) in zip(res, grid):
        _sound(o, text, piece)  # (the CRC32 and ISIZE of the trailer were checked against the register the resume started from)
        t = o["total"]
        assert (t["plain_parallel"], t["plain_host"], t["declined"]) == (0, 1, 1), (case, piece, t)
        assert t["waves"] >= 2 and t["chunks"] >= 4, (case, piece, t)
        k = next(i for i, c in enumerate(o["calls"]) if c["declined"])
        assert o["calls"][k]["last_decline"] == NO_BOUNDARY
        assert sum(c["chunks"] for c in o["calls"][:k + 1]) == t["chunks"] and all(c["waves"] == 0 for c in o["calls"][k + 1:])
        assert sum(c["plain_host"] for c in o["calls"][-2:]) == 1  # counted where the member's trailer was checked


def test_members_behind_the_member(exe, tmp_path):
    raw, text = sc.members()
    pieces = (65536, 100_000, 300_000, 1 << 20)  # (the small member behind the two large ones is the host's, behind text cut from a wave)
    for o, piece in zip(_run(exe, tmp_path, [(32768, 4, p, 1, raw) for p in pieces]), pieces):
        _sound(o, text, piece)
        t = o["total"]
        assert (t["plain_parallel"], t["plain_host"], t["declined"]) == (2, 1, 0) and t["bgzf_members"] == 150_000 // 65280 + 1 + 1, t
    raw, text, n_bgzf = sc.mixed()
    (o,) = _run(exe, tmp_path, [(65536, 4, 65536, 1, raw)])
    _sound(o, text, 65536)
    assert (o["total"]["plain_parallel"], o["total"]["bgzf_members"]) == (1, n_bgzf)


def test_damage_is_reported_where_the_host_path_reports_it(exe, tmp_path):
    cases = sc.damaged()
    names = sorted(cases)
    dev = _run(exe, tmp_path, [(32768, 4, 65536, 1, cases[n][0]) for n in names])
    host = _run(exe, tmp_path, [(32768, 4, 65536, 0, cases[n][0]) for n in names])
    for name, d, h in zip(names, dev, host):
        raw, k, at = cases[name]
        assert sc.zlib_refuses(raw), name
        with pytest.raises(capi.LambdaExtError) as whole:
            capi.gunzip(None, raw)
        assert d["rc"] == capi.LX_EINVAL and "lambda_ext error -1: " + d["error"] == str(whole.value) and d["error"] == h["error"], (name, d["error"], str(whole.value))
        assert d["error"].startswith(f"lx_gunzip: member {k} at byte {at}: "), (name, d["error"])
        assert d["ncalls"] == h["ncalls"] >= 2, (name, d["ncalls"], h["ncalls"])  # the same call, and not the first
        good, same = b"".join(d["pieces"]), b"".join(h["pieces"])  # (behind the damage both may hand out what the damaged bits decode to)
        assert good[:len(same)] == same[:len(good)] and d["pieces"][0] == (pc.text(600_000) if k else pc.text(1_000_000))[:65536], name
        assert d["total"]["chunks"] > 0 and d["total"]["plain_parallel"] == k, (name, d["total"])
