"""The parallel decode of a plain gzip member (lambda_amd/csrc/lx_pgunzip.h) without a GPU: tests/native/pgunzip_check.cpp runs
the header's find / decode / chain / resolve chunk by chunk under AddressSanitizer and UBSan, every buffer a heap block of its
exact size.  zlib says what every stream decodes to, where its final block ends, and which streams are refused."""
import subprocess
import zlib
from pathlib import Path

import pytest

from lambda_amd import build
from tests import pgunzip_cases as pc

ROOT = Path(__file__).resolve().parent.parent
DECODED, NO_BOUNDARY, ROOM, STATUS, CHAIN = 0, 1, 2, 3, 4  # (LX_GUNZIP_DECLINE_*)


def _cases():
    """(name, chunk, wave, stream, data or None when zlib refuses the stream, reasons the program may give, extra check)."""
    C = []
    for level in (1, 6, 9):
        C.append((f"text600k_l{level}", 65536, 512, pc.gz(600_000, level), pc.text(600_000), {DECODED}, lambda o: o["chunks"] >= 4 and o["dropped"] == 0))
    g = pc.gz(600_000, 6)
    for c in pc.edge_chunks(g):
        C.append((f"edge_{c}", c, 512, g, pc.text(600_000), {DECODED}, lambda o: o["dropped"] == 0))
    C.append(("two_waves", 32768, 4, g, pc.text(600_000), {DECODED}, lambda o: o["waves"] >= 2 and o["chunks"] >= 8))
    m, data = pc.marker_stream()
    C.append(("markers", 32768, 512, m, data, {DECODED}, lambda o: o["chunks"] == 3 and o["markers"] >= 5 * 258))
    C.append(("markers_two_waves", 32768, 2, m, data, {DECODED}, lambda o: o["waves"] == 2))
    C.append(("full_flush", 65536, 512, *pc.flushed(), {DECODED}, lambda o: o["chunks"] >= 4))
    C.append(("fixed_only", 65536, 512, *pc.fixed_only(), {NO_BOUNDARY}, None))
    C.append(("random_stored", 65536, 512, *pc.random_stored(), {DECODED, NO_BOUNDARY}, None))
    C.append(("false_positives", 65536, 512, *pc.false_positives(), {DECODED, NO_BOUNDARY, CHAIN}, lambda o: o["reason"] or o["dropped"] > 0))
    C.append(("false_positives_behind_text", 65536, 512, *pc.false_positives_behind_text(), {DECODED, CHAIN}, lambda o: o["reason"] or o["dropped"] > 0))
    C.append(("zeros", 65536, 512, *pc.zeros(), {DECODED, ROOM}, None))
    for name, bad in pc.corrupt(pc.gz(1_000_000, 6)):
        refused_inside = name in ("flip", "cut")  # (a wrong trailer is the caller's to see: the program reports the CRC it took)
        # (a damaged stream may also decode, to other bytes: then the CRC32 must give it away)
        C.append((f"corrupt_{name}", 65536, 512, bad, None if refused_inside else pc.text(1_000_000), {STATUS, DECODED} if refused_inside else {DECODED}, None))
    return C


def _build_check(tmp_path):
    rocm_include = Path(build._hipcc()).resolve().parent.parent / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        rocm_include = Path("/opt/rocm/include")
    exe = tmp_path / "pgunzip_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           f"-I{rocm_include}", f"-I{ROOT / 'lambda_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "pgunzip_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_parallel_decode_on_the_cpu_matches_zlib(tmp_path):
    cases = _cases()
    for name, _, _, stream, data, _, _ in cases:  # zlib's verdicts first
        if data is None or name.startswith("corrupt_"):
            assert pc.zlib_refuses(stream), name
        else:
            assert zlib.decompress(stream, 31) == data, name
    corpus, out = tmp_path / "corpus.bin", tmp_path / "bytes.bin"
    corpus.write_bytes(pc.pack_corpus([(c, w, s[pc.HEADER:]) for _, c, w, s, _, _, _ in cases]))
    exe = _build_check(tmp_path)
    r = subprocess.run([str(exe), str(corpus), str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    got, at = out.read_bytes(), 0
    for i, (line, (name, chunk, wave, stream, data, reasons, extra)) in enumerate(zip(lines, cases)):
        f = line.split()
        o = dict(zip(("reason", "consumed", "out_len", "crc", "chunks", "dropped", "waves", "markers"), [int(f[1]), int(f[2]), int(f[3]), int(f[4], 16)] + [int(x) for x in f[5:]]))
        print(name, o)
        assert int(f[0]) == i and o["reason"] in reasons, (name, line)
        if o["reason"] == DECODED and data is None:
            at += o["out_len"]
            assert o["crc"] != int.from_bytes(pc.gz(1_000_000, 6)[-8:-4], "little"), (name, line)
        elif o["reason"] == DECODED:
            mine = got[at:at + o["out_len"]]
            at += o["out_len"]
            assert mine == data, name
            assert o["crc"] == zlib.crc32(data) and o["consumed"] == pc.deflate_len(stream), (name, line)
        if extra is not None:
            assert extra(o), (name, line)
    assert at == len(got)
