"""The DEFLATE decoder (lambda_amd/csrc/lx_inflate.h) on streams built on purpose (tests/deflate_craft.py), without a GPU.

zlib is the reference throughout: every VALID case is first held against `zlib.decompress(raw, -15)`, and the differential run
asks zlib for its verdict on 35 of its own streams and 30 000 copies with one or two flipped bits.  The host path
(`capi.gunzip(None, ...)`) runs Inflater<HostSink, uint64_t>; the kernel's own instantiation, Inflater<LdsSink, uint32_t>, runs in
tests/native/inflate_check.cpp under AddressSanitizer and UBSan with every input and output in a heap block of its exact size."""
import struct
import subprocess
import zlib
from collections import Counter
from pathlib import Path

import pytest

from lambda_amd import build, capi
from tests import deflate_craft as dc

ROOT = Path(__file__).resolve().parent.parent
GOOD = dc.bgzf_member(zlib.compress(b">good\nACGT\n", 6)[2:-4], b">good\nACGT\n")

VALID_NAMES = [v.name for v in dc.valid_cases()]
INVALID_NAMES = [c.name for c in dc.invalid_cases()]


def test_corpora_hold_what_they_say():
    """The writer against zlib and against itself, before anything of the project runs."""
    for v in dc.valid_cases():
        assert zlib.decompress(v.raw, -15) == v.data, v.name
        d = zlib.decompressobj(-15)
        d.decompress(v.raw)
        assert d.eof and d.unused_data == b"", v.name  # (the stream is all of raw: no spare byte)
        assert len(dc.bgzf_member(v.raw, v.data)) <= 65536
    by = {v.name: v for v in dc.valid_cases()}
    assert len(by) == len(VALID_NAMES) and len(set(INVALID_NAMES)) == len(INVALID_NAMES)
    assert len(by["stored_len65505"].raw) == 65510 and len(dc.bgzf_member(*by["stored_len65505"][1:])) == 65536
    assert len(by["copy_258_ends_on_65536"].data) == 65536
    assert by["dynamic_end_of_block_only"].data == b"" and len(by["dynamic_end_of_block_only"].raw) == 139
    # the codes the cases rely on: complete where they are meant to be, and as long as they are meant to be
    assert dc.canonical(dc.STAIRS)[1] == 1 and dc.canonical(dc.DEFAULT_CL)[1] == 1 and max(dc.STAIRS) == 15
    assert dc.canonical(dc.FIXED_LIT)[1] == 1 and dc.canonical(dc.FIXED_DIST)[1] == 1
    assert dc.canonical([0] * 256 + [1])[1] == dc.canonical([1])[1] == dc.Fraction(1, 2)
    groups = Counter(c.group for c in dc.invalid_cases())
    assert set(groups) == set("abcdefgh"), groups
    for c in dc.invalid_cases():
        assert len(c.texts) == 1 or (c.group == "b" and len(c.texts) == 2), c.name
        assert len(c.member()) <= 65536 and c.isize <= 65536
        refused = not dc.zlib_verdict(c.raw)[0]
        assert refused == c.zlib_refuses, c.name
        if not c.zlib_refuses:  # the stream is good: what is wrong is the wrapper around it
            assert c.group in "gh" and zlib.decompress(c.raw, -15) == c.data
    # every status of the decoder and of the kernel's wrapper checks has a case
    said = {t for c in dc.invalid_cases() if len(c.texts) == 1 for t in c.texts}
    assert said == set(dc.STATUS_TEXTS[1:]) | {dc.W_ISIZE, dc.W_TRAILING, dc.W_CRC}


@pytest.mark.parametrize("name", VALID_NAMES)
def test_host_decodes_valid_case(name):
    v = next(v for v in dc.valid_cases() if v.name == name)
    assert capi.gunzip(None, dc.bgzf_member(v.raw, v.data)) == v.data
    assert capi.gunzip(None, dc.plain_member(v.raw, v.data)) == v.data
    # between two other members, and with a name and further subfields in the header
    deco = {} if len(v.raw) > 65000 else dict(extra_before=b"XY\x01\x00z", extra_after=b"AB\x00\x00", fname=b"case")  # (no room in the largest)
    m = dc.bgzf_member(v.raw, v.data, **deco)
    assert capi.gunzip(None, GOOD + m + dc.plain_member(v.raw, v.data) + GOOD) == b">good\nACGT\n" + v.data * 2 + b">good\nACGT\n"


def _refused(stream, member, what):
    with pytest.raises(capi.LambdaExtError) as e:
        capi.gunzip(None, stream)
    assert e.value.code == capi.LX_EINVAL and f"lx_gunzip: member {member} " in str(e.value), (what, str(e.value))
    return str(e.value)


@pytest.mark.parametrize("name", INVALID_NAMES)
def test_host_refuses_invalid_case(name):
    c = next(c for c in dc.invalid_cases() if c.name == name)
    _refused(GOOD + c.member() + GOOD, 1, name)
    _refused(GOOD + dc.plain_member(c.raw, c.data, c.isize, c.crc) + GOOD, 1, name)
    _refused(c.member(), 0, name)
    if c.zlib_refuses:
        # with nothing behind the stream the host path gives the decoder's own status (the device gives it always: it knows the
        # stream's length from BSIZE).  One text per case; the truncation group may read missing bits as a code that is none.
        msg = _refused(dc.plain_member(c.raw, b"")[:-8], 0, name)
        assert any(msg.endswith(": " + t) for t in c.texts), (name, msg)
        with pytest.raises(zlib.error):
            zlib.decompress(c.raw, -15)


def test_differential_against_zlib_on_flipped_bits():
    """35 zlib streams (five inputs, seven level / strategy settings, a full flush in the middle) and 30 000 mutants of one or two
    flipped bits.  What zlib accepts must decode to zlib's bytes from exactly the bytes zlib consumed; what zlib refuses must be
    refused, whatever trailer follows and also when nothing follows, and then with one of the decoder's seven stream statuses."""
    M = dc.mutants()
    assert len(M) == 35 + dc.N_MUTANTS
    accepted = refused = 0
    texts = Counter()
    for i, m in enumerate(M):
        if m.accepted:
            accepted += 1
            raw = m.raw[:m.consumed]
            assert capi.gunzip(None, dc.plain_member(raw, m.data)) == m.data, i
            if i % 16 == 0:
                assert capi.gunzip(None, GOOD + dc.bgzf_member(raw, m.data) + GOOD) == b">good\nACGT\n" + m.data + b">good\nACGT\n", i
        else:
            refused += 1
            with pytest.raises(capi.LambdaExtError):
                capi.gunzip(None, dc.plain_member(m.raw, b"", isize=m.true_len, crc=i))
            with pytest.raises(capi.LambdaExtError) as e:
                capi.gunzip(None, dc.plain_member(m.raw, b"")[:-8])
            text = str(e.value).rsplit(": ", 1)[-1]
            assert text in dc.STATUS_TEXTS[1:8], (i, str(e.value))  # ("truncated gzip trailer" would mean: the stream was accepted)
            texts[text] += 1
    counts = f"accepted {accepted}, refused {refused} of {len(M)}; " + ", ".join(f"{t}: {texts[t]}" for t in dc.STATUS_TEXTS[1:8])
    assert accepted >= 0.2 * len(M) and refused >= 0.2 * len(M), counts
    assert all(texts[t] >= 50 for t in dc.STATUS_TEXTS[1:8]), counts


# ---- the kernel's instantiation under the sanitizers

def _records():
    """(input, capacity, expectation) per record of the stand-alone program's corpus.  The expectation: ("ok", bytes), or a set of
    statuses; 1..8 are lx::inflate::Status, 101 = fewer bytes than the capacity, 102 = the stream ends before the input does."""
    R = []
    inside = set(range(1, 9))  # refused inside the stream: whichever of its checks comes first at this capacity
    for v in dc.valid_cases():
        n = len(v.data)
        R.append((v.raw, n, ("ok", v.data)))
        if n:
            R.append((v.raw, n - 1, {8}))
        if n < 65536:
            R.append((v.raw, n + 1, {101}))
    for c in dc.invalid_cases():
        n = len(c.data)
        caps = sorted({0, 1, 100, n, max(n - 1, 0), 65536})
        if c.group in "abcdef":
            for cap in caps:
                R.append((c.raw, cap, inside))
            R.append((c.raw, c.isize, {dc.STATUS_TEXTS.index(t) for t in c.texts}))
        elif c.group == "g":  # a good stream of n bytes: the capacity alone decides
            for cap in caps:
                R.append((c.raw, cap, {8} if cap < n else {101} if cap > n else ("ok", c.data)))
            R.append((c.raw, c.isize, {8}))
        else:
            R.append((c.raw, c.isize, {dc.W_ISIZE: {101}, dc.W_TRAILING: {102}, dc.W_CRC: ("ok", c.data)}[c.texts[0]]))
    for m in dc.mutants():
        if m.accepted:
            n = len(m.data)
            R.append((m.raw[:m.consumed], n, ("ok", m.data)))
            if n:
                R.append((m.raw[:m.consumed], n - 1, {8}))
            if m.consumed < len(m.raw):
                R.append((m.raw, n, {102}))
        else:
            for cap in sorted({0, 1, 100, m.true_len, m.true_len - 1, 65536}):
                R.append((m.raw, cap, inside))
    return R


def _build_check(tmp_path):
    rocm_include = Path(build._hipcc()).resolve().parent.parent / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        rocm_include = Path("/opt/rocm/include")
    exe = tmp_path / "inflate_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           f"-I{rocm_include}", f"-I{ROOT / 'lambda_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "inflate_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_kernel_instantiation_clean_under_sanitizers(tmp_path):
    """Inflater<LdsSink, uint32_t> -- the very code the kernel's deciding lane runs -- on the crafted cases and the mutants, in
    exact-size heap blocks: a clean exit under AddressSanitizer and UBSan, the statuses the corpora state, and zlib's bytes."""
    R = _records()
    corpus = tmp_path / "corpus.bin"
    with open(corpus, "wb") as f:
        f.write(b"LXIC" + struct.pack("<I", len(R)))
        for raw, cap, _ in R:
            f.write(struct.pack("<II", len(raw), cap) + raw)
    exe = _build_check(tmp_path)
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(R)
    for i, (line, (raw, cap, want)) in enumerate(zip(lines, R)):
        idx, st, used, pos, crc = line.split()
        assert int(idx) == i and int(pos) <= cap
        if isinstance(want, tuple):
            assert (int(st), int(used), int(pos), int(crc, 16)) == (0, len(raw), len(want[1]), zlib.crc32(want[1])), (i, line, cap)
        else:
            assert int(st) in want, (i, line, cap, sorted(want))
