"""The incremental FASTA / FASTQ parser of the front end (lambda_amd/csrc/host/lx_query_blocks.hpp), without a GPU and without
the library: tests/native/query_blocks_check.cpp, built with g++ under AddressSanitizer and UBSan, feeds it every input below in
pieces of 1, 2, 3, 7 and 4096 bytes, whole, and in pieces of changing size, and holds records and error texts against the
whole-text rules the front end had before (kept in that program as the yardstick).  This file states the inputs, and for the named
ones what the whole-text parse itself must give; and it asks the same program where BlockCutter closes its blocks."""
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

# name -> (text, records or None, end of the error text or "")
NAMED = {
    "empty": (b"", [], ""),
    "blanks_only": (b" \n\t\r\n  ", [], ""),
    "fasta_multi_line": (b">a one\nACGT\nAC\n>b\nGG\n", [("a one", "ACGTAC"), ("b", "GG")], ""),
    "fasta_crlf": (b">a one\r\nACGT\r\nAC\r\n>b\r\nGG\r\n", [("a one", "ACGTAC"), ("b", "GG")], ""),
    "fasta_blank_lines_and_blanks_inside": (b"\n\n>a\n\nAC GT\n\n \tA C\t\n\n>b\n\nG G\n\n", [("a", "ACGTAC"), ("b", "GG")], ""),
    "fasta_empty_sequence": (b">a\n>b\n\n>c\nAC\n>d", [("a", ""), ("b", ""), ("c", "AC"), ("d", "")], ""),
    "fasta_last_record_without_newline": (b">a\nAC\n>b\nGGT", [("a", "AC"), ("b", "GGT")], ""),
    "fasta_last_line_is_cr": (b">a\nAC\r", [("a", "AC")], ""),
    "fasta_text_in_front_of_the_first_record": (b"; a comment\nACGT\n>a\nAC\n", [("a", "AC")], ""),
    "fasta_blanks_in_front": (b"  \n \t\n>a\nAC\n", [("a", "AC")], ""),
    "fasta_empty_id_and_at_lines": (b">\nAC\n@x\n+\n>b x \nG\n", [("", "AC@x+"), ("b x ", "G")], ""),
    "fastq_plain": (b"@r1 x\nACGT\n+\nIIII\n@r2\nGG\n+r2\n#!\n", [("r1 x", "ACGT"), ("r2", "GG")], ""),
    "fastq_crlf_no_last_newline": (b"@r1\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nGG\r\n+\r\n#!", [("r1", "ACGT"), ("r2", "GG")], ""),
    "fastq_quality_starts_with_at_plus_gt": (b"@r1\nACGT\n+\n@III\n@r2\nACGT\n+\n+III\n@r3\nACGT\n+\n>@+I\n@r4\nAC\n+\n@@\n",
                                             [("r1", "ACGT"), ("r2", "ACGT"), ("r3", "ACGT"), ("r4", "AC")], ""),
    "fastq_multi_line": (b"@r1\nAC\nGT\n\nA C\n+\n@I\nII\n+@\n\n@r2\nG\n+\nI\n", [("r1", "ACGTAC"), ("r2", "G")], ""),
    "fastq_blank_lines_between_records": (b"\n@r1\nAC\n+\nII\n\n\r\n@r2\nG\n+\nI\n\n", [("r1", "AC"), ("r2", "G")], ""),
    "fastq_empty_sequence": (b"@r1\n+\n@r2\nAC\n+\nII\n@r3\n\n+\n", [("r1", ""), ("r2", "AC"), ("r3", "")], ""),
    "fastq_no_plus_line": (b"@r1\nAC\n+\nII\n@r2\nACGT\nII\n", [("r1", "AC")], "reads.fq: FASTQ record 'r2' has no '+' line"),
    "fastq_too_few_qualities": (b"@r1\nAC\n+\nII\n@r2\nACGT\n+\nII\n", [("r1", "AC")],
                                "reads.fq: FASTQ record 'r2' has 2 quality characters for 4 letters"),
    "fastq_too_many_qualities": (b"@r1\nACGT\n+\nII\nIII\n@r2\nA\n+\nI\n", [], "reads.fq: FASTQ record 'r1' has 5 quality characters for 4 letters"),
    "fastq_not_a_record": (b"@r1\nAC\n+\nII\nACGT\n", [("r1", "AC")], "reads.fq: FASTQ record expected, found a line starting with 'A'"),
    "fastq_blank_line_of_blanks_in_front": (b" \t\n\n@r1\nAC\n+\nII\n", [], "reads.fq: FASTQ record expected, found a line starting with ' '"),
    "fastq_blanks_in_front_of_the_at": (b"\n  @r1\nAC\n+\nII\n", [], "reads.fq: FASTQ record expected, found a line starting with ' '"),
    "fastq_header_only": (b"@r1", [], "reads.fq: FASTQ record 'r1' has no '+' line"),
    "nul_bytes": (b">a\0b\nA\0C\n", [("a\0b", "A\0C")], ""),
}


def _generated():
    """Texts put together at random from the line kinds of both formats, line ends "\\n", "\\r\\n" and none at the end: whatever they
    are, the two parses must agree."""
    rng = np.random.default_rng(7)
    lines = [b">id", b">", b"@id", b"@", b"+", b"+id", b"ACGT", b"AC GT", b"", b" ", b"\t", b"IIII", b"@III", b"+II>", b">II", b"\r", b"A", b"II"]
    out = []
    for _ in range(300):
        k = int(rng.integers(1, 14))
        first = [b">id", b"@id", b"", b" "][int(rng.integers(0, 4))]
        parts = [first] + [lines[int(i)] for i in rng.integers(0, len(lines), k)]
        eol = [b"\n", b"\r\n"][int(rng.integers(0, 2))]
        out.append(eol.join(parts) + (eol if rng.integers(0, 2) else b""))
    for t in range(200):  # well-formed FASTQ of multi-line records; every second text then loses one line
        parts = []
        for r in range(int(rng.integers(1, 6))):
            n, cut = int(rng.integers(0, 30)), int(rng.integers(0, 30))
            seq, qual = b"ACGTN" * n, rng.choice(list(b"@+>I#"), 5 * n).astype(np.uint8).tobytes()
            parts += [b"@r%d" % r, seq[:cut], seq[cut:], b"+", qual[:cut], qual[cut:]] + [b""] * int(rng.integers(0, 2))
        if t % 2:
            del parts[int(rng.integers(0, len(parts)))]
        eol = [b"\n", b"\r\n"][int(rng.integers(0, 2))]
        out.append(eol.join(parts) + (eol if rng.integers(0, 2) else b""))
    long_fa = b"".join(b">read%d\n%s\n" % (i, b"ACGT" * int(rng.integers(0, 40))) for i in range(400))  # lines across 4096-byte pieces
    long_fq = b"".join(b"@read%d\n%s\n+\n%s\n" % (i, b"ACGT" * int(n), b"@+>I" * int(n)) for i, n in enumerate(rng.integers(0, 40, 400)))
    return out + [long_fa, long_fq]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("query_blocks")
    exe = tmp / "query_blocks_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{ROOT / 'lambda_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "query_blocks_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(texts):
        corpus = tmp / "corpus.bin"
        corpus.write_bytes(b"LXQB" + struct.pack("<I", len(texts)) + b"".join(struct.pack("<I", len(t)) + t for t in texts))
        r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        out, cur = [], None
        plain = lambda s: re.sub(r"\\([0-9a-f]{2})", lambda m: chr(int(m[1], 16)), s)
        for line in r.stdout.split("\n")[:-1]:
            if line.startswith("R "):
                cur[2].append(tuple(plain(f) for f in line[2:].split("|")))
            else:
                head, err = line.split(" E:", 1)
                idx, n, letters = map(int, head.split())
                cur = (n, letters, [], plain(err))
                out.append(cur)
                assert idx == len(out) - 1
        assert len(out) == len(texts) and all(n == len(recs) for n, _, recs, _ in out)
        return out

    run.exe = exe
    return run


def test_pieces_give_the_records_and_errors_of_the_whole_text(check):
    names = sorted(NAMED)
    got = check([NAMED[n][0] for n in names])
    for name, (n, letters, recs, err) in zip(names, got):
        _, want, want_err = NAMED[name]
        assert recs == [tuple(w) for w in want] and err == want_err, (name, recs, err)
        assert letters == sum(len(r[1]) for r in recs), name


def test_generated_texts_agree(check):
    texts = _generated()
    got = check(texts)
    # the corpus reaches both formats, both outcomes, and records that cross the 4096-byte pieces
    assert sum(1 for g in got if g[3]) >= 30 and sum(1 for g in got if not g[3] and g[0] >= 2) >= 30
    assert sum(1 for t, g in zip(texts, got) if t.lstrip(b" \t\r\n")[:1] == b"@" and not g[3] and g[0]) >= 10
    assert got[-2][0] == 400 and got[-1][0] == 400 and not got[-1][3]


def test_the_cutter_closes_at_exactly_n_reads_and_at_the_letter_cap(check):
    n = 9
    lens = ["150"] * n
    cutter = lambda reads, letters, ls: subprocess.run([str(check.exe), "cutter", str(reads), str(letters), *ls], capture_output=True, text=True, timeout=60)
    for reads, want in ((1, "1 " * 9 + "open 0"), (2, "2 2 2 2 open 1"), (n - 1, "8 open 1"), (n, "9 open 0"), (n + 1, "open 9")):
        r = cutter(reads, 1 << 30, lens)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.strip() == want, (reads, r.stdout, r.stderr)
    # the letter cap: a block closes behind the read with which it holds `cap` letters or more, whatever the read count allows
    for cap, ls, want in ((450, lens, "3 3 3 open 0"), (451, lens, "4 4 open 1"), (1, ["0", "0", "5", "0"], "3 open 1"), (1 << 30, [str(1 << 30), "7"], "1 open 1"),
                          (1 << 30, [str((1 << 30) - 1), "0", "1", "2"], "3 open 1"), (300, ["150"] * 5, "2 2 open 1")):
        r = cutter(1 << 20, cap, ls)
        assert r.returncode == 0 and r.stdout.strip() == want, (cap, ls, r.stdout)
    r = cutter(2, 450, lens)  # whichever comes first
    assert r.stdout.strip() == "2 2 2 2 open 1"
    r = cutter(5, 450, lens)
    assert r.stdout.strip() == "3 3 3 open 0"
