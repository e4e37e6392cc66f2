"""The FASTQ qualities of the front end's incremental parser (lambda_amd/csrc/host/lx_query_blocks.hpp, keepQualities), without a
GPU and without the library: tests/native/fastq_qual_check.cpp, built with g++ under AddressSanitizer and UBSan, parses every text
below whole and in pieces of 1, 2, 3 and 7 bytes, with the qualities kept and with them dropped, and fails if two of those parses
differ.  This file states the texts and what both parses must give."""
import re
import struct
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

# name -> (text, [(id, letters, qualities)], end of the error text with the qualities kept or "")
ACCEPTED = {
    "plain": (b"@r1 x\nACGT\n+\nIIII\n@r2\nGG\n+r2\n#!\n", [("r1 x", "ACGT", "IIII"), ("r2", "GG", "#!")]),
    "multi_line": (b"@r1\nAC\nGT\n\nA C\n+\n@I\nI~\n+!\n\n@r2\nG\n+\nI\n", [("r1", "ACGTAC", "@II~+!"), ("r2", "G", "I")]),
    "quality_starts_with_at_plus_gt": (b"@r1\nACGT\n+\n@ABC\n@r2\nACGT\n+\n+DEF\n@r3\nACGT\n+\n>@+I\n@r4\nAC\n+\n@@\n",
                                       [("r1", "ACGT", "@ABC"), ("r2", "ACGT", "+DEF"), ("r3", "ACGT", ">@+I"), ("r4", "AC", "@@")]),
    "crlf": (b"@r1\r\nACGT\r\n+\r\nI!~J\r\n@r2\r\nGG\r\n+\r\n#!\r\n", [("r1", "ACGT", "I!~J"), ("r2", "GG", "#!")]),
    "crlf_multi_line": (b"@r1\r\nAC\r\nGT\r\n+\r\nI!\r\n~J\r\n", [("r1", "ACGT", "I!~J")]),
    "last_line_without_newline": (b"@r1\nACGT\n+\nIIII\n@r2\nGG\n+\n#!", [("r1", "ACGT", "IIII"), ("r2", "GG", "#!")]),
    "last_line_is_cr": (b"@r1\nACGT\n+\nABCD\r", [("r1", "ACGT", "ABCD")]),
    "empty_record": (b"@r1\n+\n@r2\nAC\n+\nI#\n@r3\n\n+\n\n@r4\nG\n+\n~\n", [("r1", "", ""), ("r2", "AC", "I#"), ("r3", "", ""), ("r4", "G", "~")]),
    "edges_of_the_range": (b"@r\nACGT\n+\n!~!~\n", [("r", "ACGT", "!~!~")]),
    "fasta": (b">a one\nACGT\nAC\n>b\nGG\n", [("a one", "ACGTAC", ""), ("b", "GG", "")]),
}
# name -> (text, records in front of the refused one, the refused record, the byte as the message prints it)
REFUSED = {
    "space": (b"@r1\nAC\n+\nII\n@r2\nACGT\n+\nI II\n", [("r1", "AC", "II")], "r2", "0x20"),
    "tab": (b"@r1\nACGT\n+\nII\tI\n", [], "r1", "0x09"),
    "del": (b"@r1\nAC\n+\nII\n@read two\nACGT\nAC\n+\nIIII\nI\x7f\n", [("r1", "AC", "II")], "read two", "0x7f"),
    "high_bit": (b"@r1\nACGT\n+\nII\xc3I\n", [], "r1", "0xc3"),
    "nul": (b"@r1\nACGT\n+\n\0III\n", [], "r1", "0x00"),
}
# what the parser gives for the refused texts when it drops the qualities: what it gave before it could keep them
REFUSED_WHEN_DROPPED = {
    "space": [("r1", "AC", ""), ("r2", "ACGT", "")],
    "tab": [("r1", "ACGT", "")],
    "del": [("r1", "AC", ""), ("read two", "ACGTAC", "")],
    "high_bit": [("r1", "ACGT", "")],
    "nul": [("r1", "ACGT", "")],
}


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fastq_qual")
    exe = tmp / "fastq_qual_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{ROOT / 'lambda_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "fastq_qual_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(texts):
        """Per text: {"K": (records, error), "D": (records, error)} -- the qualities kept, dropped."""
        corpus = tmp / "corpus.bin"
        corpus.write_bytes(b"LXQB" + struct.pack("<I", len(texts)) + b"".join(struct.pack("<I", len(t)) + t for t in texts))
        r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        plain = lambda s: re.sub(r"\\([0-9a-f]{2})", lambda m: chr(int(m[1], 16)), s)
        out, cur = [dict() for _ in texts], None
        for line in r.stdout.split("\n")[:-1]:
            if line.startswith("R "):
                cur[0].append(tuple(plain(f) for f in line[2:].split("|")))
            else:
                head, err = line.split(" E:", 1)
                idx, mode, n = head.split()
                cur = ([], plain(err), int(n))
                out[int(idx)][mode] = cur
        assert all(set(o) == {"K", "D"} and all(len(v[0]) == v[2] for v in o.values()) for o in out)
        return [{k: (v[0], v[1]) for k, v in o.items()} for o in out]

    return run


def test_kept_qualities_are_the_lines_as_they_stand(check):
    names = sorted(ACCEPTED)
    for name, got in zip(names, check([ACCEPTED[n][0] for n in names])):
        want = ACCEPTED[name][1]
        assert got["K"] == (want, ""), (name, got["K"])
        assert got["D"] == ([(i, l, "") for i, l, _ in want], ""), (name, got["D"])  # dropped: the same records, no qualities


def test_bytes_outside_the_range_are_refused_naming_the_record(check):
    names = sorted(REFUSED)
    for name, got in zip(names, check([REFUSED[n][0] for n in names])):
        _, front, rec, byte = REFUSED[name]
        recs, err = got["K"]
        assert recs == front, (name, recs)
        assert err.startswith("reads.fq: ") and f"FASTQ record '{rec}'" in err and byte in err, (name, err)
        assert got["D"] == (REFUSED_WHEN_DROPPED[name], ""), (name, got["D"])


def test_the_count_rule_and_its_messages_do_not_change(check):
    texts = [b"@r1\nAC\n+\nII\n@r2\nACGT\n+\nII\n", b"@r1\nACGT\n+\nII\nIII\n@r2\nA\n+\nI\n", b"@r1\nAC\n+\nII\n@r2\nACGT\nII\n", b"@r1\nAC\n+\nII\nACGT\n"]
    errors = ["reads.fq: FASTQ record 'r2' has 2 quality characters for 4 letters", "reads.fq: FASTQ record 'r1' has 5 quality characters for 4 letters",
              "reads.fq: FASTQ record 'r2' has no '+' line", "reads.fq: FASTQ record expected, found a line starting with 'A'"]
    for got, err in zip(check(texts), errors):
        assert got["K"][1] == err and got["D"][1] == err
        assert [r[:2] for r in got["K"][0]] == [r[:2] for r in got["D"][0]]
