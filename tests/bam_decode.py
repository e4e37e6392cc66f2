"""A small BAM reader for the tests (SAM/BAM specification 4.2): the uncompressed stream back to SAM text lines."""
import struct

TAG_TYPES = {"ae": "f", "AS": "S", "ap": "S", "ar": "C", "ai": "C", "qf": "c", "sf": "c", "lt": "I", "NM": "I", "IH": "I",
             "st": "Z", "ls": "Z", "qs": "Z", "OC": "Z"}
_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def decode(bam: bytes):
    """(header text, [(name, length)], [record dict]) of an uncompressed BAM stream."""
    assert bam[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", bam, 4)
    text = bam[8:8 + l_text].decode()
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", bam, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", bam, p)
        name = bam[p + 4:p + 4 + ln - 1].decode()
        (lr,) = struct.unpack_from("<i", bam, p + 4 + ln)
        refs.append((name, lr))
        p += 8 + ln
    recs = []
    while p < len(bam):
        (bs,) = struct.unpack_from("<i", bam, p)
        end = p + 4 + bs
        ref_id, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", bam, p + 4)
        q = p + 36
        name = bam[q:q + l_name - 1].decode()
        q += l_name
        cig = struct.unpack_from(f"<{n_cig}I", bam, q)
        q += 4 * n_cig
        seq = "".join("=ACMGRSVTWYHKDBN"[(bam[q + i // 2] >> (4 * (1 - i % 2))) & 15] for i in range(l_seq))
        q += (l_seq + 1) // 2
        qual = bam[q:q + l_seq]
        q += l_seq
        tags = []
        while q < end:
            key, t = bam[q:q + 2].decode(), chr(bam[q + 2])
            q += 3
            if t == "Z":
                z = bam.index(b"\0", q)
                tags.append((key, t, bam[q:z].decode()))
                q = z + 1
            elif t == "f":
                tags.append((key, t, struct.unpack_from("<f", bam, q)[0]))
                q += 4
            else:
                fmt = _INT[t]
                tags.append((key, t, struct.unpack_from(fmt, bam, q)[0]))
                q += struct.calcsize(fmt)
        assert q == end
        recs.append(dict(ref_id=ref_id, pos=pos, name=name, mapq=mapq, bin=bin_, cigar=cig, flag=flag, l_seq=l_seq, seq=seq, qual=qual,
                         next=(nref, npos, tlen), tags=tags))
        p = end
    return text, refs, recs


def span(cigar) -> int:
    return sum(c >> 4 for c in cigar if (c & 15) in (0, 2, 3, 7, 8))


def to_sam(bam: bytes) -> list[str]:
    """The SAM lines (header lines first) a BAM stream stands for, as this project's SAM writer prints them."""
    text, refs, recs = decode(bam)
    lines = text.splitlines()
    for r in recs:
        cig = "".join(f"{c >> 4}{'MIDNSHP=X'[c & 15]}" for c in r["cigar"]) or "*"
        seq = r["seq"] or "*"
        assert r["qual"] == b"\xff" * r["l_seq"]
        f = [r["name"], str(r["flag"]), refs[r["ref_id"]][0], str(r["pos"] + 1), str(r["mapq"]), cig, "*", "0", "0", seq, "*"]
        for key, t, v in r["tags"]:
            f.append(f"{key}:f:{v:g}" if t == "f" else f"{key}:Z:{v}" if t == "Z" else f"{key}:i:{v}")
        lines.append("\t".join(f))
    return lines
