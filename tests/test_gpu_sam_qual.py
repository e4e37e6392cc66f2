"""FASTQ base qualities in SAM and BAM records made on the device (lx_text.hip, lx_bam.hip; lx_output_options::q_qual,
lx_out_append_ex, --sam-bam-qual).  Every comparison is device bytes == host bytes; the host writer is pinned by the model of
tests/test_sam_qual.py, which is applied here once more to the lists this file builds and to the front end's output."""
import gzip
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests.bam_decode import decode
from tests.test_bam_encoding import ALL_TAGS, PROGRAMS, _case, _options
from tests.test_sam_qual import COMBOS, _append_pieces, check_against_model, group_starts, qual_bytes, records_of, render

pytestmark = pytest.mark.gpu

SAM, BAM = capi.LX_OUT_SAM, capi.LX_OUT_BAM
SCAN_TILE = 2048
MIN_RANGE = 128 << 10
DEV, HOST = capi.LX_RENDER_DEV, capi.LX_RENDER_HOST


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


def _args(m, ops, names):
    return (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"])


def dev_sam(h, program, m, ops, names, qa, qoff, opt, qq, header=True):
    return h.render_text(SAM, *_args(m, ops, names), program=program, write_header=header, q_ascii=qa, q_ascii_off=qoff, options=opt, q_qual=qq)


def dev_bam(h, program, m, ops, names, qa, qoff, opt, qq, header=True):
    return h.render_bam(*_args(m, ops, names), program=program, write_header=header, q_ascii=qa, q_ascii_off=qoff, options=opt, q_qual=qq)


def same(h, program, m, ops, names, qa, qoff, opt, qq):
    """Both device writers against the host writer; the host's SAM and BAM."""
    sam = render(SAM, program, m, ops, names, qa, qoff, opt, qq)
    got = dev_sam(h, program, m, ops, names, qa, qoff, opt, qq)
    assert got.split(b"\n") == sam.split(b"\n")  # (text: the first line that differs reads better than two blobs)
    assert got == sam
    bam = render(BAM, program, m, ops, names, qa, qoff, opt, qq)
    got = dev_bam(h, program, m, ops, names, qa, qoff, opt, qq)
    assert len(got) == len(bam) and decode(got)[2] == decode(bam)[2]
    assert got == bam
    return sam, bam


# ---- 1. every program, option combination and tag set

@pytest.mark.parametrize("tags", [ALL_TAGS, None], ids=["all", "default"])
@pytest.mark.parametrize("seq,hard,tree", COMBOS)
@pytest.mark.parametrize("program", PROGRAMS)
def test_device_writers_equal_the_host_writer(handle, program, seq, hard, tree, tags):
    m, ops, names, qa, qoff = _case(program, seed=PROGRAMS.index(program) * 7 + seq)
    opt, keep = _options(program, tags, seq, hard, tree, m, len(names["s_ids"]))
    qq = qual_bytes(len(qa))
    sam, bam = same(handle, program, m, ops, names, qa, qoff, opt, qq)
    carried = program in ("blastn", "blastx", "tblastx") and seq != capi.LX_SAM_SEQ_NEVER
    assert (sam != render(SAM, program, m, ops, names, qa, qoff, opt)) == carried  # (the qualities are in the bytes compared)
    assert (bam != render(BAM, program, m, ops, names, qa, qoff, opt)) == carried
    # without them the device writers make the bytes they made before
    assert dev_sam(handle, program, m, ops, names, qa, qoff, opt, None) == render(SAM, program, m, ops, names, qa, qoff, opt)
    assert dev_bam(handle, program, m, ops, names, qa, qoff, opt, None) == render(BAM, program, m, ops, names, qa, qoff, opt)


# ---- 2. the smallest shapes where the new code can go wrong

def _rows(q_lens, specs, ns=3):
    """Records (n_qid, frame, q_start, q_end) over reads of the given lengths: ops of one M run, everything else plain."""
    rng = np.random.default_rng(17)
    qa = "".join("ACGT"[i] for i in rng.integers(0, 4, int(sum(q_lens)))).encode()
    qoff = np.concatenate([[0], np.cumsum(q_lens)[:-1]]).astype(np.uint64)
    ops, recs = b"", []
    for q, frame, a, e in specs:
        o = b"M" * (e - a)
        r = np.zeros(1, dtype=capi.BLAST_MATCH_DTYPE)[0]
        r["n_qid"], r["qry_id"], r["n_sid"], r["subj_id"] = q, q, q % ns, 0
        r["q_start"], r["q_end"], r["s_start"], r["s_end"] = a, e, 5 + q, 5 + q + (e - a)
        r["bit_score"], r["score"], r["e_value"], r["identity"] = 50.5, 40, 1e-5, 90.0
        r["alignment_length"], r["num_matches"], r["num_positives"] = len(o), len(o), len(o)
        r["ops_off"], r["n_ops"], r["q_frame"], r["s_frame"] = len(ops), len(o), frame, 0
        ops += o
        recs.append(r)
    names = dict(q_ids=[f"read{i} x" for i in range(len(q_lens))], q_lens=np.asarray(q_lens, dtype=np.uint64),
                 s_ids=[f"s{j} subject" for j in range(ns)], s_lens=np.full(ns, 5000))
    return np.array(recs, dtype=capi.BLAST_MATCH_DTYPE), ops, names, qa, qoff


def _shapes(program, hard):
    """(list, the l_seq values it must show).  BLASTN: 0, 1, 2, 3 (BAM's last nibble next to the first quality byte), 63, 64, 65 (the
    emit loops' stride of one wavefront) and 129.  A translated query's SEQ has three letters per residue, so of those BLASTX can show
    0, 3, 63 and 129; 66 and 132 stand in for the others.  Both strands throughout.  The first read's window starts at byte 0 of the
    quality buffer, the last read's ends at its last byte (on the plus strand, and read backwards on the minus strand).  Behind
    them two reads for --sam-bam-seq uniq: three records of one frame and range (the second and third suppressed), and the next
    group's first record with the same frame and range (written)."""
    if program == "blastn":
        want = [0, 1, 2, 3, 63, 64, 65, 129]
        if hard:
            lens = [140] * 10
            specs = [(0, 1, 0, 64), (0, -1, 70, 140)]  # (the minus strand's last letters are the read's first: both windows start at byte 0)
            for q, l in enumerate(want, 1):
                specs += [(q, 1, q % 5, q % 5 + l), (q, -1, 3, 3 + l)]
            specs += [(9, 1, 75, 140), (9, -1, 0, 65)]  # both windows end at the buffer's last byte
        else:
            lens = [1, 2, 3, 63, 64, 65, 129]
            specs = [(q, f, 0, n) for q, n in enumerate(lens) for f in (1, -1)]
        uniq = (1, 2, 9)
    else:
        want = [0, 3, 63, 66, 129, 132]
        if hard:
            lens = [150] * 8
            specs = [(0, 1, 0, 21), (0, -1, 28, 50)]  # nucleotides [0, 63) on the plus strand; [150 - 150, 150 - 84) read backwards
            for q, residues in enumerate((0, 1, 21, 22, 43, 44), 1):
                f = (1, 2, 3)[q % 3]
                specs += [(q, f, q % 4, q % 4 + residues), (q, -f, 2, 2 + residues)]
            specs += [(7, 1, 29, 50), (7, -1, 0, 22)]  # both windows end at the buffer's last byte
        else:
            lens = [3, 2, 5, 63, 65, 68, 129, 132]  # frames 1, 1, 3, 1, 3, 3, 1, 1: 1, 0, 1, 21, 21, 22, 43, 44 residues
            frames = [1, 1, 3, 1, 3, 3, 1, 1]
            specs = [(q, s * f, 0, (n - (f - 1)) // 3) for q, (n, f) in enumerate(zip(lens, frames)) for s in (1, -1)]
        uniq = (2, 3, 20)
    q = len(lens)
    lens = lens + [150, 150]
    # (the last record of all: the minus strand from the read's last letter on, so that a window ends at the buffer's last byte)
    specs += [(q, uniq[0], uniq[1], uniq[2])] * 3 + [(q + 1, uniq[0], uniq[1], uniq[2]), (q + 1, -1, 0, uniq[2])]
    return _rows(lens, specs), want


def _window(program, row, off, n, hard):
    """[lo, hi) of the quality buffer that the record's QUAL is taken from (the model's slice, in the buffer's coordinates)."""
    frame, a, e = int(row["q_frame"]), int(row["q_start"]), int(row["q_end"])
    if program == "blastn":
        lo, hi = (a, e) if hard else (0, n)
    else:
        fc = abs(frame) - 1
        a, e = (a, e) if hard else (0, (n - fc) // 3)
        lo, hi = 3 * a + fc, 3 * e + fc
    return (off + n - hi, off + n - lo) if frame < 0 else (off + lo, off + hi)


@pytest.mark.parametrize("seq", [capi.LX_SAM_SEQ_ALWAYS, capi.LX_SAM_SEQ_UNIQ], ids=["always", "uniq"])
@pytest.mark.parametrize("hard", [1, 0], ids=["hard", "soft"])
@pytest.mark.parametrize("program", ["blastn", "blastx"])
def test_smallest_shapes(handle, program, hard, seq):
    (m, ops, names, qa, qoff), want = _shapes(program, hard)
    opt, keep = _options(program, ALL_TAGS, seq, hard, False, m, len(names["s_ids"]))
    qq = qual_bytes(len(qa))
    sam, bam = same(handle, program, m, ops, names, qa, qoff, opt, qq)
    check_against_model(program, m, names, qoff, qq, hard, sam)
    lines, recs = records_of(sam), decode(bam)[2]
    l_seq = [0 if f[9] == b"*" else len(f[9]) for f in lines]
    assert [r["l_seq"] for r in recs] == l_seq
    if program == "blastn" and not hard and seq == capi.LX_SAM_SEQ_ALWAYS:
        want = want[1:]  # (a soft-clipped read that is always written has its whole length: no record without SEQ)
    assert set(want) <= set(l_seq), sorted(set(l_seq))
    for f, r in zip(lines, recs):
        assert r["qual"] == (b"\xff" * r["l_seq"] if f[10] == b"*" else bytes(c - 33 for c in f[10]))
    # both strands, the buffer's first and last byte
    assert {int(f[1]) & 16 for f in lines if f[10] != b"*"} == {0, 16}
    windows = [_window(program, r, int(qoff[int(r["n_qid"])]), int(names["q_lens"][int(r["n_qid"])]), hard) for r, f in zip(m, lines) if f[10] != b"*"]
    assert any(lo == 0 and hi > lo for lo, hi in windows) and any(hi == len(qq) and hi > lo for lo, hi in windows)
    assert all(0 <= lo <= hi <= len(qq) for lo, hi in windows)
    # uniq: suppressed inside the group, written again at the next group's first record
    stars = [f[10] == b"*" for f in lines[-5:]]
    assert stars == ([False, True, True, False, False] if seq == capi.LX_SAM_SEQ_UNIQ else [False] * 5)


# ---- 3. tile and range edges

def _reads(n, length=150):
    """n reads of `length` letters, one record each, strands alternating, --sam-bam-clip soft: every record carries the whole read."""
    return _rows([length] * n, [(q, 1 if q % 2 else -1, 10, length - 20) for q in range(n)])


@pytest.mark.parametrize("n", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_record_counts_around_the_scan_tile(handle, n):
    m, ops, names, qa, qoff = _reads(n, length=40)
    opt, keep = _options("blastn", None, capi.LX_SAM_SEQ_ALWAYS, 1, False, m, len(names["s_ids"]))
    same(handle, "blastn", m, ops, names, qa, qoff, opt, qual_bytes(len(qa)))


@pytest.fixture(scope="module")
def ranged():
    m, ops, names, qa, qoff = _reads(3000)
    opt, keep = _options("blastn", None, capi.LX_SAM_SEQ_ALWAYS, 0, False, m, len(names["s_ids"]))
    return m, ops, names, qa, qoff, opt, keep, qual_bytes(len(qa))


def test_several_ranges_give_the_same_bytes(ranged):
    m, ops, names, qa, qoff, opt, keep, qq = ranged
    sam, bam = render(SAM, "blastn", m, ops, names, qa, qoff, opt, qq), render(BAM, "blastn", m, ops, names, qa, qoff, opt, qq)
    # (the qualities are in the sizes the ranges are cut from)
    assert len(sam) - len(render(SAM, "blastn", m, ops, names, qa, qoff, opt)) == 3000 * 149
    with capi.Handle(0) as h:
        assert dev_sam(h, "blastn", m, ops, names, qa, qoff, opt, qq) == sam
        one_range = h.last_phase_ms(12)[1]
        h.set_option(capi.LX_OPT_BAM_RANGE_BYTES, MIN_RANGE)
        assert dev_sam(h, "blastn", m, ops, names, qa, qoff, opt, qq) == sam
        assert h.last_phase_ms(12)[1] > one_range  # an emit per range: more than one range
        assert dev_bam(h, "blastn", m, ops, names, qa, qoff, opt, qq) == bam


@pytest.mark.parametrize("fmt,name", [(SAM, "o.sam.gz"), (BAM, "o.bam")])
def test_written_files_over_several_ranges(ranged, tmp_path, fmt, name):
    m, ops, names, qa, qoff, opt, keep, qq = ranged
    kw = dict(program="blastn", q_ascii=qa, q_ascii_off=qoff, options=opt, q_qual=qq)
    with capi.Handle(0) as h:
        h.write_records_bgzf(tmp_path / ("host_" + name), fmt, *_args(m, ops, names), **kw)
        h.set_option(capi.LX_OPT_BAM_RANGE_BYTES, MIN_RANGE)
        if fmt == BAM:
            h.write_bam(tmp_path / name, *_args(m, ops, names), **kw)
        else:
            h.write_text(tmp_path / name, fmt, *_args(m, ops, names), bgzf=True, **kw)
        assert h.last_phase_ms(4)[1] >= 2  # the encoder ran once per range
    raw = (tmp_path / name).read_bytes()
    assert raw == (tmp_path / ("host_" + name)).read_bytes()  # member for member
    assert gzip.decompress(raw) == render(fmt, "blastn", m, ops, names, qa, qoff, opt, qq)


# ---- 4. lx_out_append_ex

@pytest.mark.parametrize("fmt,bgzf,name", [(SAM, False, "o.sam"), (SAM, True, "o.sam.gz"), (BAM, True, "o.bam")])
@pytest.mark.parametrize("program", ["blastn", "blastx"])
def test_pieces_rendered_on_either_side_equal_the_one_shot_file(handle, tmp_path, program, fmt, bgzf, name):
    m, ops, names, qa, qoff = _case(program, seed=31, nq=9)
    opt, keep = _options(program, ALL_TAGS, capi.LX_SAM_SEQ_UNIQ, 1, False, m, 4)
    qq = qual_bytes(len(qa))
    ref, p = tmp_path / ("ref_" + name), tmp_path / name
    if bgzf:
        handle.write_records_bgzf(ref, fmt, *_args(m, ops, names), program=program, q_ascii=qa, q_ascii_off=qoff, options=opt, q_qual=qq)
    else:
        ref.write_bytes(render(fmt, program, m, ops, names, qa, qoff, opt, qq))
    starts = group_starts(m)
    kw = dict(handle=handle, bgzf=bgzf, fmt=fmt)
    for where in (DEV, [HOST, DEV], [DEV, HOST]):
        _append_pieces(p, program, m, ops, names, qa, qoff, opt, qq, starts, where=where, **kw)
        assert p.read_bytes() == ref.read_bytes(), where
    _append_pieces(p, program, m, ops, names, qa, qoff, opt, qq, [0, starts[4], len(m)], where=DEV, **kw)
    assert p.read_bytes() == ref.read_bytes()
    # pieces without qualities in between (lx_out_append): the file the host makes of the same pieces
    quals = [i % 3 != 1 for i in range(len(starts))]
    _append_pieces(ref, program, m, ops, names, qa, qoff, opt, qq, starts, where=HOST, quals=quals, **kw)
    assert ref.read_bytes() != p.read_bytes()
    for where in (DEV, [DEV, HOST]):
        _append_pieces(p, program, m, ops, names, qa, qoff, opt, qq, starts, where=where, quals=quals, **kw)
        assert p.read_bytes() == ref.read_bytes(), where
    text = gzip.decompress(p.read_bytes()) if bgzf else p.read_bytes()
    if fmt == SAM:
        by_group = [{f[10] == b"*" for f in records_of(text)[lo:hi] if f[9] != b"*"} for lo, hi in zip(starts[:-1], starts[1:])]
        assert by_group == [{not q} for q in quals[:len(by_group)]]


# ---- 5. the front end, end to end

COMP = str.maketrans("ACGT", "TGCA")
CODON = {"A": "GCT", "C": "TGC", "D": "GAC", "E": "GAA", "F": "TTC", "G": "GGA", "H": "CAC", "I": "ATC", "K": "AAG", "L": "CTG", "M": "ATG",
         "N": "AAC", "P": "CCA", "Q": "CAG", "R": "CGT", "S": "TCA", "T": "ACT", "V": "GTG", "W": "TGG", "Y": "TAC"}


def _fasta(path, ids, seqs):
    path.write_text("".join(f">{i}\n{s}\n" for i, s in zip(ids, seqs)))


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """searchn: 30 reads of 100 nt planted in a nucleotide database, both strands, two mismatches each.  searchp (BLASTX): 24 DNA
    reads that spell 33 residues of a protein of a small database behind 0 .. 2 letters, both strands.  Each read set as FASTQ
    (qualities: slices of the tests' quality buffer, so every read has its own) and as FASTA."""
    tmp = tmp_path_factory.mktemp("planted")
    rng = np.random.default_rng(51)
    genome = ["".join("ACGT"[i] for i in rng.integers(0, 4, 3000)) for _ in range(3)]
    _fasta(tmp / "g.fasta", [f"chr{i} contig" for i in range(3)], genome)
    reads = []
    for k in range(30):
        c, a = int(rng.integers(0, 3)), int(rng.integers(0, 2900))
        r = list(genome[c][a:a + 100])
        for p_ in rng.integers(0, 100, 2):
            r[p_] = "ACGT"[int(rng.integers(0, 4))]
        r = "".join(r)
        reads.append(r.translate(COMP)[::-1] if k % 2 else r)
    aas = sorted(CODON)
    prots = ["".join(aas[i] for i in rng.integers(0, 20, 120)) for _ in range(20)]
    _fasta(tmp / "p.fasta", [f"sp{j} protein {j}" for j in range(20)], prots)
    xreads = []
    for k in range(24):
        j, a = int(rng.integers(0, 20)), int(rng.integers(0, 87))
        r = "ACG"[:k % 3] + "".join(CODON[c] for c in prots[j][a:a + 33]) + "T"
        xreads.append(r.translate(COMP)[::-1] if k % 2 else r)
    sets = {}
    for name, rs in (("n", reads), ("x", xreads)):
        ids = [f"{name}read{k} len={len(r)}" for k, r in enumerate(rs)]
        qq = qual_bytes(sum(len(r) for r in rs)).decode()
        offs = np.concatenate([[0], np.cumsum([len(r) for r in rs])])
        quals = [qq[offs[k]:offs[k + 1]] for k in range(len(rs))]
        (tmp / f"{name}.fq").write_text("".join(f"@{i}\n{r}\n+\n{q}\n" for i, r, q in zip(ids, rs, quals)))
        _fasta(tmp / f"{name}.fa", ids, rs)
        sets[name] = {i.split()[0]: (r, q) for i, r, q in zip(ids, rs, quals)}
    return tmp, sets


SEARCHES = {"searchn": ("n", "g.fasta"), "searchp": ("x", "p.fasta")}


def _run(tmp, out_dir, cmd, query, name, *extra):
    cli = build.build_cli()
    r = subprocess.run([str(cli), cmd, "-q", str(tmp / query), "-d", str(tmp / SEARCHES[cmd][1]), "-o", str(out_dir / name), "--version-to-outputfile", "0",
                        *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return (out_dir / name).read_bytes(), r.stderr


def _check_lines(lines, reads):
    """QUAL of every record: the read's qualities over the letters SEQ shows (found in the read as it was read: SEQ is a piece of
    the read, or of its reverse complement, and occurs in it once), turned with the strand."""
    carried = 0
    for f in lines:
        read, qual = reads[f[0].decode()]
        if f[9] == b"*":
            assert f[10] == b"*"
            continue
        minus = bool(int(f[1]) & 16)
        turned, tq = (read.translate(COMP)[::-1], qual[::-1]) if minus else (read, qual)
        seq = f[9].decode()
        assert turned.count(seq) == 1
        at = turned.index(seq)
        assert f[10].decode() == tq[at:at + len(seq)], f
        carried += 1
    return carried


@pytest.mark.parametrize("ext", ["sam", "bam"])
@pytest.mark.parametrize("cmd", ["searchn", "searchp"])
def test_cli_writes_the_fastq_qualities(planted, tmp_path, cmd, ext):
    tmp, sets = planted
    q = SEARCHES[cmd][0]
    yes = ("--sam-bam-qual", "yes")
    on_gpu, _ = _run(tmp, tmp_path, cmd, q + ".fq", "gpu." + ext, *yes, "--render", "gpu")
    on_host, _ = _run(tmp, tmp_path, cmd, q + ".fq", "host." + ext, *yes, "--render", "host")
    assert on_gpu == on_host
    for mode in ("gpu", "host"):
        lazy, _ = _run(tmp, tmp_path, cmd, q + ".fq", f"lazy_{mode}." + ext, *yes, "--render", mode, "--lazy-query", "1", "--query-block", "3")
        assert lazy == on_gpu, mode
    sam, _ = _run(tmp, tmp_path, cmd, q + ".fq", "ref.sam", *yes) if ext == "bam" else (on_gpu, "")
    lines = records_of(sam)
    assert len({f[0] for f in lines}) >= len(sets[q]) * 3 // 4  # (the planted reads are found)
    assert _check_lines(lines, sets[q]) >= len(sets[q]) * 3 // 4
    assert {int(f[1]) & 16 for f in lines if f[10] != b"*"} == {0, 16}
    if ext == "bam":
        recs = decode(gzip.decompress(on_gpu))[2]
        assert len(recs) == len(lines)
        for f, r in zip(lines, recs):
            assert r["qual"] == (b"\xff" * r["l_seq"] if f[10] == b"*" else bytes(c - 33 for c in f[10]))


@pytest.mark.parametrize("cmd", ["searchn", "searchp"])
def test_cli_no_and_fasta_queries(planted, tmp_path, cmd):
    tmp, sets = planted
    q = SEARCHES[cmd][0]
    from_fasta, _ = _run(tmp, tmp_path, cmd, q + ".fa", "fa.sam")
    no, err = _run(tmp, tmp_path, cmd, q + ".fq", "no.sam", "--sam-bam-qual", "no")
    assert no == from_fasta and "no qualities" not in err
    assert all(f[10] == b"*" for f in records_of(no)) and len(records_of(no)) > 0
    for extra in ((), ("--lazy-query", "1", "--query-block", "5")):
        yes, err = _run(tmp, tmp_path, cmd, q + ".fa", "fa_yes.sam", "--sam-bam-qual", "yes", "--render", "gpu", *extra)
        assert yes == from_fasta
        assert err.count("--sam-bam-qual yes: the query file has no qualities") == 1, err
