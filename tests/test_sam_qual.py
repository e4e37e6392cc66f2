"""FASTQ base qualities in SAM and BAM records (lx_output_options::q_qual, lx_out_append_ex, --sam-bam-qual), on the host: QUAL is
written exactly where SEQ is written, over the same letters, in the same direction.  The yardstick is a model of that rule stated
here from the rows alone; the host writer pinned by it is what the device writers are held against (tests/test_gpu_sam_qual.py).
No GPU needed."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests.bam_decode import decode
from tests.test_bam_encoding import ALL_TAGS, PROGRAMS, _case, _options

SAM, BAM = capi.LX_OUT_SAM, capi.LX_OUT_BAM
COMBOS = [(capi.LX_SAM_SEQ_ALWAYS, 1, True), (capi.LX_SAM_SEQ_UNIQ, 0, False), (capi.LX_SAM_SEQ_NEVER, 1, False), (capi.LX_SAM_SEQ_UNIQ, 1, True)]


def qual_bytes(n: int) -> bytes:
    """The tests' quality buffer: byte i is 33 + (7 i + i // 94) % 94 -- neighbours differ and no read is a palindrome, so a shift by
    one, a missed reversal or a wrong read shows."""
    i = np.arange(n, dtype=np.int64)
    return (33 + (7 * i + i // 94) % 94).astype(np.uint8).tobytes()


def model_qual(program, row, read_qual: bytes, hard) -> bytes:
    """QUAL of a record whose SEQ is written, from the row and the read's qualities alone."""
    frame, a, e, n = int(row["q_frame"]), int(row["q_start"]), int(row["q_end"]), len(read_qual)
    turned = read_qual[::-1] if frame < 0 else read_qual
    if program == "blastn":
        return turned[a:e] if hard else turned
    fc = abs(frame) - 1
    if not hard:
        a, e = 0, (n - fc) // 3
    return turned[3 * a + fc:3 * e + fc]


def render(fmt, program, m, ops, names, qa, qoff, opt, q_qual=None, header=True):
    return capi.render_records(fmt, m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program, write_header=header,
                               q_ascii=qa, q_ascii_off=qoff, options=opt, q_qual=q_qual)


def records_of(sam: bytes):
    return [line.split(b"\t") for line in sam.split(b"\n") if line and not line.startswith(b"@")]


def check_against_model(program, m, names, qoff, qq, hard, sam: bytes):
    """Column 11 of every line against the model; the number of records that carry qualities."""
    lines = records_of(sam)
    assert len(lines) == len(m)
    with_qual = 0
    for row, f in zip(m, lines):
        q = int(row["n_qid"])
        read = qq[int(qoff[q]):int(qoff[q]) + int(names["q_lens"][q])]
        if f[9] == b"*":
            assert f[10] == b"*", f
        else:
            assert f[10] == model_qual(program, row, read, hard), (program, row, f[9], f[10])
            assert len(f[10]) == len(f[9])
            with_qual += 1
    return with_qual


@pytest.fixture(scope="module")
def cases():
    out = {}
    for program in PROGRAMS:
        for seq, hard, tree in COMBOS:
            m, ops, names, qa, qoff = _case(program, seed=PROGRAMS.index(program) * 7 + seq)
            opt, keep = _options(program, ALL_TAGS, seq, hard, tree, m, len(names["s_ids"]))
            out[program, seq, hard, tree] = (m, ops, names, qa, qoff, opt, keep, qual_bytes(len(qa)))
    return out


@pytest.mark.parametrize("seq,hard,tree", COMBOS)
@pytest.mark.parametrize("program", PROGRAMS)
def test_sam_qual_equals_the_model(cases, program, seq, hard, tree):
    m, ops, names, qa, qoff, opt, keep, qq = cases[program, seq, hard, tree]
    sam = render(SAM, program, m, ops, names, qa, qoff, opt, qq)
    n = check_against_model(program, m, names, qoff, qq, hard, sam)
    dna = program in ("blastn", "blastx", "tblastx")
    if dna and seq != capi.LX_SAM_SEQ_NEVER:
        assert n >= len(names["q_ids"])  # (the first record of every query at least)
        assert any(int(r["q_frame"]) < 0 for r, f in zip(m, records_of(sam)) if f[10] != b"*")  # the minus strand is there
    else:
        assert n == 0  # a protein query, --sam-bam-seq never: "*" everywhere
    if seq == capi.LX_SAM_SEQ_UNIQ and dna:
        assert n < len(m)  # (a record suppressed by uniq)


@pytest.mark.parametrize("seq,hard,tree", COMBOS)
@pytest.mark.parametrize("program", PROGRAMS)
def test_only_the_quality_field_differs(cases, program, seq, hard, tree):
    m, ops, names, qa, qoff, opt, keep, qq = cases[program, seq, hard, tree]
    with_q, without = render(SAM, program, m, ops, names, qa, qoff, opt, qq), render(SAM, program, m, ops, names, qa, qoff, opt)
    a, b = with_q.split(b"\n"), without.split(b"\n")
    assert len(a) == len(b)
    for x, y in zip(a, b):
        fx, fy = x.split(b"\t"), y.split(b"\t")
        if not x.startswith(b"@") and x:
            assert fy[10] == b"*"
            fx[10] = b"*"
        assert fx == fy
    # BAM: the same sizes, every byte but the quality bytes equal
    bam_q, bam = render(BAM, program, m, ops, names, qa, qoff, opt, qq), render(BAM, program, m, ops, names, qa, qoff, opt)
    assert len(bam_q) == len(bam)
    _, _, recs_q = decode(bam_q)
    _, _, recs = decode(bam)
    masked = bytearray(bam_q)  # (walk the records to blank the quality bytes)
    text, refs, _ = decode(bam)
    p = 8 + len(text.encode()) + 4 + sum(8 + len(n) + 1 for n, _ in refs)
    for r in recs_q:
        (bs,) = np.frombuffer(bam_q, "<i4", 1, p)
        l_name, n_cig, l_seq = bam_q[p + 12], int(np.frombuffer(bam_q, "<u2", 1, p + 16)[0]), r["l_seq"]
        q = p + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
        masked[q:q + l_seq] = b"\xff" * l_seq
        p += 4 + int(bs)
    assert p == len(bam_q) and bytes(masked) == bam
    assert [{k: v for k, v in r.items() if k != "qual"} for r in recs_q] == [{k: v for k, v in r.items() if k != "qual"} for r in recs]


@pytest.mark.parametrize("seq,hard,tree", COMBOS)
@pytest.mark.parametrize("program", PROGRAMS)
def test_bam_qual_is_the_sam_string_minus_33(cases, program, seq, hard, tree):
    m, ops, names, qa, qoff, opt, keep, qq = cases[program, seq, hard, tree]
    lines = records_of(render(SAM, program, m, ops, names, qa, qoff, opt, qq))
    _, _, recs = decode(render(BAM, program, m, ops, names, qa, qoff, opt, qq))
    assert len(recs) == len(lines)
    for f, r in zip(lines, recs):
        assert r["l_seq"] == (0 if f[9] == b"*" else len(f[9]))
        if f[10] == b"*":
            assert r["qual"] == b"\xff" * r["l_seq"]
        else:
            assert r["qual"] == bytes(c - 33 for c in f[10])


def test_bytes_outside_the_printable_range_wrap_modulo_256():
    m, ops, names, qa, qoff = _case("blastn", seed=5)
    opt, keep = _options("blastn", None, capi.LX_SAM_SEQ_ALWAYS, 1, False, m, 4)
    i = np.arange(len(qa), dtype=np.int64)
    qq = ((i * 37 + 1) % 255 + 1).astype(np.uint8)  # 1 .. 255, 0 left out (SAM's text line would end there)
    qq[qq == 9] = 200  # (and no tab or newline: the SAM line is split on them below)
    qq[qq == 10] = 201
    qq = qq.tobytes()
    assert min(qq) < 33 and max(qq) > 126
    lines = records_of(render(SAM, "blastn", m, ops, names, qa, qoff, opt, qq))
    _, _, recs = decode(render(BAM, "blastn", m, ops, names, qa, qoff, opt, qq))
    seen = set()
    for row, f, r in zip(m, lines, recs):
        q = int(row["n_qid"])
        want = model_qual("blastn", row, qq[int(qoff[q]):int(qoff[q]) + int(names["q_lens"][q])], 1)
        assert f[10] == want  # SAM: the bytes as they stand
        assert r["qual"] == bytes((b - 33) & 0xFF for b in want)
        seen |= set(want)
    assert min(seen) < 33 and max(seen) > 126


def test_the_file_writer_the_null_letters_and_the_tabular_formats(tmp_path):
    for program in ("blastn", "tblastx"):
        m, ops, names, qa, qoff = _case(program, seed=9)
        opt, keep = _options(program, ALL_TAGS, capi.LX_SAM_SEQ_UNIQ, 1, True, m, 4)
        qq = qual_bytes(len(qa))
        args = (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"])
        p = tmp_path / "o.sam"
        capi.write_records(p, SAM, *args, program=program, q_ascii=qa, q_ascii_off=qoff, options=opt, q_qual=qq)
        assert p.read_bytes() == render(SAM, program, m, ops, names, qa, qoff, opt, qq)
        assert p.read_bytes() != render(SAM, program, m, ops, names, qa, qoff, opt)
        # q_qual without the letters is not read
        assert render(SAM, program, m, ops, names, None, None, opt, qq) == render(SAM, program, m, ops, names, None, None, opt)
        assert render(BAM, program, m, ops, names, None, qoff, opt, qq) == render(BAM, program, m, ops, names, None, qoff, opt)
        for fmt in (capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS):
            assert render(fmt, program, m, ops, names, qa, qoff, opt, qq) == render(fmt, program, m, ops, names, qa, qoff, opt)
    o = capi.output_options()
    assert not o.q_qual  # lx_output_options_default: none


def _append_pieces(path, program, m, ops, names, qa, qoff, opt, qq, cuts, where=capi.LX_RENDER_HOST, handle=None, bgzf=False, fmt=SAM, quals=None):
    """The list through lx_out in pieces [cuts[i], cuts[i + 1]) of whole query groups, each with the ids, lengths, letters and
    qualities of its own queries; quals[i] False: that piece goes through lx_out_append, without qualities."""
    with capi.Out(handle, path, fmt, names["s_ids"], names["s_lens"], program=program, bgzf=bgzf, options=opt) as out:
        for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            piece = m[lo:hi].copy()
            q0, q1 = int(piece["n_qid"].min()), int(piece["n_qid"].max()) + 1
            piece["n_qid"] -= q0
            a0, a1 = int(qoff[q0]), int(qoff[q1 - 1]) + int(names["q_lens"][q1 - 1])
            use = quals is None or quals[i]
            w = where[i % len(where)] if isinstance(where, (list, tuple)) else where
            out.append(w, piece, ops, names["q_ids"][q0:q1], names["q_lens"][q0:q1], q_ascii=qa[a0:a1], q_ascii_off=np.asarray(qoff[q0:q1]) - a0,
                       q_qual=qq[a0:a1] if use else None)


def group_starts(m):
    return [0] + [k for k in range(1, len(m)) if m["n_qid"][k] != m["n_qid"][k - 1]] + [len(m)]


@pytest.mark.parametrize("program", ["blastn", "blastx"])
def test_pieces_on_the_host_equal_the_one_shot_writer(tmp_path, program):
    m, ops, names, qa, qoff = _case(program, seed=13)
    opt, keep = _options(program, None, capi.LX_SAM_SEQ_UNIQ, 1, False, m, 4, ref_header=0)
    qq = qual_bytes(len(qa))
    ref = render(SAM, program, m, ops, names, qa, qoff, opt, qq)
    plain = render(SAM, program, m, ops, names, qa, qoff, opt)
    assert ref != plain
    starts = group_starts(m)
    p = tmp_path / "o.sam"
    for cut in starts[1:-1]:  # two pieces, cut at every group boundary in turn
        _append_pieces(p, program, m, ops, names, qa, qoff, opt, qq, [0, cut, len(m)])
        assert p.read_bytes() == ref, cut
    _append_pieces(p, program, m, ops, names, qa, qoff, opt, qq, starts)  # one piece per group
    assert p.read_bytes() == ref
    _append_pieces(p, program, m, ops, names, qa, qoff, opt, qq, [0, len(m)])
    assert p.read_bytes() == ref
    # lx_out_append on the same kind of object: no qualities
    _append_pieces(p, program, m, ops, names, qa, qoff, opt, qq, starts, quals=[False] * len(starts))
    assert p.read_bytes() == plain
    # and mixed: the pieces appended without them write "*", the others their qualities
    _append_pieces(p, program, m, ops, names, qa, qoff, opt, qq, starts, quals=[i % 2 == 0 for i in range(len(starts))])
    want = ref.split(b"\n")
    head = len(want) - 1 - len(m)
    for g, (lo, hi) in enumerate(zip(starts[:-1], starts[1:])):
        if g % 2:
            want[head + lo:head + hi] = plain.split(b"\n")[head + lo:head + hi]
    assert p.read_bytes() == b"\n".join(want)


def _cli(tmp_path, *args):
    cli = build.build_cli()
    # (the query and database do not exist: what is refused while the options are parsed is refused before they are opened)
    return subprocess.run([str(cli), "searchn", "-q", str(tmp_path / "none.fq"), "-d", str(tmp_path / "none.fa"), *args], capture_output=True, text=True)


@pytest.mark.parametrize("args,why", [(["--sam-bam-qual", "yes", "-o", "x.m8"], "tabular format"),
                                      (["--sam-bam-qual", "yes", "-o", "x.m9.gz"], "tabular format"),
                                      (["--sam-bam-qual", "yes", "--sam-bam-seq", "never", "-o", "x.sam"], "QUAL is written where SEQ is written"),
                                      (["--sam-bam-seq", "never", "-o", "x.bam", "--sam-bam-qual", "yes"], "QUAL is written where SEQ is written"),
                                      (["--sam-bam-qual", "maybe", "-o", "x.sam"], "--sam-bam-qual takes no or yes")])
def test_cli_refuses_at_parse_time(tmp_path, args, why):
    r = _cli(tmp_path, *[str(tmp_path / a) if a.startswith("x.") else a for a in args])
    assert r.returncode != 0 and why in r.stderr, r.stderr
    assert "cannot open" not in r.stderr


@pytest.mark.parametrize("name", ["x.sam", "x.sam.gz", "x.bam"])
@pytest.mark.parametrize("value", ["yes", "no"])
def test_cli_accepts_sam_and_bam_up_to_the_inputs(tmp_path, name, value):
    r = _cli(tmp_path, "--sam-bam-qual", value, "-o", str(tmp_path / name))
    assert r.returncode != 0 and "cannot open" in r.stderr and "sam-bam-qual" not in r.stderr, r.stderr


def test_the_binding_has_the_field_and_the_export():
    assert OutputOptionsLast() == "q_qual"
    lib = capi.load()
    assert lib.lx_abi_version() == 3
    assert lib.lx_out_append_ex(None, 0, None, 0, None, 0, None, None, None, None, None, None, 0) == capi.LX_EINVAL


def OutputOptionsLast():
    return capi.OutputOptions._fields_[-1][0]
