"""CPU tests of the BAM writer and of lx_render_records: the BAM stream decoded back to SAM equals the SAM writer's text line for line,
and the text formats rendered in memory equal the files of lx_write_records_ex + lx_write_footer.  No GPU needed."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests import bam_decode

ALL_TAGS = "AS OC NM IH ar ae ai ap qf qs sf st ls lt"
PROGRAMS = ["blastn", "blastp", "blastx", "tblastn", "tblastx"]


def _case(program, seed=0, nq=6, ns=4):
    """Records of every shape the SAM writer has: several per query (secondary flags, --sam-bam-seq uniq), both strands, frames."""
    rng = np.random.default_rng(seed)
    q_nucl = program in ("blastn", "blastx", "tblastx")
    alph = "ACGT" if q_nucl else "ARNDCQEGHILKMFPSTWYV"
    q_lens = rng.integers(90, 200, nq)
    q_seqs = ["".join(alph[i] for i in rng.integers(0, len(alph), int(n))) for n in q_lens]
    s_lens = rng.integers(500, 3000, ns)
    q_trans, s_trans = program in ("blastx", "tblastx"), program in ("tblastn", "tblastx")
    recs, ops = [], b""
    for q in range(nq):
        for k in range(int(rng.integers(1, 5))):
            qf = int(rng.choice([-1, 1])) if program == "blastn" else int(rng.choice([-3, -2, -1, 1, 2, 3])) if q_trans else 0
            sf = int(rng.choice([-3, -2, -1, 1, 2, 3])) if s_trans else 0
            frame_len = (int(q_lens[q]) - (abs(qf) - 1)) // 3 if q_trans else int(q_lens[q])
            a = int(rng.integers(0, frame_len // 3))
            run = [int(x) for x in rng.integers(2, 9, 3)]
            o = b"M" * run[0] + b"D" * int(rng.integers(0, 3)) + b"M" * run[1] + b"I" * int(rng.integers(0, 3)) + b"M" * run[2]
            e = min(frame_len, a + run[0] + run[1] + run[2] + o.count(b"I"))
            if k == 2 and recs:  # same query range and frame as the previous record: no SEQ under "uniq"
                a, e, qf = int(recs[-1]["q_start"]), int(recs[-1]["q_end"]), int(recs[-1]["q_frame"])
            r = np.zeros(1, dtype=capi.BLAST_MATCH_DTYPE)[0]
            r["n_qid"], r["qry_id"], r["n_sid"], r["subj_id"] = q, q, int(rng.integers(0, ns)), 0
            ss = int(rng.integers(0, 10)) if s_trans else int(rng.integers(0, 400))
            r["q_start"], r["q_end"], r["s_start"], r["s_end"] = a, e, ss, ss + (e - a)
            r["bit_score"], r["score"], r["e_value"] = float(rng.uniform(20, 900)), int(rng.integers(20, 600)), float(10.0 ** rng.uniform(-180, 1))
            r["identity"], r["alignment_length"] = float(rng.uniform(40, 100)), len(o)
            r["num_matches"], r["num_positives"] = len(o) - int(rng.integers(0, 5)), len(o) - int(rng.integers(0, 3))
            r["ops_off"], r["n_ops"], r["q_frame"], r["s_frame"] = len(ops), len(o), qf, sf
            ops += o
            recs.append(r)
    m = np.array(recs, dtype=capi.BLAST_MATCH_DTYPE)
    qa = "".join(q_seqs).encode()
    qoff = np.concatenate([[0], np.cumsum(q_lens)[:-1]]).astype(np.uint64)
    names = dict(q_ids=[f"q{i} desc" for i in range(nq)], q_lens=q_lens, s_ids=[f"s{j} subject" for j in range(ns)], s_lens=s_lens)
    return m, ops, names, qa, qoff


def _tax(ns):
    parents = np.array([0, 0, 1, 1, 2, 2], np.uint32)
    heights = np.array([0, 1, 2, 2, 3, 3], np.uint32)
    s_tax_off = np.array([0, 1, 3, 3, 4][: ns + 1] + [4] * max(0, ns + 1 - 5), np.uint64)
    s_tax_ids = np.array([4, 5, 3, 2], np.uint32)
    return parents, heights, s_tax_off, s_tax_ids


def _options(program, tags, seq, hard, tree, m, ns, ref_header=1):
    o = capi.output_options(sam_tags=tags, sam_seq=seq, sam_hard_clip=hard, sam_with_ref_header=ref_header)
    keep = []
    if tree:
        parents, heights, off, ids = _tax(ns)
        qid, lca = capi.compute_lca(m, parents, heights, off, ids)
        t = capi.TaxTree(parents.ctypes.data, heights.ctypes.data, len(parents), off.ctypes.data, ids.ctypes.data, ns)
        tn = (C.c_char_p * 6)(*[f"taxon {i}".encode() for i in range(6)])
        o.tax, o.lca_qid, o.lca_tax, o.n_lca = C.addressof(t), qid.ctypes.data, lca.ctypes.data, len(qid)
        o.tax_names = C.cast(tn, C.c_void_p)
        keep += [parents, heights, off, ids, qid, lca, t, tn]
    return o, keep


def _render(fmt, program, m, ops, names, qa, qoff, opt, footer=-1):
    return capi.render_records(fmt, m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program,
                               q_ascii=qa, q_ascii_off=qoff, options=opt, footer_records=footer)


@pytest.mark.parametrize("program", PROGRAMS)
@pytest.mark.parametrize("seq,hard,tree", [(capi.LX_SAM_SEQ_ALWAYS, 1, True), (capi.LX_SAM_SEQ_UNIQ, 0, False),
                                           (capi.LX_SAM_SEQ_NEVER, 1, False), (capi.LX_SAM_SEQ_UNIQ, 1, True)])
def test_bam_decodes_to_the_sam_text(tmp_path, program, seq, hard, tree):
    m, ops, names, qa, qoff = _case(program, seed=PROGRAMS.index(program) * 7 + seq)
    opt, keep = _options(program, ALL_TAGS, seq, hard, tree, m, len(names["s_ids"]))
    sam_path = tmp_path / "o.sam"
    capi.write_records(sam_path, capi.LX_OUT_SAM, m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program,
                       q_ascii=qa, q_ascii_off=qoff, options=opt)
    bam = _render(capi.LX_OUT_BAM, program, m, ops, names, qa, qoff, opt)
    assert bam_decode.to_sam(bam) == sam_path.read_text().splitlines()
    text, refs, recs = bam_decode.decode(bam)
    assert refs == [(n.split()[0], int(l)) for n, l in zip(names["s_ids"], names["s_lens"])]
    assert len(recs) == len(m)
    for r in recs:
        assert [(k, t) for k, t, _ in r["tags"]] == [(k, bam_decode.TAG_TYPES[k]) for k, _, _ in r["tags"]]
        assert len(r["tags"]) == 14
        assert r["bin"] == bam_decode.reg2bin(r["pos"], r["pos"] + (bam_decode.span(r["cigar"]) or 1))
        assert r["mapq"] == 255 and r["next"] == (-1, -1, 0)
        if program in ("blastp", "tblastn"):
            assert r["l_seq"] == 0 and r["cigar"] == ()


def test_bam_header_carries_the_references_without_the_option():
    m, ops, names, qa, qoff = _case("blastn", seed=3)
    opt, _ = _options("blastn", "AS NM ae ai qf", capi.LX_SAM_SEQ_UNIQ, 1, False, m, 4, ref_header=0)
    bam = _render(capi.LX_OUT_BAM, "blastn", m, ops, names, qa, qoff, opt)
    text, refs, _ = bam_decode.decode(bam)
    assert text.count("@SQ\t") == len(refs) == 4
    # default tags keep their types too
    assert [k for k, _, _ in bam_decode.decode(bam)[2][0]["tags"]] == ["ae", "AS", "ai", "qf", "NM"]


@pytest.mark.parametrize("fmt", [capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS, capi.LX_OUT_SAM])
@pytest.mark.parametrize("program", PROGRAMS)
def test_rendered_text_equals_the_file_writer(tmp_path, fmt, program):
    m, ops, names, qa, qoff = _case(program, seed=11)
    opt, keep = _options(program, ALL_TAGS, capi.LX_SAM_SEQ_UNIQ, 1, True, m, 4)
    p = tmp_path / "o.txt"
    capi.write_records(p, fmt, m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program, q_ascii=qa,
                       q_ascii_off=qoff, options=opt)
    capi.write_footer(p, fmt, 6)
    assert _render(fmt, program, m, ops, names, qa, qoff, opt, footer=6) == p.read_bytes()
    p.unlink()
    capi.write_records(p, fmt, m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program, q_ascii=qa,
                       q_ascii_off=qoff, options=opt)
    assert _render(fmt, program, m, ops, names, qa, qoff, opt) == p.read_bytes()


def test_new_entries_refuse_bad_arguments():
    lib = capi.load()
    out = C.c_void_p()
    m, ops, names, qa, qoff = _case("blastp", seed=1)
    with pytest.raises(capi.LambdaExtError) as e:
        _render(capi.LX_OUT_BAM, "blastq", m, ops, names, qa, qoff, None)
    assert e.value.args[0] == capi.LX_EINVAL or "blastq" not in str(e.value)
    assert lib.lx_render_records(7, 1, b"blastp", None, 0, None, None, None, None, None, -1, C.byref(out)) == capi.LX_EINVAL
    assert lib.lx_render_records(capi.LX_OUT_BAM, 1, b"blastp", None, 0, None, None, None, None, None, -1, None) == capi.LX_EINVAL
    assert lib.lx_render_records(capi.LX_OUT_SAM, 1, b"blastp", None, 0, None, None, None, None, None, -1, C.byref(out)) == capi.LX_EINVAL
    bad_tag = capi.output_options(sam_tags="AS xx")
    with pytest.raises(capi.LambdaExtError):
        _render(capi.LX_OUT_BAM, "blastp", m, ops, names, qa, qoff, bad_tag)
    # BAM does not go through the text writer
    assert lib.lx_write_records_ex(b"/nonexistent/x.bam", capi.LX_OUT_BAM, 1, b"blastp", None, 0, None, None, None, None, None) == capi.LX_EINVAL
    assert lib.lx_check_output_options(capi.LX_OUT_BAM, None) == capi.LX_OK
    # the compression entries: a NULL handle before anything else
    got = C.c_uint64(0)
    buf = (C.c_uint8 * 64)()
    assert lib.lx_bgzf_compress(None, buf, 1, buf, 64, C.byref(got), 0) == capi.LX_EINVAL
    assert lib.lx_write_records_bgzf(None, b"x.bam", capi.LX_OUT_BAM, b"blastp", None, 0, None, None, None, None, None, -1) == capi.LX_EINVAL
    assert capi.bgzf_bound(0) == 28 and capi.bgzf_bound(65280) == 65280 + 31 + 28 and capi.bgzf_bound(65281) == 65281 + 62 + 28


@pytest.mark.parametrize("name", ["o.bz2", "o.m8.bz2", "o.sam.bz2", "o.m0", "o.m0.gz", "o.bam.gz", "o.txt"])
def test_cli_refuses_unsupported_output_formats_at_parse_time(tmp_path, name):
    cli = build.build_cli()
    # (the query and database do not exist: the format is refused before they are opened)
    r = subprocess.run([str(cli), "searchp", "-q", str(tmp_path / "none.fa"), "-d", str(tmp_path / "none.fa"), "-o", str(tmp_path / name)],
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "output format is chosen by the extension: .m8, .m9, .sam or .bam, the first three optionally with .gz" in r.stderr, r.stderr
    assert ".m0, .bz2 and .bam.gz are not supported" in r.stderr


@pytest.mark.parametrize("name", ["o.bam", "o.m8.gz", "o.m9.gz", "o.sam.gz"])
def test_cli_accepts_bam_and_gz_outputs_at_parse_time(tmp_path, name):
    cli = build.build_cli()
    r = subprocess.run([str(cli), "searchp", "-q", str(tmp_path / "none.fa"), "-d", str(tmp_path / "none.fa"), "-o", str(tmp_path / name)],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "chosen by the extension" not in r.stderr, r.stderr
