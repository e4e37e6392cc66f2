"""GPU tests of the BAM record kernels (lx_bam.hip) behind lx_render_bam_dev / lx_write_bam_dev: the bytes equal those of the host writer
(lx_render_records(LX_OUT_BAM) / lx_write_records_bgzf, itself pinned to the SAM text by tests/test_bam_encoding.py) for every program
and option, at the smallest shapes where a field can go wrong, at the edges of the kernels' tiles and of the ranges, and through the
front end's --render gpu."""
import ctypes as C
import gzip
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests import bam_decode
from tests.test_bam_encoding import ALL_TAGS, PROGRAMS, _case, _options, _render

pytestmark = pytest.mark.gpu

# lx_bam.h: records per emit workgroup (kBamEmitBlock = 256 threads, one wavefront of 64 per record), records per scan / size tile
EMIT_RECORDS = 256 // 64
SCAN_TILE = 2048
MIN_RANGE = 128 << 10
COMBOS = [(capi.LX_SAM_SEQ_ALWAYS, 1, True), (capi.LX_SAM_SEQ_UNIQ, 0, False), (capi.LX_SAM_SEQ_NEVER, 1, False), (capi.LX_SAM_SEQ_UNIQ, 1, True)]


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


def _dev(h, program, m, ops, names, qa, qoff, opt, write_header=True):
    return h.render_bam(m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program, write_header=write_header,
                        q_ascii=qa, q_ascii_off=qoff, options=opt)


def _host(program, m, ops, names, qa, qoff, opt, write_header=True):
    return capi.render_records(capi.LX_OUT_BAM, m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program,
                               write_header=write_header, q_ascii=qa, q_ascii_off=qoff, options=opt)


def _same(h, program, m, ops, names, qa, qoff, opt, write_header=True):
    dev, ref = _dev(h, program, m, ops, names, qa, qoff, opt, write_header), _host(program, m, ops, names, qa, qoff, opt, write_header)
    if dev != ref and write_header:  # a framing error reads better as SAM lines than as hex (where both streams still decode)
        try:
            lines = bam_decode.to_sam(dev), bam_decode.to_sam(ref)
        except Exception:
            lines = None
        if lines:
            assert lines[0] == lines[1]
    assert dev == ref
    return dev


def _all(program, m, ns=4, seq=capi.LX_SAM_SEQ_ALWAYS, hard=1, tree=True):
    return _options(program, ALL_TAGS, seq, hard, tree, m, ns)


# ---- formats and options

@pytest.mark.parametrize("tags", [ALL_TAGS, None], ids=["all", "default"])
@pytest.mark.parametrize("seq,hard,tree", COMBOS)
@pytest.mark.parametrize("program", PROGRAMS)
def test_bytes_equal_the_host_writer(handle, program, seq, hard, tree, tags):
    m, ops, names, qa, qoff = _case(program, seed=PROGRAMS.index(program) * 7 + seq)
    if tags is None:
        opt, keep = _options(program, "AS NM ae ai qf", seq, hard, tree, m, 4)
        opt.sam_tags = None
    else:
        opt, keep = _options(program, tags, seq, hard, tree, m, 4)
    _same(handle, program, m, ops, names, qa, qoff, opt)


@pytest.mark.parametrize("program", PROGRAMS)
def test_device_bytes_decode_to_the_sam_text(handle, tmp_path, program):
    m, ops, names, qa, qoff = _case(program, seed=31)
    opt, keep = _all(program, m, seq=capi.LX_SAM_SEQ_UNIQ)
    sam = tmp_path / "o.sam"
    capi.write_records(sam, capi.LX_OUT_SAM, m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program,
                       q_ascii=qa, q_ascii_off=qoff, options=opt)
    assert bam_decode.to_sam(_dev(handle, program, m, ops, names, qa, qoff, opt)) == sam.read_text().splitlines()


# ---- the smallest shapes where a field can go wrong

@pytest.mark.parametrize("program", ["blastn", "blastx", "blastp"])
@pytest.mark.parametrize("header", [True, False])
def test_no_records_and_one_record(handle, program, header):
    m, ops, names, qa, qoff = _case(program, seed=2)
    for n in (0, 1):
        opt, keep = _all(program, m[:n])
        got = _same(handle, program, m[:n], ops, names, qa, qoff, opt, write_header=header)
        assert (len(got) == 0) == (n == 0 and not header)


@pytest.mark.parametrize("program", ["blastn", "blastx", "tblastn"])
@pytest.mark.parametrize("seq", [capi.LX_SAM_SEQ_UNIQ, capi.LX_SAM_SEQ_ALWAYS])
def test_group_of_one_and_group_of_five(handle, program, seq):
    m, ops, names, qa, qoff = _case(program, seed=4, nq=8)
    m = m[:8].copy()
    m["n_qid"] = [0, 1, 1, 1, 1, 1, 2, 3]
    for k in (3, 4, 6):  # the same frame and query range as the row before: inside the group (no SEQ under uniq) and across its end (SEQ)
        for f in ("q_frame", "q_start", "q_end"):
            m[f][k] = m[f][k - 1]
    opt, keep = _all(program, m, seq=seq)
    _same(handle, program, m, ops, names, qa, qoff, opt)
    _, _, recs = bam_decode.decode(_dev(handle, program, m, ops, names, qa, qoff, opt))
    assert [r["flag"] & 256 for r in recs] == [0, 0, 256, 256, 256, 256, 0, 0]


@pytest.mark.parametrize("hard", [1, 0])
def test_sequence_lengths_and_empty_selections(handle, hard):
    for program in ("blastn", "blastx"):
        m, ops, names, qa, qoff = _case(program, seed=5)
        m = m[:6].copy()
        m["q_frame"] = [1, -1, 1, -1, 1, -1] if program == "blastn" else [1, -2, 3, -1, 2, -3]
        m["q_start"] = [3, 3, 7, 7, 2, 0]
        m["q_end"] = [4, 8, 7, 7, 10 ** 6, 10 ** 6]  # l_seq 1 and odd (blastn), start == end, an end beyond the frame
        opt, keep = _all(program, m, hard=hard)
        _same(handle, program, m, ops, names, qa, qoff, opt)


@pytest.mark.parametrize("program", ["blastn", "blastx", "blastp"])
def test_ops_shapes(handle, program):
    m, _, names, qa, qoff = _case(program, seed=6)
    m = m[:6].copy()
    pieces = [b"", b"DDMMMIMM", b"IMMMDDM", b"MMXMM", b"M", b"MIDMID"]  # none, D first, I first, a byte that is no op, one, every change
    ops, at = b"", []
    for p in pieces:
        at.append(len(ops))
        ops += p
    m["ops_off"], m["n_ops"] = at, [len(p) for p in pieces]
    for hard in (1, 0):
        opt, keep = _all(program, m, hard=hard)
        got = _same(handle, program, m, ops, names, qa, qoff, opt)
    _, _, recs = bam_decode.decode(got)
    if program != "blastp":
        assert recs[3]["cigar"] == () and recs[3]["bin"] == bam_decode.reg2bin(recs[3]["pos"], recs[3]["pos"] + 1)


@pytest.mark.parametrize("program", ["blastn", "blastx", "tblastx"])
def test_strands_and_frames(handle, program):
    m, ops, names, qa, qoff = _case(program, seed=7)
    m = m[:6].copy()
    m["q_frame"] = [1, -1, 1, -1, 1, -1] if program == "blastn" else [1, -1, 2, -2, 3, -3]
    m["q_start"], m["q_end"] = 2, 20
    if program == "tblastx":
        m["s_frame"] = [-1, 1, -2, 2, -3, 3]
    for seq, hard in ((capi.LX_SAM_SEQ_ALWAYS, 1), (capi.LX_SAM_SEQ_ALWAYS, 0)):
        opt, keep = _all(program, m, seq=seq, hard=hard)
        _same(handle, program, m, ops, names, qa, qoff, opt)


def test_query_ids_long_and_with_a_tab(handle):
    m, ops, names, qa, qoff = _case("blastn", seed=8)
    names["q_ids"][0] = "x" * 300 + " rest"  # l_read_name wraps to 45
    names["q_ids"][1] = "left\tright of the tab"
    names["q_ids"][2] = ""
    opt, keep = _all("blastn", m)
    got = _same(handle, "blastn", m, ops, names, qa, qoff, opt)
    assert b"x" * 300 + b"\0" in got


def test_taxa_per_subject_and_a_query_missing_from_the_lca_pairs(handle):
    m, ops, names, qa, qoff = _case("blastp", seed=9)
    m["n_sid"] = np.arange(len(m)) % 4  # tests.test_bam_encoding._tax: subjects with 1, 2, 0 and 1 taxa
    opt, keep = _all("blastp", m)
    _same(handle, "blastp", m, ops, names, qa, qoff, opt)
    # lcaOf's cursor only moves forward: a query that is not in the list takes it to the end, and every later query gets 0
    qid = np.ctypeslib.as_array(C.cast(opt.lca_qid, C.POINTER(C.c_uint64)), (opt.n_lca,)).copy()
    lca = np.ctypeslib.as_array(C.cast(opt.lca_tax, C.POINTER(C.c_uint32)), (opt.n_lca,)).copy()
    qid, lca = np.delete(qid, 2), np.delete(lca, 2)
    opt.lca_qid, opt.lca_tax, opt.n_lca = qid.ctypes.data, lca.ctypes.data, len(qid)
    got = _same(handle, "blastp", m, ops, names, qa, qoff, opt)
    _, _, recs = bam_decode.decode(got)
    lt = [dict((k, v) for k, _, v in r["tags"])["lt"] for r in recs]
    assert all(v == 0 for v, q in zip(lt, m["n_qid"]) if q >= 2)
    # no tree at all, and names without a tree
    opt2, keep2 = _all("blastp", m, tree=False)
    _same(handle, "blastp", m, ops, names, qa, qoff, opt2)


def test_number_edges_of_the_tags(handle):
    m, ops, names, qa, qoff = _case("blastn", seed=10)
    m = m[:6].copy()
    m["e_value"][:3] = [1e-180, 1e-40, 5.0]  # float 0, a float denormal, a plain value
    m["score"][0], m["identity"][0] = 300, 100.0  # the wrapping casts of ar and ai
    m["bit_score"][1] = 70000.5
    m["alignment_length"][2] = 0  # ap 0
    m["num_positives"][3], m["alignment_length"][3] = 2, 3  # 66.66... truncated
    m["num_positives"][4], m["alignment_length"][4] = 29, 29
    opt, keep = _all("blastn", m)
    _same(handle, "blastn", m, ops, names, qa, qoff, opt)


# ---- edges of the machinery

def _tiled(program, total, seed=12, seq=capi.LX_SAM_SEQ_ALWAYS):
    """`total` records: the rows of one _case repeated, every repetition with query ids of its own."""
    m, ops, names, qa, qoff = _case(program, seed=seed)
    nq, reps = len(names["q_ids"]), total // len(m) + 1
    big = np.tile(m, reps)
    big["n_qid"] += np.repeat(np.arange(reps, dtype=np.uint64) * nq, len(m))
    big["qry_id"] = big["n_qid"]
    names = dict(q_ids=[f"r{t}_{x}" for t in range(reps) for x in names["q_ids"]], q_lens=np.tile(names["q_lens"], reps), s_ids=names["s_ids"],
                 s_lens=names["s_lens"])
    return big[:total].copy(), ops, names, qa, np.tile(qoff, reps)


@pytest.mark.parametrize("n", [EMIT_RECORDS - 1, EMIT_RECORDS, EMIT_RECORDS + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_record_counts_around_the_workgroup_and_the_tile(handle, n):
    m, ops, names, qa, qoff = _tiled("blastx", n)
    opt, keep = _all("blastx", m, seq=capi.LX_SAM_SEQ_UNIQ)
    _same(handle, "blastx", m, ops, names, qa, qoff, opt)


@pytest.fixture(scope="module")
def three_ranges():
    m, ops, names, qa, qoff = _tiled("blastn", 3 * SCAN_TILE + 100)
    opt, keep = _all("blastn", m)
    ref = _host("blastn", m, ops, names, qa, qoff, opt)
    assert len(ref) > 3 * MIN_RANGE  # at least three ranges at the smallest budget
    return (m, ops, names, qa, qoff, opt, keep), ref


def test_ranges_change_the_cuts_not_the_bytes(three_ranges):
    (m, ops, names, qa, qoff, opt, keep), ref = three_ranges
    with capi.Handle(0) as h:
        h.set_option(capi.LX_OPT_BAM_RANGE_BYTES, MIN_RANGE)
        assert h.get_option(capi.LX_OPT_BAM_RANGE_BYTES) == MIN_RANGE
        assert _dev(h, "blastn", m, ops, names, qa, qoff, opt) == ref
        ms, launches = h.last_phase_ms(11)
        assert launches >= 4 and ms > 0  # groups + measure, then one emit per range
        h.set_option(capi.LX_OPT_BAM_RANGE_BYTES, 0)
        assert _dev(h, "blastn", m, ops, names, qa, qoff, opt) == ref
        for bad in (1, MIN_RANGE - 1, (2 << 30) + 1):
            with pytest.raises(capi.LambdaExtError):
                h.set_option(capi.LX_OPT_BAM_RANGE_BYTES, bad)


def test_a_record_larger_than_a_bgzf_block(handle, tmp_path):
    m, ops, names, qa, qoff = _case("blastn", seed=13)
    rng = np.random.default_rng(13)
    long_q = "".join("ACGTN"[i] for i in rng.integers(0, 5, 70_000)).encode()
    names["q_lens"] = names["q_lens"].copy()
    names["q_lens"][1] = len(long_q)
    qoff = qoff.copy()
    qoff[1] = len(qa)
    qa = qa + long_q
    opt, keep = _all("blastn", m, hard=0)
    got = _same(handle, "blastn", m, ops, names, qa, qoff, opt)
    assert len(got) > 2 * 65280
    args = (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"])
    handle.write_bam(tmp_path / "a.bam", *args, program="blastn", q_ascii=qa, q_ascii_off=qoff, options=opt)
    handle.write_records_bgzf(tmp_path / "b.bam", capi.LX_OUT_BAM, *args, program="blastn", q_ascii=qa, q_ascii_off=qoff, options=opt)
    assert (tmp_path / "a.bam").read_bytes() == (tmp_path / "b.bam").read_bytes()


# ---- refusals

def test_refusals_leave_the_handle_usable(handle):
    m, ops, names, qa, qoff = _case("blastx", seed=14)
    opt, keep = _all("blastx", m)
    bad_sid = m.copy()
    bad_sid["n_sid"][-1] = len(names["s_ids"])
    bad_ops = m.copy()
    bad_ops["ops_off"][-1] = len(ops) - int(bad_ops["n_ops"][-1]) + 1
    bad_tag = capi.output_options(sam_tags="AS xx")
    for rows, o in ((bad_sid, opt), (m, bad_tag), (bad_ops, opt)):
        with pytest.raises(capi.LambdaExtError) as e:
            _dev(handle, "blastx", rows, ops, names, qa, qoff, o)
        assert e.value.code == capi.LX_EINVAL
        _same(handle, "blastx", m, ops, names, qa, qoff, opt)
    with pytest.raises(capi.LambdaExtError) as e:
        _dev(handle, "blastx", m, ops, names, qa, qoff, bad_tag)
    assert "Unknown column specifier \"xx\"" in str(e.value)
    with pytest.raises(capi.LambdaExtError):
        _dev(handle, "blastq", m, ops, names, qa, qoff, opt)


# ---- the file writer

@pytest.mark.parametrize("program", PROGRAMS)
def test_write_bam_equals_write_records_bgzf(handle, tmp_path, program):
    m, ops, names, qa, qoff = _case(program, seed=21)
    opt, keep = _options(program, ALL_TAGS, capi.LX_SAM_SEQ_UNIQ, 1, True, m, 4)
    args = (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"])
    handle.write_bam(tmp_path / "a.bam", *args, program=program, q_ascii=qa, q_ascii_off=qoff, options=opt)
    handle.write_records_bgzf(tmp_path / "b.bam", capi.LX_OUT_BAM, *args, program=program, q_ascii=qa, q_ascii_off=qoff, options=opt)
    raw = (tmp_path / "a.bam").read_bytes()
    assert raw == (tmp_path / "b.bam").read_bytes()
    assert gzip.decompress(raw) == _render(capi.LX_OUT_BAM, program, m, ops, names, qa, qoff, opt)


def test_write_bam_over_three_ranges(three_ranges, tmp_path):
    (m, ops, names, qa, qoff, opt, keep), ref = three_ranges
    args = (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"])
    with capi.Handle(0) as h:
        h.write_records_bgzf(tmp_path / "b.bam", capi.LX_OUT_BAM, *args, program="blastn", q_ascii=qa, q_ascii_off=qoff, options=opt)
        h.set_option(capi.LX_OPT_BAM_RANGE_BYTES, MIN_RANGE)
        h.write_bam(tmp_path / "a.bam", *args, program="blastn", q_ascii=qa, q_ascii_off=qoff, options=opt)
        ms, launches = h.last_phase_ms(4)
        assert launches >= 3 and ms > 0  # the encoder ran once per range
    raw = (tmp_path / "a.bam").read_bytes()
    assert raw == (tmp_path / "b.bam").read_bytes()
    assert gzip.decompress(raw) == ref


# ---- determinism

def test_deterministic_across_calls_and_handles(handle):
    m, ops, names, qa, qoff = _tiled("tblastx", 700, seed=15)
    opt, keep = _all("tblastx", m)
    a = _dev(handle, "tblastx", m, ops, names, qa, qoff, opt)
    assert _dev(handle, "tblastx", m, ops, names, qa, qoff, opt) == a
    with capi.Handle(0) as h2:
        assert _dev(h2, "tblastx", m, ops, names, qa, qoff, opt) == a
    assert a == _host("tblastx", m, ops, names, qa, qoff, opt)


# ---- the front end

def test_cli_render_gpu_writes_the_same_file(tmp_path):
    from tests.test_gpu_bgzf import _small
    _small(tmp_path)
    cli = build.build_cli()

    def run(name, mode):
        r = subprocess.run([str(cli), "searchn", "-q", str(tmp_path / "r.fasta"), "-d", str(tmp_path / "g.fasta"), "-o", str(tmp_path / name),
                            "--version-to-outputfile", "0", "--render", mode], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stderr

    on_gpu, on_host = run("g.bam", "gpu"), run("h.bam", "host")
    assert "BAM records rendered and BGZF-compressed on the GPU" in on_gpu, on_gpu
    assert "rendered" not in on_host and "BGZF compression on the GPU" in on_host, on_host
    raw = (tmp_path / "g.bam").read_bytes()
    assert raw == (tmp_path / "h.bam").read_bytes()
    assert len(bam_decode.decode(gzip.decompress(raw))[2]) > 0
