"""GPU tests of the text record kernels (lx_text.hip) behind lx_render_text_dev / lx_write_text_dev: the bytes equal those of the host
writer (lx_render_records, lx_write_records_ex + lx_write_footer, lx_write_records_bgzf -- whose numbers are snprintf's) for .m8, .m9 and
.sam, for every program and option, at the smallest shapes where a field can go wrong, at the number formatter's ties and edges, at the
edges of the kernels' tiles and of the ranges, and through the front end's --render gpu."""
import gzip
import struct
import subprocess

import numpy as np
import pytest

from lambda_amd import build, capi
from tests.test_bam_encoding import ALL_TAGS, PROGRAMS, _case, _options

pytestmark = pytest.mark.gpu

M8, M9, SAM = capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS, capi.LX_OUT_SAM
# lx_text.h: records per emit workgroup (kTextEmitBlock = 256 threads, one wavefront of 64 per record), records per scan / size tile
EMIT_RECORDS = 256 // 64
SCAN_TILE = 2048
MIN_RANGE = 128 << 10
COMBOS = [(capi.LX_SAM_SEQ_ALWAYS, 1, True), (capi.LX_SAM_SEQ_UNIQ, 0, False), (capi.LX_SAM_SEQ_NEVER, 1, False), (capi.LX_SAM_SEQ_UNIQ, 1, True)]
# all 24 columns of kColumns in a shuffled order, one of them twice
ALL_COLUMNS = ("sframe qlen evalue sseqid staxids gaps qstart ppos bitscore qseqid lcataxid send frames length slen pident evalue mismatch "
               "qframe sstart nident score positive qend gapopen")
assert len(set(ALL_COLUMNS.split())) == 24 and len(ALL_COLUMNS.split()) == 25


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


def _dev(h, fmt, program, m, ops, names, qa, qoff, opt, write_header=True, footer=-1):
    return h.render_text(fmt, m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program, write_header=write_header,
                         q_ascii=qa, q_ascii_off=qoff, options=opt, footer_records=footer)


def _host(fmt, program, m, ops, names, qa, qoff, opt, write_header=True, footer=-1):
    return capi.render_records(fmt, m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program=program,
                               write_header=write_header, q_ascii=qa, q_ascii_off=qoff, options=opt, footer_records=footer)


def _same(h, fmt, program, m, ops, names, qa, qoff, opt, write_header=True, footer=-1):
    dev = _dev(h, fmt, program, m, ops, names, qa, qoff, opt, write_header, footer)
    ref = _host(fmt, program, m, ops, names, qa, qoff, opt, write_header, footer)
    assert dev.split(b"\n") == ref.split(b"\n")  # (text: the first line that differs reads better than two blobs)
    assert dev == ref
    return dev


def _opt(program, m, columns=None, tags=ALL_TAGS, seq=capi.LX_SAM_SEQ_ALWAYS, hard=1, tree=True, ns=4):
    """Options for all three formats at once: the columns for the tabular ones, the tags and clipping for SAM, the taxonomy for both."""
    opt, keep = _options(program, tags, seq, hard, tree, m, ns)
    if columns is not None:
        opt.columns = columns.encode()
    opt.db_name = b"some/index.lba"
    return opt, keep


def _all_formats(h, program, m, ops, names, qa, qoff, opt, **kw):
    return [_same(h, fmt, program, m, ops, names, qa, qoff, opt, **kw) for fmt in (M8, M9, SAM)]


# ---- formats and options

@pytest.mark.parametrize("program", PROGRAMS)
def test_m8_standard_columns(handle, program):
    m, ops, names, qa, qoff = _case(program, seed=PROGRAMS.index(program) + 40)
    got = _same(handle, M8, program, m, ops, names, qa, qoff, None)
    assert got.count(b"\n") == len(m) and all(line.count(b"\t") == 11 for line in got.splitlines())


@pytest.mark.parametrize("tree", [True, False])
@pytest.mark.parametrize("program", PROGRAMS)
def test_m9_all_columns_shuffled_and_one_repeated(handle, program, tree):
    m, ops, names, qa, qoff = _case(program, seed=PROGRAMS.index(program) + 50)
    m["n_sid"] = np.arange(len(m)) % 4  # tests.test_bam_encoding._tax: subjects with 1, 2, 0 and 1 taxa
    opt, keep = _opt(program, m, ALL_COLUMNS, tree=tree)
    groups = len(set(m["n_qid"].tolist()))
    got = _same(handle, M9, program, m, ops, names, qa, qoff, opt, footer=groups)
    assert got.count(b"# Fields: ") == groups and got.endswith(b"# BLAST processed %d queries\n" % groups)
    opt.version_to_output, opt.version = 1, b"9.9.9"
    _same(handle, M9, program, m, ops, names, qa, qoff, opt)
    _same(handle, M8, program, m, ops, names, qa, qoff, opt, footer=3)  # (no footer in .m8)


@pytest.mark.parametrize("tags", [ALL_TAGS, None], ids=["all", "default"])
@pytest.mark.parametrize("seq,hard,tree", COMBOS)
@pytest.mark.parametrize("program", PROGRAMS)
def test_sam_equals_the_host_writer(handle, program, seq, hard, tree, tags):
    m, ops, names, qa, qoff = _case(program, seed=PROGRAMS.index(program) * 7 + seq)
    if tags is None:
        opt, keep = _options(program, "AS NM ae ai qf", seq, hard, tree, m, 4)
        opt.sam_tags = None
    else:
        opt, keep = _options(program, tags, seq, hard, tree, m, 4)
    _same(handle, SAM, program, m, ops, names, qa, qoff, opt)
    opt.sam_with_ref_header = 0
    _same(handle, SAM, program, m, ops, names, qa, qoff, opt)


# ---- the smallest shapes where a field can go wrong

@pytest.mark.parametrize("program", ["blastn", "blastx", "blastp"])
@pytest.mark.parametrize("header", [True, False])
def test_no_records_and_one_record(handle, program, header):
    m, ops, names, qa, qoff = _case(program, seed=2)
    for n in (0, 1):
        opt, keep = _opt(program, m[:n], ALL_COLUMNS)
        m8, m9, sam = _all_formats(handle, program, m[:n], ops, names, qa, qoff, opt, write_header=header)
        assert (len(m8) == 0) == (n == 0) and (len(sam) == 0) == (n == 0 and not header)
        assert _same(handle, M9, program, m[:n], ops, names, qa, qoff, opt, write_header=header, footer=n).endswith(b" queries\n")


@pytest.mark.parametrize("program", ["blastn", "blastx", "tblastn"])
@pytest.mark.parametrize("seq", [capi.LX_SAM_SEQ_UNIQ, capi.LX_SAM_SEQ_ALWAYS])
def test_group_of_one_and_group_of_five(handle, program, seq):
    m, ops, names, qa, qoff = _case(program, seed=4, nq=8)
    m = m[:8].copy()
    m["n_qid"] = [0, 1, 1, 1, 1, 1, 2, 3]
    for k in (3, 4, 6):  # the same frame and query range as the row before: inside the group (no SEQ under uniq) and across its end (SEQ)
        for f in ("q_frame", "q_start", "q_end"):
            m[f][k] = m[f][k - 1]
    opt, keep = _opt(program, m, ALL_COLUMNS, seq=seq)
    m8, m9, sam = _all_formats(handle, program, m, ops, names, qa, qoff, opt, write_header=False)
    assert [int(x.split()[1]) for x in m9.splitlines() if x.endswith(b"hits found")] == [1, 5, 1, 1]
    lines = sam.splitlines()
    assert [int(x.split(b"\t")[1]) & 256 for x in lines] == [0, 0, 256, 256, 256, 256, 0, 0]
    if program != "tblastn":
        stars = [x.split(b"\t")[9] == b"*" for x in lines]
        if seq == capi.LX_SAM_SEQ_UNIQ:  # suppressed inside the group, written again for the next group's first record
            assert stars[3] and stars[4] and not (stars[0] or stars[1] or stars[6] or stars[7])
        else:
            assert not any(stars)


@pytest.mark.parametrize("hard", [1, 0])
def test_sequence_lengths_and_empty_selections(handle, hard):
    for program in ("blastn", "blastx"):
        m, ops, names, qa, qoff = _case(program, seed=5)
        m = m[:6].copy()
        m["q_frame"] = [1, -1, 1, -1, 1, -1] if program == "blastn" else [1, -2, 3, -1, 2, -3]
        m["q_start"] = [3, 3, 7, 7, 2, 0]
        m["q_end"] = [4, 8, 7, 7, 10 ** 6, 10 ** 6]  # one letter, start == end, an end beyond the frame (coordinates that wrap)
        opt, keep = _opt(program, m, ALL_COLUMNS, hard=hard)
        _all_formats(handle, program, m, ops, names, qa, qoff, opt)


@pytest.mark.parametrize("program", ["blastn", "blastx", "blastp"])
def test_ops_shapes(handle, program):
    m, _, names, qa, qoff = _case(program, seed=6)
    m = m[:7].copy()
    pieces = [b"", b"DDMMMIMM", b"IMMMDDM", b"MMXMM", b"M", b"MIDMID", b""]  # none, D first, I first, a byte that is no op, one, every change
    ops, at = b"", []
    for p in pieces:
        at.append(len(ops))
        ops += p
    m["ops_off"], m["n_ops"] = at, [len(p) for p in pieces]
    m["q_frame"][1:3] = [-1, 1] if program != "blastp" else 0  # D first on the minus strand: the reversed CIGAR ends with it
    m["q_start"][6], m["q_end"][6] = 0, names["q_lens"][m["n_qid"][6]]  # no ops and no clips: an empty CIGAR, OC "*"
    for hard in (1, 0):
        opt, keep = _opt(program, m, ALL_COLUMNS, hard=hard)
        m8, m9, sam = _all_formats(handle, program, m, ops, names, qa, qoff, opt, write_header=False)
    if program != "blastp":
        assert sam.splitlines()[3].split(b"\t")[5] == b"*"


@pytest.mark.parametrize("program", PROGRAMS)
def test_strands_and_frames_of_the_coordinate_columns(handle, program):
    m, ops, names, qa, qoff = _case(program, seed=7)
    m = m[:7].copy()
    q_trans, s_trans = program in ("blastx", "tblastx"), program in ("tblastn", "tblastx")
    m["q_frame"] = [1, -1, 2, -2, 3, -3, 1] if q_trans else [1, -1, 1, -1, 1, -1, 1] if program == "blastn" else 0
    m["s_frame"] = [-1, 1, -2, 2, -3, 3, -1] if s_trans else 0
    m["q_start"], m["q_end"] = 2, 20
    m["s_start"], m["s_end"] = [0, 1, 2, 3, 5, 8, 13], [18, 19, 20, 21, 23, 26, 31]
    cols = "qseqid sseqid qstart qend sstart send frames qframe sframe qlen slen"
    for hard in (1, 0):
        opt, keep = _opt(program, m, cols, hard=hard)
        m8, m9, sam = _all_formats(handle, program, m, ops, names, qa, qoff, opt)
    rows = [x.split(b"\t") for x in m8.splitlines()]
    if program == "blastn":  # the mirrored query, the swapped subject
        assert all((int(r[2]) < int(r[3])) and (int(r[4]) > int(r[5])) == (f < 0) for r, f in zip(rows, m["q_frame"]))
    if s_trans:
        assert all((int(r[4]) > int(r[5])) == (f < 0) for r, f in zip(rows, m["s_frame"]))


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def test_numbers_at_the_formatters_ties_and_edges(handle):
    """24 rows: e_value, bit_score and identity at the ties and edges of the formatter; ppos through 12.5, 37.5 and 99.995-like quotients."""
    m, ops, names, qa, qoff = _case("blastn", seed=10, nq=12)
    m = np.tile(m, 3)[:24].copy()
    m["n_qid"] = np.arange(24) // 2
    smallest_float = struct.unpack("<f", struct.pack("<I", 1))[0]
    e_values = [1.25, 1.75, 9.95e-5, 9.96e-10, 5e-324, 1.7976931348623157e308, 0.0, -0.0, 1e-5, 1e-4, 999999.5, 123456.703125, smallest_float,
                smallest_float / 2, smallest_float * 0.75, float("inf"), float("nan"), 2.2250738585072014e-308, 1e-180, 1e-40, 9.5, 0.00095,
                f32(1e-5), 3.4028235677973366e38]
    # (SAM's AS casts the bit score to an integer: the values stay where that cast is defined; the table below goes beyond)
    bit_scores = [0.25, 0.75, 0.05, 0.15, 0.35, -0.04, 99.95, 99.949999, 0.0, -0.0, 2147483647.75, -2147483647.75, 5e-324, 12345.65, 0.5, 1.5, 2.5,
                  70000.5, 65535.99, 65536.0, 300.45, 1e-300, 999.95, 0.95]
    identities = [0.125, 0.375, 99.995, 100.0, 0.0, 12.5, 37.5, 62.5, 87.5, 0.005, 0.015, 0.025, 99.99, 50.0, 33.333332, 66.666664, 1.0e-45,
                  255.5, 256.0, 300.0, 12.345, 12.355, 99.5, 7.0]
    assert len(e_values) == len(bit_scores) == len(identities) == 24
    m["e_value"], m["bit_score"], m["identity"] = e_values, bit_scores, np.array(identities, np.float32)
    # ppos = 100 * positives / length: 12.5 and 37.5, exact ties of %.2f (1/800 = 0.125 %, 3/800 = 0.375 %, k/1600, k/32), quotients whose
    # double lies a hair off a tie or off 100 (19999/20000 = 99.995, 1/3, 2/3), 0 / 0, and more positives than columns
    # (SAM's ap casts ppos to an integer: the quotients stay where that cast is defined; the table below goes beyond)
    pairs = [(1, 8), (3, 8), (19999, 20000), (1, 800), (3, 800), (1, 1600), (3, 1600), (1, 3), (2, 3), (0, 0), (5, 0), (29, 29), (1, 16), (3, 16),
             (39999, 40000), (199999, 200000), (7, 3), (1, 2 ** 31 - 1), (300, 1), (-3, 8), (1, 32), (3, 32), (1001, 1600), (333, 800)]
    assert len(pairs) == 24
    m["num_positives"], m["alignment_length"] = [p for p, _ in pairs], [a for _, a in pairs]
    cols = "qseqid evalue bitscore pident ppos positive length"
    opt, keep = _opt("blastn", m, cols)
    m8, m9, sam = _all_formats(handle, "blastn", m, ops, names, qa, qoff, opt)
    rows = [x.split(b"\t") for x in m8.splitlines()]
    assert [r[1] for r in rows[:6]] == [b"1.2e+00", b"1.8e+00", b"1.0e-04", b"1.0e-09", b"4.9e-324", b"1.8e+308"]
    assert [r[2] for r in rows[:6]] == [b"0.2", b"0.8", b"0.1", b"0.1", b"0.3", b"-0.0"]
    assert [r[3] for r in rows[:3]] == [b"0.12", b"0.38", b"100.00"] and [r[4] for r in rows[:3]] == [b"12.50", b"37.50", b"100.00"]
    ae = [dict(t.split(b":", 2)[::2] for t in x.split(b"\t")[11:])[b"ae"] for x in sam.splitlines() if not x.startswith(b"@")]
    assert ae[8:13] == [b"1e-05", b"0.0001", b"1e+06", b"123457", b"1.4013e-45"] and ae[6:8] == [b"0", b"-0"]
    # the ends of the domain, in the tabular formats (no integer casts there)
    m["bit_score"][:4] = [1e15 - 0.125, -(1e15 - 0.125), 999999999999999.9, 562949953421311.95]
    m["identity"][:2] = [9.99999e14, -9.99999e14]
    m["num_positives"][4:6], m["alignment_length"][4:6] = [2 ** 31 - 1, -2 ** 31], [1, 1]
    for fmt in (M8, M9):
        got = _same(handle, fmt, "blastn", m, ops, names, qa, qoff, opt)
    assert b"\t999999999999999.9\t" in got and b"\t-999999999999999.9\t" in got


def test_ids_with_and_without_a_second_word_empty_and_long(handle):
    m, ops, names, qa, qoff = _case("blastn", seed=8)
    names["q_ids"][0] = "x" * 300 + " rest of the line"  # longer than the stage of a wavefront
    names["q_ids"][1] = "left\tright of the tab"
    names["q_ids"][2] = ""
    names["q_ids"][3] = "oneword"
    names["s_ids"][0] = "y" * 300
    names["s_ids"][1] = ""
    names["s_ids"][2] = "sub ject"
    opt, keep = _opt("blastn", m, "qseqid sseqid qseqid evalue")
    m8, m9, sam = _all_formats(handle, "blastn", m, ops, names, qa, qoff, opt)
    assert b"# Query: " + b"x" * 300 + b" rest of the line\n" in m9 and b"# Query: \n" in m9 and b"# Query: left\tright of the tab\n" in m9


def test_a_sequence_longer_than_many_stages(handle):
    m, ops, names, qa, qoff = _case("blastn", seed=13)
    rng = np.random.default_rng(13)
    long_q = "".join("ACGTN"[i] for i in rng.integers(0, 5, 5_000)).encode()
    names["q_lens"] = names["q_lens"].copy()
    names["q_lens"][1] = len(long_q)
    qoff = qoff.copy()
    qoff[1] = len(qa)
    qa = qa + long_q
    opt, keep = _opt("blastn", m, hard=0)
    _same(handle, SAM, "blastn", m, ops, names, qa, qoff, opt)


def test_taxa_and_a_query_missing_from_the_lca_pairs(handle):
    import ctypes as C
    m, ops, names, qa, qoff = _case("blastp", seed=9)
    m["n_sid"] = np.arange(len(m)) % 4
    opt, keep = _opt("blastp", m, "qseqid staxids lcataxid")
    qid = np.ctypeslib.as_array(C.cast(opt.lca_qid, C.POINTER(C.c_uint64)), (opt.n_lca,)).copy()
    lca = np.ctypeslib.as_array(C.cast(opt.lca_tax, C.POINTER(C.c_uint32)), (opt.n_lca,)).copy()
    qid, lca = np.delete(qid, 2), np.delete(lca, 2)
    opt.lca_qid, opt.lca_tax, opt.n_lca = qid.ctypes.data, lca.ctypes.data, len(qid)
    m8, m9, sam = _all_formats(handle, "blastp", m, ops, names, qa, qoff, opt)
    assert all(x.split(b"\t")[2] == b"0" for x, q in zip(m8.splitlines(), m["n_qid"]) if q >= 2)


def test_tabular_formats_do_not_read_the_ops(handle):
    """As in the host writer: a front end that writes .m8 keeps no ops, and the rows' ops_off / n_ops point nowhere."""
    m, ops, names, qa, qoff = _case("blastx", seed=16)
    opt, keep = _opt("blastx", m, ALL_COLUMNS)
    for fmt in (M8, M9):
        assert _dev(handle, fmt, "blastx", m, b"", names, qa, qoff, opt) == _host(fmt, "blastx", m, ops, names, qa, qoff, opt)
    with pytest.raises(capi.LambdaExtError):
        _dev(handle, SAM, "blastx", m, b"", names, qa, qoff, opt)


# ---- edges of the machinery

def _tiled(program, total, seed=12):
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
    opt, keep = _opt("blastx", m, ALL_COLUMNS, seq=capi.LX_SAM_SEQ_UNIQ)
    _all_formats(handle, "blastx", m, ops, names, qa, qoff, opt)


@pytest.fixture(scope="module")
def three_ranges():
    m, ops, names, qa, qoff = _tiled("blastn", 3 * SCAN_TILE + 100)
    opt, keep = _opt("blastn", m, ALL_COLUMNS)
    groups = len(set(m["n_qid"].tolist()))
    refs = {fmt: _host(fmt, "blastn", m, ops, names, qa, qoff, opt, footer=groups) for fmt in (M8, M9, SAM)}
    assert all(len(r) > 3 * MIN_RANGE for r in refs.values())  # at least three ranges at the smallest budget
    return (m, ops, names, qa, qoff, opt, keep, groups), refs


def test_ranges_change_the_cuts_not_the_bytes(three_ranges):
    (m, ops, names, qa, qoff, opt, keep, groups), refs = three_ranges
    with capi.Handle(0) as h:
        h.set_option(capi.LX_OPT_BAM_RANGE_BYTES, MIN_RANGE)
        for fmt in (M8, M9, SAM):
            assert _dev(h, fmt, "blastn", m, ops, names, qa, qoff, opt, footer=groups) == refs[fmt]
            ms, launches = h.last_phase_ms(12)
            assert launches >= 4 and ms > 0  # groups, numbers + measure, then one emit per range
        h.set_option(capi.LX_OPT_BAM_RANGE_BYTES, 0)
        assert _dev(h, M9, "blastn", m, ops, names, qa, qoff, opt, footer=groups) == refs[M9]


@pytest.mark.parametrize("fmt,ext", [(M8, "m8"), (M9, "m9"), (SAM, "sam")])
def test_written_files_over_three_ranges(three_ranges, tmp_path, fmt, ext):
    (m, ops, names, qa, qoff, opt, keep, groups), refs = three_ranges
    args = (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"])
    kw = dict(program="blastn", q_ascii=qa, q_ascii_off=qoff, options=opt)
    plain, packed = tmp_path / f"host.{ext}", tmp_path / f"host.{ext}.gz"
    capi.write_records(plain, fmt, *args, **kw)
    capi.write_footer(plain, fmt, groups)
    with capi.Handle(0) as h:
        h.write_records_bgzf(packed, fmt, *args, footer_records=groups, **kw)
        h.set_option(capi.LX_OPT_BAM_RANGE_BYTES, MIN_RANGE)
        h.write_text(tmp_path / f"dev.{ext}", fmt, *args, bgzf=False, footer_records=groups, **kw)
        h.write_text(tmp_path / f"dev.{ext}.gz", fmt, *args, bgzf=True, footer_records=groups, **kw)
        ms, launches = h.last_phase_ms(4)
        assert launches >= 3 and ms > 0  # the encoder ran once per range
    assert plain.read_bytes() == refs[fmt] == (tmp_path / f"dev.{ext}").read_bytes()
    raw = (tmp_path / f"dev.{ext}.gz").read_bytes()
    assert raw == packed.read_bytes()
    assert gzip.decompress(raw) == refs[fmt]


@pytest.mark.parametrize("n", [0, 3])
def test_written_files_of_no_and_few_records(handle, tmp_path, n):
    m, ops, names, qa, qoff = _case("blastx", seed=21)
    m = m[:n]
    args = (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"])
    kw = dict(program="blastx", q_ascii=qa, q_ascii_off=qoff, options=None)
    for fmt in (M8, M9, SAM):
        ref = _host(fmt, "blastx", m, ops, names, qa, qoff, None, footer=n)
        handle.write_records_bgzf(tmp_path / "host.gz", fmt, *args, footer_records=n, **kw)
        handle.write_text(tmp_path / "dev.txt", fmt, *args, bgzf=False, footer_records=n, **kw)
        handle.write_text(tmp_path / "dev.gz", fmt, *args, bgzf=True, footer_records=n, **kw)
        assert (tmp_path / "dev.txt").read_bytes() == ref
        assert (tmp_path / "dev.gz").read_bytes() == (tmp_path / "host.gz").read_bytes()
        assert gzip.decompress((tmp_path / "dev.gz").read_bytes()) == ref


# ---- refusals

def test_refusals_leave_the_handle_usable(handle):
    m, ops, names, qa, qoff = _case("blastx", seed=14)
    opt, keep = _opt("blastx", m, ALL_COLUMNS)
    bad_sid = m.copy()
    bad_sid["n_sid"][-1] = len(names["s_ids"])
    bad_ops = m.copy()
    bad_ops["ops_off"][-1] = len(ops) - int(bad_ops["n_ops"][-1]) + 1
    bad_num = m.copy()
    bad_num["bit_score"][0] = 1e15
    bad_col = capi.output_options(columns="qseqid btop")
    for fmt, rows, o in ((M8, bad_sid, opt), (M9, m, bad_col), (SAM, bad_ops, opt), (M8, bad_num, opt), (capi.LX_OUT_BAM, m, opt)):
        with pytest.raises(capi.LambdaExtError) as e:
            _dev(handle, fmt, "blastx", rows, ops, names, qa, qoff, o)
        assert e.value.code == capi.LX_EINVAL
        _same(handle, M9, "blastx", m, ops, names, qa, qoff, opt)
    with pytest.raises(capi.LambdaExtError) as e:
        _dev(handle, M8, "blastx", m, ops, names, qa, qoff, bad_col)
    assert "Unknown column specifier \"btop\"" in str(e.value)


# ---- determinism

def test_two_calls_on_one_handle_give_the_same_bytes(handle):
    m, ops, names, qa, qoff = _tiled("tblastx", 700, seed=15)
    opt, keep = _opt("tblastx", m, ALL_COLUMNS)
    for fmt in (M8, M9, SAM):
        a = _dev(handle, fmt, "tblastx", m, ops, names, qa, qoff, opt)
        assert _dev(handle, fmt, "tblastx", m, ops, names, qa, qoff, opt) == a
        assert a == _host(fmt, "tblastx", m, ops, names, qa, qoff, opt)


# ---- the front end

@pytest.mark.parametrize("name", ["x.m8", "x.sam.gz"])
def test_cli_render_gpu_writes_the_same_file(tmp_path, name):
    from tests.test_gpu_bgzf import _small
    _small(tmp_path)
    cli = build.build_cli()

    def run(out, mode):
        r = subprocess.run([str(cli), "searchn", "-q", str(tmp_path / "r.fasta"), "-d", str(tmp_path / "g.fasta"), "-o", str(tmp_path / out),
                            "--version-to-outputfile", "0", "--render", mode], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stderr

    on_gpu, on_host = run("gpu_" + name, "gpu"), run("host_" + name, "host")
    assert "records rendered" in on_gpu and "on the GPU" in on_gpu, on_gpu
    assert "rendered" not in on_host, on_host
    raw = (tmp_path / ("gpu_" + name)).read_bytes()
    assert raw == (tmp_path / ("host_" + name)).read_bytes()
    assert len((gzip.decompress(raw) if name.endswith(".gz") else raw).splitlines()) > 0
