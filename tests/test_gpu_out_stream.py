"""lx_out_* on the device: compressed .m8 / .m9 / .sam files and BAM written piece by piece -- rendered on the host, on the device, or
in turns -- are byte for byte the files lx_write_records_bgzf and lx_write_text_dev / lx_write_bam_dev make of the whole list.  The
cuts are searched over the stream's size in front of every query (from lx_render_records), so that a 65 280-byte block boundary
falls inside a piece, exactly on a piece's end, and behind several pieces that together stay below one block."""
import numpy as np
import pytest

from lambda_amd import capi
from tests import out_stream_cases as oc
from tests.test_bam_encoding import ALL_TAGS, _case, _options, _render

pytestmark = pytest.mark.gpu
BLOCK = 65280
NQ, NS = 1000, 30
FORMATS = {"m8": capi.LX_OUT_BLAST_TAB, "m9": capi.LX_OUT_BLAST_TAB_COMMENTS, "sam": capi.LX_OUT_SAM, "bam": capi.LX_OUT_BAM}
H, D = capi.LX_RENDER_HOST, capi.LX_RENDER_DEV


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


@pytest.fixture(scope="module")
def case():
    return _case("blastn", seed=21, nq=NQ, ns=NS)  # about 2 500 records


def _opt(fmt, m):
    opt, keep = _options("blastn", ALL_TAGS, capi.LX_SAM_SEQ_UNIQ, 1, True, m, NS)
    if fmt in (capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS):
        opt.columns = b"std qlen slen staxids lcataxid"
    return opt, keep


def _group_size(fmt, case, opt, lca, q):
    """Bytes of query q's records in the stream."""
    m, ops, names, qa, qoff = case
    p = oc.piece(m, names, qoff, lca, q, q + 1)
    o = capi.OutputOptions.from_buffer_copy(opt)
    o.lca_qid, o.lca_tax, o.n_lca = p["lca_qid"].ctypes.data, p["lca_tax"].ctypes.data, len(p["lca_qid"])
    return len(capi.render_records(fmt, p["bms"], ops, p["q_ids"], p["q_lens"], names["s_ids"], names["s_lens"], program="blastn",
                                   write_header=False, q_ascii=qa, q_ascii_off=p["q_ascii_off"], options=o))


def _prefix(fmt, case, opt):
    """prefix[q] = bytes of the stream in front of query q's records (prefix[NQ]: in front of the footer)."""
    m, ops, names, qa, qoff = case
    lca = oc.lca_pairs(opt)
    header = len(_render(fmt, "blastn", m[:0], ops, names, qa, qoff, opt))
    return np.concatenate([[header], header + np.cumsum([_group_size(fmt, case, opt, lca, q) for q in range(NQ)])])


def _longer(ids, g, x):
    """The ids with the first word of ids[g] x characters longer."""
    return ids[:g] + [ids[g].replace(" ", "x" * x + " ", 1)] + ids[g + 1:]


def _boundary_on_a_cut(fmt, case, opt):
    """The case with two query ids lengthened so that the stream in front of some query is exactly one block; that query's number."""
    m, ops, names, qa, qoff = case
    lca = oc.lca_pairs(opt)
    prefix = _prefix(fmt, case, opt)
    q = int(np.searchsorted(prefix, BLOCK, side="right")) - 1  # the last query whose records begin inside the first block
    need = BLOCK - int(prefix[q])
    if need == 0:
        return case, q
    ids = list(names["q_ids"])
    # bytes per character: the id's first word stands once per record, and the whole id in .m9's comment line
    per = {g: _group_size(fmt, (m, ops, dict(names, q_ids=_longer(ids, g, 1)), qa, qoff), opt, lca, g) - int(prefix[g + 1] - prefix[g])
           for g in range(max(0, q - 12), q)}
    for a in per:
        for b in per:
            for x in range(need // per[a] + 1):
                if a != b and (need - per[a] * x) % per[b] == 0:
                    grown = (m, ops, dict(names, q_ids=_longer(_longer(ids, a, x), b, (need - per[a] * x) // per[b])), qa, qoff)
                    assert int(_prefix(fmt, grown, opt)[q]) == BLOCK
                    return grown, q
    raise AssertionError("no pair of ids reaches the block boundary")


def _one_shot(handle, tmp_path, fmt, case, opt):
    """The yardsticks: the host-rendered file and the device-rendered one (which agree)."""
    m, ops, names, qa, qoff = case
    a, b = tmp_path / "host.gz", tmp_path / "dev.gz"
    args = (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"])
    kw = dict(program="blastn", q_ascii=qa, q_ascii_off=qoff, options=opt)
    handle.write_records_bgzf(a, fmt, *args, footer_records=NQ, **kw)
    if fmt == capi.LX_OUT_BAM:
        handle.write_bam(b, *args, **kw)
    else:
        handle.write_text(b, fmt, *args, bgzf=True, footer_records=NQ, **kw)
    assert a.read_bytes() == b.read_bytes()
    return a.read_bytes()


def _sides(n):
    return {"host": H, "device": D, "in_turns": [(D, H)[i % 2] for i in range(n)], "in_turns_host_first": [(H, D)[i % 2] for i in range(n)]}


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_a_boundary_inside_a_piece_and_behind_small_pieces(handle, tmp_path, case, fmt):
    m = case[0]
    opt, keep = _opt(FORMATS[fmt], m)
    prefix = _prefix(FORMATS[fmt], case, opt)
    assert prefix[NQ] > 2 * BLOCK  # more than two blocks of stream
    want = _one_shot(handle, tmp_path, FORMATS[fmt], case, opt)
    # two pieces, each with a block boundary strictly inside (the stream is more than two blocks long)
    halves = [int(np.searchsorted(prefix, prefix[NQ] // 2))]
    for lo, hi in zip([0] + halves, halves + [NQ]):
        assert prefix[lo] // BLOCK < (prefix[hi] - 1) // BLOCK
    assert all(prefix[c] % BLOCK for c in halves)  # (and the cut itself is on none)
    # twenty pieces of one query each that together, header included, stay below one block; an empty piece among them; then the rest
    assert prefix[20] < BLOCK
    small = list(range(1, 11)) + [10] + list(range(11, 21))
    for cuts in (halves, small):
        for side, where in _sides(len(cuts) + 1).items():
            got = oc.write_in_pieces(handle, tmp_path / "pieces.gz", FORMATS[fmt], case, opt, cuts, where, bgzf=True, footer=NQ)
            assert got == want, (fmt, cuts[:3], side)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_a_boundary_exactly_on_a_piece_end(handle, tmp_path, case, fmt):
    opt, keep = _opt(FORMATS[fmt], case[0])
    grown, q = _boundary_on_a_cut(FORMATS[fmt], case, opt)
    want = _one_shot(handle, tmp_path, FORMATS[fmt], grown, opt)
    for cuts in ([q], [q // 2, q, q + 1, (q + NQ) // 2]):
        for side, where in _sides(len(cuts) + 1).items():
            got = oc.write_in_pieces(handle, tmp_path / "pieces.gz", FORMATS[fmt], grown, opt, cuts, where, bgzf=True, footer=NQ)
            assert got == want, (fmt, cuts, side)


def test_plain_text_files_rendered_on_the_device(handle, tmp_path, case):
    m, ops, names, qa, qoff = case
    for fmt in (capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS, capi.LX_OUT_SAM):
        opt, keep = _opt(fmt, m)
        want = _render(fmt, "blastn", m, ops, names, qa, qoff, opt, footer=NQ)
        for where in (D, [D, H, D, H]):
            assert oc.write_in_pieces(handle, tmp_path / "pieces.txt", fmt, case, opt, [1, 400, 400], where, footer=NQ) == want


def test_refusals_and_phase_times(handle, tmp_path, case):
    m, ops, names, qa, qoff = case
    p = tmp_path / "o.bam"
    with pytest.raises(capi.LambdaExtError, match='Unknown column specifier "zz"'):
        capi.Out(handle, p, capi.LX_OUT_BAM, names["s_ids"], names["s_lens"], program="blastn", options=capi.output_options(sam_tags="AS zz"))
    assert not p.exists()
    lca = oc.lca_pairs(None)
    first, rest = oc.piece(m, names, qoff, lca, 0, 600), oc.piece(m, names, qoff, lca, 600, NQ)
    with capi.Out(handle, p, capi.LX_OUT_BAM, names["s_ids"], names["s_lens"], program="blastn") as out:
        out.append(D, first["bms"], ops, first["q_ids"], first["q_lens"], q_ascii=qa, q_ascii_off=first["q_ascii_off"])
        assert handle.last_phase_ms(11)[1] > 0 and handle.last_phase_ms(4)[1] > 0  # the render kernels and the encoder ran in this append
        size = p.stat().st_size
        with pytest.raises(capi.LambdaExtError) as e:  # records that name a query the piece does not have: refused, the file as it was
            out.append(D, rest["bms"], ops, rest["q_ids"][:3], rest["q_lens"][:3], q_ascii=qa, q_ascii_off=rest["q_ascii_off"][:3])
        assert e.value.code == capi.LX_EINVAL
        out.append(D, m[:0], b"", [], [])
        out.append(H, rest["bms"], ops, rest["q_ids"], rest["q_lens"], q_ascii=qa, q_ascii_off=rest["q_ascii_off"])
        out.close()
    assert p.stat().st_size > size
    handle.write_bam(tmp_path / "whole.bam", m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], program="blastn", q_ascii=qa,
                     q_ascii_off=qoff)
    assert p.read_bytes() == (tmp_path / "whole.bam").read_bytes()
