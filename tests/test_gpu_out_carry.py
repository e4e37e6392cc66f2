"""The block-carry loop of the device writers at the three places where its callers differ: an initial carry of a block or more (a
header longer than one 65 280-byte BGZF block), no ranges at all (no record), and a tail behind the last range (the .m9 footer).  The
files of lx_write_bam_dev, lx_write_text_dev(bgzf=1) and of lx_out_append with LX_RENDER_DEV are byte for byte the host writer's."""
import pytest

from lambda_amd import capi
from tests import out_stream_cases as oc
from tests.test_bam_encoding import ALL_TAGS, _case, _options, _render

pytestmark = pytest.mark.gpu
BLOCK = 65280
NS = 3000  # subjects with 30-character ids: a reference list, and a list of @SQ lines, of more than one block
COUNTS = [0, 1, 5]
FORMATS = {"bam": capi.LX_OUT_BAM, "sam": capi.LX_OUT_SAM}


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


@pytest.fixture(scope="module")
def case():
    m, ops, names, qa, qoff = _case("blastn", seed=0, nq=2, ns=NS)
    names = dict(names, s_ids=[f"subject_{j:06d}_{'x' * 15} desc" for j in range(NS)])
    assert all(len(s.split()[0]) == 30 for s in names["s_ids"])
    per = [int((m["n_qid"] == q).sum()) for q in range(2)]
    assert per[0] >= 2 and per[1] >= 3, per
    return m, ops, names, qa, qoff


def _records(case, count):
    """The case with `count` records: none, the first one, or two of the first query and three of the second."""
    m, ops, names, qa, qoff = case
    first = int((m["n_qid"] == 0).sum())
    part = {0: m[:0], 1: m[:1], 5: m[[0, 1, first, first + 1, first + 2]]}[count].copy()
    return part, ops, names, qa, qoff


def _opt(m):
    return _options("blastn", ALL_TAGS, capi.LX_SAM_SEQ_UNIQ, 1, True, m, NS, ref_header=1)


def _args(sub):
    m, ops, names, qa, qoff = sub
    return (m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"]), dict(program="blastn", q_ascii=qa, q_ascii_off=qoff)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_a_header_of_more_than_a_block(handle, tmp_path, case, fmt, count):
    f, sub = FORMATS[fmt], _records(case, count)
    opt, keep = _opt(sub[0])
    m, ops, names, qa, qoff = sub
    assert len(_render(f, "blastn", m[:0], ops, names, qa, qoff, opt)) > BLOCK  # the header alone
    args, kw = _args(sub)
    host, dev = tmp_path / "host.gz", tmp_path / "dev.gz"
    handle.write_records_bgzf(host, f, *args, options=opt, **kw)
    if f == capi.LX_OUT_BAM:
        handle.write_bam(dev, *args, options=opt, **kw)
    else:
        handle.write_text(dev, f, *args, bgzf=True, options=opt, **kw)
    want = host.read_bytes()
    assert dev.read_bytes() == want, (fmt, count, "one shot")
    # the same list as two pieces (one query each) rendered on the device
    assert oc.write_in_pieces(handle, tmp_path / "pieces.gz", f, sub, opt, [1], capi.LX_RENDER_DEV, bgzf=True) == want, (fmt, count, "pieces")


def test_m9_footer_behind_no_record(handle, tmp_path, case):
    sub = _records(case, 0)
    opt, keep = _opt(sub[0])
    args, kw = _args(sub)
    host, dev = tmp_path / "host.gz", tmp_path / "dev.gz"
    handle.write_records_bgzf(host, capi.LX_OUT_BLAST_TAB_COMMENTS, *args, options=opt, footer_records=2, **kw)
    handle.write_text(dev, capi.LX_OUT_BLAST_TAB_COMMENTS, *args, bgzf=True, options=opt, footer_records=2, **kw)
    assert dev.read_bytes() == host.read_bytes()
