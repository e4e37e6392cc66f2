"""GPU tests of the device record writers (lx_text.hip, lx_bam.hip, lx_recdev.h) at real subject coordinates: the lists of
tests/record_coords.py through lx_render_text_dev and lx_render_bam_dev equal the host writer's bytes, and -- so that a restatement
error the host and the device share cannot pass -- the independent model directly, for the tabular coordinates, SAM's POS and CIGAR and
BAM's pos, bin and n_cigar_op.  One list goes through the file writers; a BAM output refuses a subject BAM cannot hold before any
device work."""
import gzip

import pytest

from lambda_amd import capi
from tests import record_coords as rc

pytestmark = pytest.mark.gpu

M8, M9, SAM, BAM = capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS, capi.LX_OUT_SAM, capi.LX_OUT_BAM


@pytest.fixture(scope="module")
def handle():
    with capi.Handle(0) as h:
        yield h


def _host(fmt, cases, opt, footer=-1):
    return capi.render_records(fmt, *cases.args(), footer_records=footer, **cases.kw(opt))


def _same_text(h, fmt, cases, opt, footer=-1):
    dev = h.render_text(fmt, *cases.args(), footer_records=footer, **cases.kw(opt))
    ref = _host(fmt, cases, opt, footer)
    assert dev.split(b"\n") == ref.split(b"\n")  # (the first line that differs reads better than two blobs)
    assert dev == ref
    return dev


@pytest.mark.parametrize("name", rc.LIST_NAMES)
def test_tabular_formats_equal_the_host_writer_and_the_model(handle, name):
    cases = rc.lists()[name]
    opt = rc.options(cases)
    rc.assert_m8_equals_model(_same_text(handle, M8, cases, opt), name)
    m9 = _same_text(handle, M9, cases, opt, footer=len(cases.names["q_ids"]))
    rc.assert_m8_equals_model(b"".join(line + b"\n" for line in m9.split(b"\n") if line and not line.startswith(b"#")), name)


@pytest.mark.parametrize("hard", [1, 0])
@pytest.mark.parametrize("name", rc.LIST_NAMES)
def test_sam_equals_the_host_writer_and_the_model(handle, name, hard):
    cases = rc.lists()[name]
    rc.assert_sam_equals_model(_same_text(handle, SAM, cases, rc.options(cases, hard)), name, hard)


@pytest.mark.parametrize("hard", [1, 0])
@pytest.mark.parametrize("name", rc.BAM_LIST_NAMES)
def test_bam_equals_the_host_writer_and_the_model(handle, name, hard):
    cases = rc.lists()[name]
    opt = rc.options(cases, hard)
    dev = handle.render_bam(*cases.args(), **cases.kw(opt))
    assert dev == _host(BAM, cases, opt)
    rc.assert_bam_equals_model(dev, name, hard)


def test_default_tags_and_no_header(handle):
    """the record kernels alone (no header in front), with the tags a front end asks for by default"""
    cases = rc.lists()["translated_subject_pos-tblastx"]
    opt = rc.options(cases)
    opt.sam_tags = None
    for fmt in (M8, SAM):
        dev = handle.render_text(fmt, *cases.args(), write_header=False, **cases.kw(opt))
        assert dev == capi.render_records(fmt, *cases.args(), write_header=False, **cases.kw(opt))
    rc.assert_sam_equals_model(dev, cases.name, 1)
    dev = handle.render_bam(*cases.args(), write_header=False, **cases.kw(opt))
    assert dev == capi.render_records(BAM, *cases.args(), write_header=False, **cases.kw(opt))


def test_one_list_through_the_file_writers(handle, tmp_path):
    cases = rc.lists()["bin_levels-tblastx"]
    opt = rc.options(cases)
    handle.write_records_bgzf(tmp_path / "host.sam.gz", SAM, *cases.args(), **cases.kw(opt))
    handle.write_text(tmp_path / "dev.sam.gz", SAM, *cases.args(), bgzf=True, **cases.kw(opt))
    raw = (tmp_path / "dev.sam.gz").read_bytes()
    assert raw == (tmp_path / "host.sam.gz").read_bytes()
    sam = gzip.decompress(raw)
    assert sam == _host(SAM, cases, opt)
    rc.assert_sam_equals_model(sam, cases.name, 1)
    handle.write_records_bgzf(tmp_path / "host.bam", BAM, *cases.args(), **cases.kw(opt))
    handle.write_bam(tmp_path / "dev.bam", *cases.args(), **cases.kw(opt))
    raw = (tmp_path / "dev.bam").read_bytes()
    assert raw == (tmp_path / "host.bam").read_bytes()
    rc.assert_bam_equals_model(gzip.decompress(raw), cases.name, 1)


def test_bam_refuses_a_subject_of_2_31_letters_before_any_device_work(tmp_path):
    cases = rc.lists()["bin_levels-blastx"]
    opt = rc.options(cases)
    s_lens = cases.names["s_lens"].copy()
    s_lens[2] = 2 ** 31
    args = cases.args()[:5] + (s_lens,)
    path = tmp_path / "o.bam"
    with capi.Handle(0) as h:  # (a handle of its own: nothing has run on it)
        def refused(call):
            with pytest.raises(capi.LambdaExtError) as e:
                call()
            assert e.value.code == capi.LX_EINVAL and '"s2"' in str(e.value) and "2147483648" in str(e.value), str(e.value)
            assert not path.exists()
            for phase in (4, 11, 12):  # the encoder's kernels, the BAM writer's, the text writer's
                assert h.last_phase_ms(phase) == (0.0, 0)

        refused(lambda: h.render_bam(*args, **cases.kw(opt)))
        refused(lambda: h.write_bam(path, *args, **cases.kw(opt)))
        refused(lambda: h.write_records_bgzf(path, BAM, *args, **cases.kw(opt)))
        refused(lambda: capi.Out(h, path, BAM, args[4], s_lens, program=cases.program, options=opt))
        # the text formats print the length they are given, and the handle is as usable as before
        for fmt in (M8, SAM):
            assert h.render_text(fmt, *args, **cases.kw(opt)) == capi.render_records(fmt, *args, **cases.kw(opt))
        s_lens[2] = 2 ** 31 - 1
        assert h.render_bam(*cases.args()[:5], s_lens, **cases.kw(opt)) == _host(BAM, cases, opt)
        assert h.last_phase_ms(11)[1] > 0
