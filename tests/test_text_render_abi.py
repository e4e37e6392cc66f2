"""CPU tests of the device text writer's boundary: lx_render_text_dev, lx_write_text_dev and lx_format_number are declared, exported and
bound, and both writer entries refuse what they must -- LX_OUT_BAM, an unknown column, a bit score outside the formatter's domain, a row
that names a query the lists do not have, a NULL handle -- with LX_EINVAL and a text, before a file or a device is touched.  The
arguments are judged before the handle, so every refusal shows without a GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from lambda_amd import build, capi
from tests.test_bam_encoding import _case

ROOT = Path(__file__).resolve().parent.parent
NEW = ["lx_render_text_dev", "lx_write_text_dev", "lx_format_number"]


def test_symbols_are_declared_exported_and_bound():
    lib = capi.load()
    header = (ROOT / "include" / "lambda_ext.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", code), name
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    for i, kind in enumerate(["LX_NUM_E1", "LX_NUM_F1", "LX_NUM_F2", "LX_NUM_G_FLOAT"]):
        assert re.search(rf"\b{kind}\s*=\s*{i}\b", code) and getattr(capi, kind) == i
    assert lib.lx_abi_version() == 3
    assert hasattr(capi.Handle, "render_text") and hasattr(capi.Handle, "write_text")
    assert {"lx_text.hip", "lx_text_host.cpp"} <= set(build.HIP_SOURCES)
    assert "lx_render_text_dev" in re.search(r"LX_OPT_BAM_RANGE_BYTES\s*=\s*17,\s*/\*(.*?)\*/", header, flags=re.S).group(1)


def _calls(tmp_path, fmt, m, ops, names, qa, qoff, opt, program="blastn"):
    """Both entries with a NULL handle: (rc, lx_last_output_error()) of each; no file may appear."""
    lib = capi.load()
    args, keep = capi._writer_args(m, ops, names["q_ids"], names["q_lens"], names["s_ids"], names["s_lens"], qa, qoff, opt)
    out = C.c_void_p(1)
    rc1 = lib.lx_render_text_dev(None, fmt, 1, program.encode(), *args[:3], len(ops), *args[3:], -1, C.byref(out))
    t1 = capi.last_output_error()
    assert out.value is None
    res = [(rc1, t1)]
    for bgzf in (0, 1):
        p = tmp_path / f"x{bgzf}.out"
        rc2 = lib.lx_write_text_dev(None, str(p).encode(), fmt, bgzf, program.encode(), *args[:3], len(ops), *args[3:], -1)
        res.append((rc2, capi.last_output_error()))
        assert not p.exists()
    return res


@pytest.fixture(scope="module")
def case():
    return _case("blastn", seed=3)


def test_null_handle_is_refused(tmp_path, case):
    m, ops, names, qa, qoff = case
    for fmt in (capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS, capi.LX_OUT_SAM):
        for rc, text in _calls(tmp_path, fmt, m, ops, names, qa, qoff, None):
            assert rc == capi.LX_EINVAL and "handle is NULL" in text


def test_bam_is_refused_with_a_pointer_to_the_bam_call(tmp_path, case):
    m, ops, names, qa, qoff = case
    for rc, text in _calls(tmp_path, capi.LX_OUT_BAM, m, ops, names, qa, qoff, None):
        assert rc == capi.LX_EINVAL and "lx_render_bam_dev" in text and "lx_write_bam_dev" in text
    for rc, text in _calls(tmp_path, 7, m, ops, names, qa, qoff, None):
        assert rc == capi.LX_EINVAL and "format" in text


def test_unknown_column_and_unknown_tag_are_refused(tmp_path, case):
    m, ops, names, qa, qoff = case
    for fmt in (capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS):
        for rc, text in _calls(tmp_path, fmt, m, ops, names, qa, qoff, capi.output_options(columns="qseqid qseq evalue")):
            assert rc == capi.LX_EINVAL and 'Unknown column specifier "qseq"' in text
    for rc, text in _calls(tmp_path, capi.LX_OUT_SAM, m, ops, names, qa, qoff, capi.output_options(sam_tags="AS zz")):
        assert rc == capi.LX_EINVAL and 'Unknown column specifier "zz"' in text


@pytest.mark.parametrize("field,value", [("bit_score", 1e15), ("bit_score", -1e15), ("bit_score", float("inf")), ("bit_score", float("nan")),
                                         ("identity", float("inf")), ("identity", 1.1e15)])  # (identity is a float: 1e15 itself rounds below)
def test_numbers_outside_the_domain_are_refused(tmp_path, case, field, value):
    m, ops, names, qa, qoff = case
    m = m.copy()
    m[field][len(m) // 2] = value
    for fmt in (capi.LX_OUT_BLAST_TAB, capi.LX_OUT_SAM):
        for rc, text in _calls(tmp_path, fmt, m, ops, names, qa, qoff, None):
            assert rc == capi.LX_EINVAL and "bit_score or identity" in text


def test_largest_numbers_of_the_domain_pass_the_check(tmp_path, case):
    m, ops, names, qa, qoff = case
    m = m.copy()
    m["bit_score"][0] = np.nextafter(1e15, 0.0)
    for rc, text in _calls(tmp_path, capi.LX_OUT_BLAST_TAB, m, ops, names, qa, qoff, None):
        assert rc == capi.LX_EINVAL and "handle is NULL" in text  # (the arguments are fine: only the handle is missing)


def test_rows_beyond_the_name_lists_are_refused(tmp_path, case):
    m, ops, names, qa, qoff = case
    for field, n in (("n_qid", len(names["q_ids"])), ("n_sid", len(names["s_ids"]))):
        bad = m.copy()
        bad[field][-1] = n
        for fmt in (capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS, capi.LX_OUT_SAM):
            for rc, text in _calls(tmp_path, fmt, bad, ops, names, qa, qoff, None):
                assert rc == capi.LX_EINVAL and "name lists do not have" in text


def test_unknown_program_and_missing_names_are_refused(tmp_path, case):
    m, ops, names, qa, qoff = case
    for rc, text in _calls(tmp_path, capi.LX_OUT_BLAST_TAB, m, ops, names, qa, qoff, None, program="blastq"):
        assert rc == capi.LX_EINVAL
    lib = capi.load()
    out = C.c_void_p(1)
    assert lib.lx_render_text_dev(None, capi.LX_OUT_SAM, 1, b"blastn", None, 0, None, 0, None, None, None, None, -1, C.byref(out)) == capi.LX_EINVAL
