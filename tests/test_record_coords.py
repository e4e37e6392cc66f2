"""CPU tests of the host record writer (host/lx_output.cpp) at real subject coordinates, against the independent model of
tests/record_coords.py: the tabular coordinate columns, SAM's POS and CIGAR, BAM's pos, bin and n_cigar_op; the BAM stream decodes to
the SAM text; the file writer writes the rendered bytes; a BAM output refuses a subject BAM cannot hold.  No GPU needed."""
import collections
import ctypes as C

import numpy as np
import pytest

from lambda_amd import capi
from tests import bam_decode, record_coords as rc

M8, M9, SAM, BAM = capi.LX_OUT_BLAST_TAB, capi.LX_OUT_BLAST_TAB_COMMENTS, capi.LX_OUT_SAM, capi.LX_OUT_BAM


def _render(fmt, cases, hard=1, footer=-1):
    opt = rc.options(cases, hard)
    return capi.render_records(fmt, *cases.args(), footer_records=footer, **cases.kw(opt))


# ---- the lists and the model, before any writer is asked

@pytest.mark.parametrize("program", rc.BIN_PROGRAMS)
def test_bin_lists_reach_every_level_the_program_can(program):
    want = rc.models(f"bin_levels-{program}")
    levels = collections.Counter(r["level"] for r in want)
    if program == "tblastn":
        # no CIGAR (src/search_output.hpp:529-531): every record covers one position, which no boundary divides -- only the finest
        # level exists.  The boundaries still separate the bins, and the positions beyond 2^29 still wrap the field.
        assert set(levels) == {5} and all(r["span"] == 1 for r in want)
        assert len({r["bam_bin"] for r in want}) >= 2 * len(rc.SHIFTS)
    else:
        assert all(levels[lv] >= 2 for lv in range(6)), levels
        assert {r["span"] == 1 for r in want} == {True, False} and max(r["n_cigar"] for r in want) > 1000
    wrapped = [r for r in want if r["pos"] >= 2 ** 29]
    assert len(wrapped) >= 4 and any(bam_decode.reg2bin(r["pos"], r["pos"] + r["span"]) > 0xFFFF for r in wrapped)
    assert max(r["pos"] + r["span"] for r in want) == rc.BAM_MAX_REF
    if program == "blastn":
        assert {int(f) for f in rc.lists()[f"bin_levels-{program}"].m["q_frame"]} == {1, -1}


@pytest.mark.parametrize("program", ["tblastn", "tblastx"])
def test_translated_list_crosses_the_sign_change_on_every_minus_frame(program):
    cases, want = rc.lists()[f"translated_subject_pos-{program}"], rc.models(f"translated_subject_pos-{program}")
    assert len(want) == 6 * 7
    by_frame = collections.defaultdict(list)
    for row, r in zip(cases.m, want):
        by_frame[int(row["s_frame"])].append((int(row["s_start"]), r["pos"]))
    for f in rc.FRAMES:
        signs = [p >= 0 for _, p in sorted(by_frame[f])]
        if f > 0:
            assert all(signs) and max(p for _, p in by_frame[f]) == 3 * ((2 ** 31 - 4) // 3) + f - 1
        else:  # 0, 1 .. t - 1 | t, t + 1, 10^6, the last codon
            assert signs == [True] * signs.count(True) + [False] * 4 and signs.count(True) >= 1
            assert min(p for _, p in by_frame[f]) < -(2 ** 31) + 1000  # (still within the 32 bits BAM has)
    assert any(r["pos_text"] in ("0", "-1", "-2") for r in want)


def test_digit_lists_reach_every_power_of_ten():
    for name, top in (("digit_edges-text", 12), ("digit_edges-bam", 9)):
        want = rc.models(name)
        assert {r["pos_text"] for r in want} == {str(v) for k in range(1, top + 1) for v in (10 ** k - 1, 10 ** k)}
        clips = {str(v) for k in range(1, 9) for v in (10 ** k - 1, 10 ** k)}
        for hard, letter in ((1, "H"), (0, "S")):
            texts = [r["cigar_text"] for r in rc.models(name, hard)]
            left = {t[: t.index(letter)] for t in texts}
            right = {t[:-1].rsplit("M", 1)[1] for t in texts}
            assert left == clips and right == clips, (left, right)


@pytest.mark.parametrize("program", ["tblastn", "tblastx"])
def test_the_models_subject_interval_translates_to_the_frames_letters(program):
    cases, dna, frames = rc.untranslate_property(program)
    minus = 0
    for row, r in zip(cases.m, rc.model(cases)):
        frame = frames[rc.FRAMES.index(int(row["s_frame"]))]
        want = frame[int(row["s_start"]): int(row["s_end"])]
        assert len(want) > 0 and (r["sstart"] > r["send"]) == (int(row["s_frame"]) < 0)
        assert np.array_equal(rc.translation_of_interval(dna, r["sstart"], r["send"]), want), (int(row["s_frame"]), r["sstart"], r["send"])
        minus += r["sstart"] > r["send"]
    assert minus == len(cases.m) // 2
    firsts = {(r["sstart"], r["send"]) for r in rc.model(cases)}
    n = rc.SUBJECT_LETTERS
    assert {(1, 3), (2, 4), (3, 5), (n, n - 2), (n - 1, n - 3), (n - 2, n - 4)} <= firsts  # the first codon of each frame


# ---- the host writer against the model

@pytest.mark.parametrize("name", rc.LIST_NAMES)
def test_tabular_coordinates_equal_the_model(name):
    cases = rc.lists()[name]
    rc.assert_m8_equals_model(_render(M8, cases), name)
    m9 = b"".join(line + b"\n" for line in _render(M9, cases).split(b"\n") if line and not line.startswith(b"#"))
    rc.assert_m8_equals_model(m9, name)


@pytest.mark.parametrize("hard", [1, 0])
@pytest.mark.parametrize("name", rc.LIST_NAMES)
def test_sam_pos_and_cigar_equal_the_model(name, hard):
    rc.assert_sam_equals_model(_render(SAM, rc.lists()[name], hard), name, hard)


@pytest.mark.parametrize("hard", [1, 0])
@pytest.mark.parametrize("name", rc.BAM_LIST_NAMES)
def test_bam_pos_bin_and_cigar_count_equal_the_model(name, hard):
    rc.assert_bam_equals_model(_render(BAM, rc.lists()[name], hard), name, hard)


@pytest.mark.parametrize("hard", [1, 0])
@pytest.mark.parametrize("name", rc.BAM_LIST_NAMES)
def test_bam_decodes_to_the_sam_text(name, hard):
    cases = rc.lists()[name]
    assert bam_decode.to_sam(_render(BAM, cases, hard)) == _render(SAM, cases, hard).decode().splitlines()


@pytest.mark.parametrize("fmt,name", [(M8, "bin_levels-blastn"), (M9, "digit_edges-text"), (SAM, "translated_subject_pos-tblastx")])
def test_file_writer_writes_the_rendered_bytes(tmp_path, fmt, name):
    cases = rc.lists()[name]
    opt = rc.options(cases)
    path = tmp_path / "o.txt"
    capi.write_records(path, fmt, *cases.args(), **cases.kw(opt))
    capi.write_footer(path, fmt, len(cases.names["q_ids"]))
    assert path.read_bytes() == _render(fmt, cases, footer=len(cases.names["q_ids"]))


# ---- what BAM cannot hold

def test_bam_refuses_a_subject_of_2_31_letters_and_the_text_formats_do_not():
    cases = rc.lists()["bin_levels-blastx"]
    opt = rc.options(cases)
    s_lens = cases.names["s_lens"].copy()
    s_lens[2] = 2 ** 31
    args = cases.args()[:5] + (s_lens,)
    with pytest.raises(capi.LambdaExtError) as e:
        capi.render_records(BAM, *args, **cases.kw(opt))
    assert e.value.code == capi.LX_EINVAL
    assert '"s2"' in str(e.value) and "2147483648" in str(e.value), str(e.value)
    # (not a matter of the rows: a list without records is refused for its header's reference list)
    with pytest.raises(capi.LambdaExtError) as e:
        capi.render_records(BAM, cases.m[:0], *args[1:], **cases.kw(opt))
    assert e.value.code == capi.LX_EINVAL and '"s2"' in str(e.value)
    for fmt in (M8, M9, SAM):
        assert capi.render_records(fmt, *args, **cases.kw(opt))
    assert b"@SQ\tSN:s2\tLN:2147483648\n" in capi.render_records(SAM, *args, **cases.kw(opt))
    # the longest subject BAM holds
    s_lens[2] = 2 ** 31 - 1
    assert capi.render_records(BAM, *cases.args()[:5], s_lens, **cases.kw(opt)) == _render(BAM, cases)
    # the text formats print what they are given, in 64 bits
    wide = rc.lists()["digit_edges-text"]
    assert b"@SQ\tSN:s0\tLN:10000000000000\n" in _render(SAM, wide)
    lib = capi.load()
    assert lib.lx_check_output_options(BAM, C.byref(opt)) == capi.LX_OK  # (the options alone are still fine)
